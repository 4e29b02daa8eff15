"""COCO keypoint scoring of the device-resident records: the last stage behind ``gather``.

``score_records(rec, gt)`` turns the record tensor that ``TeacherPipeline.gather`` / ``__call__(..., image_ids=...)``
returned into the ten statistics the reference's ``eval_student`` reports (``COCODataset._do_python_keypoint_eval``):
one launch of the scoring kernel (csrc/oks_eval.hip: score order, OKS in float64, greedy matching at ten thresholds and
three area ranges, one workgroup per record), one read-back of its compact result table, and the precision / recall
accumulation in numpy float64 on the host.  The rules are pycocotools' ``COCOeval`` for ``iouType="keypoints"``
restated ("Scoring"); pycocotools itself is not a dependency.

``CocoKeypointGT`` holds the annotations; it has the reference dataset's ``evaluate`` signature, so a loader whose
``.dataset`` is one makes ``engine.eval_student`` return the reference's dict.  ``evaluate`` writes no file (the
reference always writes ``results/keypoints_*_results.json``); ``write_keypoint_results`` writes that file on request.
"""
import ctypes
import json
from collections import OrderedDict

import numpy as np
import torch

from . import _native
from .engine import MAX_PEOPLE_RECORD, NUM_HEATMAPS, RECORD_FLOATS, pack_records, unpack_records

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
THRESHOLDS = np.linspace(.5, .95, 10)
AREA_RANGES = np.array([[0.0, 1e10], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]])       # all, medium, large; inclusive
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_DETS = 20
STAT_NAMES = ("AP", "Ap .5", "AP .75", "AP (M)", "AP (L)", "AR", "AR .5", "AR .75", "AR (M)", "AR (L)")
GT_ROW = _native.OKS_GT_ROW
PERSON = 1          # COCO's category id


def _is_ignored(ann):
    return bool(ann.get("iscrowd", 0)) or ann["num_keypoints"] == 0


class CocoKeypointGT:
    """the person keypoint annotations of a COCO-format dict or JSON file.

    ``ids``: the evaluated id set - ``image_ids`` in the order given, or all images of the source; recall counts the
    annotations of every one of them, whether an image has a record or not.  ``anns[id]``: its annotation dicts in
    source order.  ``to(device)`` builds the CSR table the kernel reads, once per device."""

    def __init__(self, source, image_ids=None):
        if not isinstance(source, dict):
            with open(source) as f:
                source = json.load(f)
        if image_ids is None:
            image_ids = [im["id"] for im in source.get("images", [])]
        self.ids = [int(i) for i in image_ids]
        if not self.ids:
            raise ValueError("CocoKeypointGT: no images to evaluate")
        if len(set(self.ids)) != len(self.ids):
            raise ValueError("CocoKeypointGT: an image id occurs twice")
        if min(self.ids) < 0 or max(self.ids) > 1 << 24:
            raise ValueError("CocoKeypointGT: image ids must lie in [0, 2**24] (a float32 record holds them exactly)")
        self.anns = {i: [] for i in self.ids}
        for ann in source.get("annotations", []):
            if ann.get("category_id", PERSON) != PERSON or ann["image_id"] not in self.anns:
                continue
            if len(ann["keypoints"]) != 3 * NUM_HEATMAPS:
                raise ValueError("CocoKeypointGT: an annotation with %d keypoint values, 51 are needed"
                                 % len(ann["keypoints"]))
            self.anns[ann["image_id"]].append(ann)
        self._tables = {}

    def __len__(self):
        return len(self.ids)

    def table(self):
        """the CSR table on the host: ``ids (n) i32`` ascending, ``offsets (n + 1) i32``, ``rows (total, 64) f64`` =
        51 keypoint values, bbox at 51..54, area at 55, iscrowd at 56, num_keypoints at 57, zeros"""
        ids = np.array(sorted(self.ids), np.int32)
        counts = [len(self.anns[int(i)]) for i in ids]
        offsets = np.zeros(len(ids) + 1, np.int32)
        offsets[1:] = np.cumsum(counts)
        rows = np.zeros((int(offsets[-1]), GT_ROW), np.float64)
        k = 0
        for i in ids:
            for ann in self.anns[int(i)]:
                rows[k, :51] = ann["keypoints"]
                rows[k, 51:55] = ann["bbox"]
                rows[k, 55], rows[k, 56], rows[k, 57] = ann["area"], ann.get("iscrowd", 0), ann["num_keypoints"]
                k += 1
        return ids, offsets, rows

    def npig(self):
        """non-ignored annotations per area range over the whole id set"""
        n = np.zeros(len(AREA_RANGES), np.int64)
        for anns in self.anns.values():
            for ann in anns:
                for r, (lo, hi) in enumerate(AREA_RANGES):
                    n[r] += not (_is_ignored(ann) or ann["area"] < lo or ann["area"] > hi)
        return n

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._tables:
            ids, offsets, rows = self.table()
            if not len(rows):
                rows = np.zeros((1, GT_ROW), np.float64)        # (a pointer the entry accepts; no offset reaches it)
            self._tables[device] = dict(
                ids=torch.from_numpy(ids).to(device), offsets=torch.from_numpy(offsets).to(device),
                rows=torch.from_numpy(rows).to(device), total=int(offsets[-1]),
                sigmas=torch.from_numpy(SIGMAS).to(device), thresholds=torch.from_numpy(THRESHOLDS).to(device),
                ranges=torch.from_numpy(AREA_RANGES).to(device))
        return self._tables[device]

    def evaluate(self, preds, scores, output_dir, dataset_with_center, test_ignore_center):
        """the reference's ``COCODataset.evaluate``: ``preds[i]`` (a list of (joints, >= 4) people) and ``scores[i]``
        belong to ``self.ids[i]``; returns ``(OrderedDict of the ten statistics, AP)``.  ``output_dir`` is not used:
        no results file is written."""
        if len(preds) != len(scores) or len(preds) > len(self.ids):
            raise ValueError("CocoKeypointGT.evaluate: %d predictions, %d score lists, %d images"
                             % (len(preds), len(scores), len(self.ids)))
        results = []
        for people, sc in zip(preds, scores):
            people = [np.asarray(p, np.float32) for p in people]
            if dataset_with_center and not test_ignore_center:
                people = [p[:-1] for p in people]
            if any(p.shape[0] != NUM_HEATMAPS or p.shape[1] < 4 for p in people):
                raise ValueError("CocoKeypointGT.evaluate: a person is (17, >= 4): x, y, value, tag per joint")
            results.append((np.stack(people) if people else np.zeros((0,), np.float32), list(sc)))
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        stats = score_records(pack_records(self.ids[:len(results)], results, device), self)
        return stats, stats["AP"]


def _launch(rec, gt, max_dets=MAX_DETS, result=None, scratch=None):
    """the one launch: ``(result (n, row_bytes) uint8, scratch uint8, table)`` on the device of ``rec``; ``result`` and
    ``scratch``: contiguous uint8 tensors of the sizes of ``rtpe_oks_eval_bytes`` to write into (fresh ones otherwise)"""
    _native.require_gpu(rec, "score_records")
    if rec.dim() != 2 or rec.shape[1] != RECORD_FLOATS or rec.dtype != torch.float32 or not rec.shape[0]:
        raise ValueError("score_records: a record tensor is (n >= 1, %d) float32, not %s %s"
                         % (RECORD_FLOATS, tuple(rec.shape), rec.dtype))
    rec = rec.contiguous()
    tab = gt.to(rec.device)
    L = _native.lib()
    n, T, R = rec.shape[0], len(THRESHOLDS), len(AREA_RANGES)
    rb, sb = ctypes.c_size_t(), ctypes.c_size_t()
    _native.check(L.rtpe_oks_eval_bytes(n, tab["total"], T, R, max_dets, ctypes.byref(rb), ctypes.byref(sb)))
    if result is None:
        result = torch.empty((n, rb.value // n), dtype=torch.uint8, device=rec.device)
    if scratch is None:
        scratch = torch.empty((sb.value,), dtype=torch.uint8, device=rec.device)
    for name, t, size in (("result", result, rb.value), ("scratch", scratch, sb.value)):
        if t.dtype != torch.uint8 or t.device != rec.device or not t.is_contiguous() or t.numel() != size:
            raise ValueError("score_records: %s must be %d contiguous uint8 on %s" % (name, size, rec.device))
    with _native.on_device(rec):
        _native.check(L.rtpe_oks_eval(
            rec.data_ptr(), n, NUM_HEATMAPS, MAX_PEOPLE_RECORD, tab["ids"].data_ptr(), tab["offsets"].data_ptr(),
            tab["rows"].data_ptr(), len(gt.ids), tab["sigmas"].data_ptr(), tab["thresholds"].data_ptr(), T,
            tab["ranges"].data_ptr(), R, max_dets, result.data_ptr(), rb.value, scratch.data_ptr(), sb.value,
            _native.stream_ptr(rec.device)))
    return result.view(n, -1), scratch, tab


def parse_result(table, max_dets=MAX_DETS):
    """the result table (n, row_bytes) uint8 on the host -> ``ids (n) i32, n_dt (n) i32, scores (n, D) f32,
    matched (n, T, R, D) bool, ignored (n, T, R, D) bool``"""
    table = np.ascontiguousarray(table)
    n, T, R, D = table.shape[0], len(THRESHOLDS), len(AREA_RANGES), max_dets
    head = table[:, :8].copy().view(np.int32)
    scores = table[:, 8:8 + 4 * D].copy().view(np.float32)
    cells = T * R * D
    o = 8 + 4 * D
    matched = table[:, o:o + cells].reshape(n, T, R, D) != 0
    ignored = table[:, o + cells:o + 2 * cells].reshape(n, T, R, D) != 0
    return head[:, 0], head[:, 1], scores, matched, ignored


def accumulate(ids, n_dt, scores, matched, ignored, npig):
    """precision ``(T, 101, R)`` and recall ``(T, R)`` from the per-record tables, -1 where a range holds no
    annotation: the records in ascending id order, all detections by descending score (stable), cumulative true and
    false positives, precision made non-increasing from the right and sampled at the 101 recall thresholds"""
    T, R = len(THRESHOLDS), len(AREA_RANGES)
    precision = -np.ones((T, len(REC_THRS), R))
    recall = -np.ones((T, R))
    by_id = np.argsort(ids, kind="stable")
    keep = np.arange(scores.shape[1])[None, :] < n_dt[by_id, None]             # (n, D)
    sc = scores[by_id][keep]
    by_score = np.argsort(-sc, kind="stable")
    for r in range(R):
        if npig[r] == 0:
            continue
        for t in range(T):
            m = matched[by_id, t, r][keep][by_score]
            ig = ignored[by_id, t, r][keep][by_score]
            tp = np.cumsum(m & ~ig).astype(np.float64)
            fp = np.cumsum(~m & ~ig).astype(np.float64)
            rc = tp / npig[r]
            pr = tp / (fp + tp + np.spacing(1))
            recall[t, r] = rc[-1] if len(rc) else 0
            pr = np.maximum.accumulate(pr[::-1])[::-1]
            at = np.searchsorted(rc, REC_THRS, side="left")
            q = np.zeros(len(REC_THRS))
            inside = at < len(pr)               # rc ascends, so do the indices: past the end from one point onwards
            q[inside] = pr[at[inside]]
            precision[t, :, r] = q
    return precision, recall


def summarize(precision, recall):
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    stats = [mean(precision[:, :, 0]), mean(precision[0, :, 0]), mean(precision[5, :, 0]), mean(precision[:, :, 1]),
             mean(precision[:, :, 2]), mean(recall[:, 0]), mean(recall[0:1, 0]), mean(recall[5:6, 0]),
             mean(recall[:, 1]), mean(recall[:, 2])]
    return OrderedDict(zip(STAT_NAMES, stats))


def score_records(rec, gt):
    """the ten COCO keypoint statistics of a record tensor against ``gt`` (a ``CocoKeypointGT``): one launch, one
    read-back of the result table, the accumulation on the host.  Records whose image is not in ``gt.ids`` are not
    evaluated; two records of one image are a ValueError."""
    result, _, _ = _launch(rec, gt)
    ids, n_dt, scores, matched, ignored = parse_result(result.cpu().numpy())
    if len(np.unique(ids)) != len(ids):
        twice = sorted(int(i) for i in set(ids.tolist()) if (ids == i).sum() > 1)
        raise ValueError("score_records: image id(s) %s occur in more than one record" % twice[:8])
    evaluated = np.isin(ids, np.array(gt.ids, np.int32))
    return summarize(*accumulate(ids[evaluated], n_dt[evaluated], scores[evaluated], matched[evaluated],
                                 ignored[evaluated], gt.npig()))


def records_to_results(rec):
    """the reference's result dicts (``_coco_keypoint_results_one_category_kernel``) of a record tensor, host only"""
    out = []
    for image_id, (people, scores) in unpack_records(rec).items():
        for kp, s in zip(people, scores):
            xy = kp[:, :3].astype(np.float64)
            left_top, right_bottom = xy.min(axis=0), xy.max(axis=0)
            out.append({"image_id": int(image_id), "category_id": PERSON, "keypoints": [float(v) for v in xy.reshape(-1)],
                        "score": float(s), "bbox": [float(left_top[0]), float(left_top[1]),
                                                    float(right_bottom[0] - left_top[0]),
                                                    float(right_bottom[1] - left_top[1])]})
    return out


def results_to_records(results, device="cpu"):
    """a record tensor from result dicts (a results JSON): people per image in file order; a record holds 30 people,
    so an image with more keeps its 30 best (stable by descending score, in the order the evaluation ranks them)"""
    per = OrderedDict()
    for res in results:
        if res.get("category_id", PERSON) != PERSON:
            continue
        kp = np.zeros((NUM_HEATMAPS, 4), np.float32)
        kp[:, :3] = np.asarray(res["keypoints"], np.float32).reshape(NUM_HEATMAPS, 3)
        people, scores = per.setdefault(int(res["image_id"]), ([], []))
        people.append(kp)
        scores.append(np.float32(res["score"]))
    packed = []
    for people, scores in per.values():
        if len(people) > MAX_PEOPLE_RECORD:
            best = np.argsort(-np.asarray(scores, np.float32), kind="stable")[:MAX_PEOPLE_RECORD]
            people, scores = [people[k] for k in best], [scores[k] for k in best]
        packed.append((np.stack(people), scores))
    return pack_records(list(per), packed, device)


def write_keypoint_results(rec_or_results, path):
    """the reference's results JSON (``image_id``, ``category_id`` 1, 51 keypoint floats, ``score``, ``bbox``; sorted
    keys, indent 4) from a record tensor or a list of result dicts.  Host only."""
    results = records_to_results(rec_or_results) if torch.is_tensor(rec_or_results) else list(rec_or_results)
    with open(path, "w") as f:
        json.dump(results, f, sort_keys=True, indent=4)
    return len(results)
