"""COCO keypoint evaluation restated in float64: plain numpy with Python loops, written for reading (DESIGN.md section 4,
"Scoring").  It is what the scoring kernel and ``rtpe.scoring`` are compared against, and what the hand-derived cases
of tests/test_scoring_host.py pin first.  Not a test module.

Data: ``gt`` maps an image id to its list of annotation dicts (``keypoints`` 51 values, ``bbox``, ``area``,
``iscrowd``, ``num_keypoints``); ``dt`` maps an image id to ``(people (n, 17, >= 3) float32, scores (n) float32)``, the
output of ``engine.unpack_records``; ``ids`` is the evaluated id set.

``faults``: names of deliberate mistakes, each of which the seeded data of the tests must notice."""
from collections import OrderedDict

import numpy as np

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
THRESHOLDS = np.linspace(.5, .95, 10)
AREA_RANGES = np.array([[0.0, 1e10], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]])
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_DETS = 20
NAMES = ("AP", "Ap .5", "AP .75", "AP (M)", "AP (L)", "AR", "AR .5", "AR .75", "AR (M)", "AR (L)")
FAULTS = ("vars_sigma_squared", "no_half", "no_spacing", "all_joints", "unstable_sort", "max_dets_30",
          "exclusive_bounds", "no_early_stop", "rematch", "side_right")


def stable_descending(values, faults=()):
    """indices by descending value, equal values in input order (with the fault: in reverse input order)"""
    idx = list(range(len(values)))
    if "unstable_sort" in faults:
        idx.reverse()
    return sorted(idx, key=lambda i: -float(values[i]))        # sorted() is stable


def detection_area(person):
    x = person[:, 0].astype(np.float64)
    y = person[:, 1].astype(np.float64)
    return (x.max() - x.min()) * (y.max() - y.min())


def oks(person, ann, faults=()):
    """one detection against one annotation; the sum runs over the joints in order"""
    kp = np.asarray(ann["keypoints"], np.float64)
    xg, yg, vg = kp[0::3], kp[1::3], kp[2::3]
    k1 = int((vg > 0).sum())
    bx, by, bw, bh = [np.float64(v) for v in ann["bbox"]]
    x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
    area = np.float64(ann["area"])
    if "no_spacing" not in faults:
        area = area + np.spacing(1)
    total, count = np.float64(0.0), 0
    for j in range(len(SIGMAS)):
        xd, yd = np.float64(person[j, 0]), np.float64(person[j, 1])
        if k1 > 0:
            if not vg[j] > 0 and "all_joints" not in faults:
                continue
            dx, dy = xd - xg[j], yd - yg[j]
        else:
            dx = max(np.float64(0.0), x0 - xd) + max(np.float64(0.0), xd - x1)
            dy = max(np.float64(0.0), y0 - yd) + max(np.float64(0.0), yd - y1)
        s2 = SIGMAS[j] * 2
        var = SIGMAS[j] * SIGMAS[j] if "vars_sigma_squared" in faults else s2 * s2
        with np.errstate(divide="ignore", invalid="ignore"):
            e = (dx * dx + dy * dy) / var / area
        if "no_half" not in faults:
            e = e / 2
        total = total + np.exp(-e)
        count += 1
    return total / count


def evaluate_image(people, scores, anns, faults=()):
    """the per-image tables: ``order`` (the kept people, by score), ``scores``, ``oks (n_dt, G)``,
    ``matched`` / ``ignored (T, R, n_dt)`` bool, and ``gt_ignored (R, G)``"""
    max_dets = 30 if "max_dets_30" in faults else MAX_DETS
    order = stable_descending(scores, faults)[:max_dets]
    n_dt, n_gt = len(order), len(anns)
    m = np.zeros((n_dt, n_gt), np.float64)
    for d, p in enumerate(order):
        for g, ann in enumerate(anns):
            m[d, g] = oks(people[p], ann, faults)
    areas = [detection_area(people[p]) for p in order]
    T, R = len(THRESHOLDS), len(AREA_RANGES)
    matched = np.zeros((T, R, n_dt), bool)
    ignored = np.zeros((T, R, n_dt), bool)
    gt_ignored = np.zeros((R, n_gt), bool)

    def outside(area, lo, hi):
        if "exclusive_bounds" in faults:
            return area <= lo or area >= hi
        return area < lo or area > hi

    for r, (lo, hi) in enumerate(AREA_RANGES):
        for g, ann in enumerate(anns):
            ignore = bool(ann.get("iscrowd", 0)) or ann["num_keypoints"] == 0
            gt_ignored[r, g] = ignore or outside(ann["area"], lo, hi)
        scan = sorted(range(n_gt), key=lambda g: gt_ignored[r, g])         # stable: non-ignored first
        for t, thr in enumerate(THRESHOLDS):
            taken = [False] * n_gt
            for d in range(n_dt):
                best, hit = min(thr, 1 - 1e-10), -1
                for g in scan:
                    if taken[g] and not anns[g].get("iscrowd", 0) and "rematch" not in faults:
                        continue
                    if hit > -1 and not gt_ignored[r, hit] and gt_ignored[r, g] and "no_early_stop" not in faults:
                        break
                    if m[d, g] < best:
                        continue
                    best, hit = m[d, g], g
                if hit > -1:
                    matched[t, r, d] = True
                    ignored[t, r, d] = gt_ignored[r, hit]
                    taken[hit] = True
                else:
                    ignored[t, r, d] = outside(areas[d], lo, hi)
    return dict(order=order, scores=np.asarray([scores[p] for p in order], np.float32), oks=m, matched=matched,
                ignored=ignored, gt_ignored=gt_ignored)


def accumulate(images, npig, faults=()):
    """``images``: the per-image tables in ascending id order; ``npig (R)``: non-ignored annotations over the whole id
    set.  Returns ``precision (T, 101, R)`` and ``recall (T, R)``, -1 where a range holds no annotation."""
    T, R = len(THRESHOLDS), len(AREA_RANGES)
    precision = -np.ones((T, len(REC_THRS), R))
    recall = -np.ones((T, R))
    scores = np.concatenate([im["scores"] for im in images]) if images else np.zeros(0, np.float32)
    by_score = stable_descending(scores, faults)
    for r in range(R):
        if npig[r] == 0:
            continue
        for t in range(T):
            m = np.concatenate([im["matched"][t, r] for im in images])[by_score] if images else np.zeros(0, bool)
            ig = np.concatenate([im["ignored"][t, r] for im in images])[by_score] if images else np.zeros(0, bool)
            tp = np.cumsum(m & ~ig).astype(np.float64)
            fp = np.cumsum(~m & ~ig).astype(np.float64)
            rc = tp / npig[r]
            pr = tp / (fp + tp + np.spacing(1))
            recall[t, r] = rc[-1] if len(rc) else 0
            for i in range(len(pr) - 1, 0, -1):             # non-increasing from the right
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            q = np.zeros(len(REC_THRS))
            at = np.searchsorted(rc, REC_THRS, side="right" if "side_right" in faults else "left")
            for k, i in enumerate(at):
                if i >= len(pr):
                    break                                   # from the first index past the end onwards: 0
                q[k] = pr[i]
            precision[t, :, r] = q
    return precision, recall


def summarize(precision, recall):
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    stats = [mean(precision[:, :, 0]), mean(precision[0, :, 0]), mean(precision[5, :, 0]), mean(precision[:, :, 1]),
             mean(precision[:, :, 2]), mean(recall[:, 0]), mean(recall[0:1, 0]), mean(recall[5:6, 0]),
             mean(recall[:, 1]), mean(recall[:, 2])]
    return OrderedDict(zip(NAMES, stats))


def evaluate(dt, gt, ids, faults=()):
    """per-image tables of the images of ``ids`` that have a record, ascending, and ``npig``"""
    images, npig = [], np.zeros(len(AREA_RANGES), np.int64)
    for i in sorted(set(int(v) for v in ids)):
        anns = gt.get(i, [])
        people, scores = dt.get(i, (np.zeros((0, 17, 3), np.float32), np.zeros(0, np.float32)))
        im = evaluate_image(people, scores, anns, faults)
        npig += (~im["gt_ignored"]).sum(axis=1)
        if i in dt:
            im["image_id"] = i
            images.append(im)
    return images, npig


def score(dt, gt, ids, faults=()):
    """the ten statistics"""
    images, npig = evaluate(dt, gt, ids, faults)
    return summarize(*accumulate(images, npig, faults))
