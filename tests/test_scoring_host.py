"""CPU tests of the keypoint scoring: the float64 restatement (tests/scoring_restated.py) against hand-derived cases,
the seeded data against seeded faults of the restatement, the data layer of ``rtpe.scoring`` (CSR table, results JSON,
refusals, ABI), and the margin condition under which the GPU tests may ask the kernel's match tables to be equal."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import scoring_restated as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = 17
ALL = ("AP", "Ap .5", "AP .75", "AR", "AR .5", "AR .75")
MED = ("AP (M)", "AR (M)")
LARGE = ("AP (L)", "AR (L)")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


# ---- building blocks, shared with tests/test_scoring_gpu.py -------------------------------------------------------------
def pose(x0=100.0, y0=50.0, dx=10.0, dy=7.0):
    """17 joints on a lattice, exact in float32: x = x0 + dx * j, y = y0 + dy * (j % 5); extent 16 dx by 4 dy
    (the default: 160 x 28, area 4480 - a medium detection)"""
    p = np.zeros((J, 4), np.float32)
    p[:, 0] = x0 + dx * np.arange(J)
    p[:, 1] = y0 + dy * (np.arange(J) % 5)
    p[:, 2] = 1.0
    return p


def ann_of(p, area, v=2, iscrowd=0, bbox=None, num_keypoints=None):
    """an annotation at the joints of person ``p``; ``v``: one value or 17; joints with v == 0 sit at (0, 0)"""
    v = np.broadcast_to(np.asarray(v, np.float64), (J,)).copy()
    kp = np.zeros((J, 3), np.float64)
    kp[:, 0], kp[:, 1], kp[:, 2] = p[:, 0], p[:, 1], v
    kp[v == 0, :2] = 0
    if bbox is None:
        bbox = [float(p[:, 0].min()), float(p[:, 1].min()), float(np.ptp(p[:, 0])), float(np.ptp(p[:, 1]))]
    return {"image_id": None, "category_id": 1, "keypoints": kp.reshape(-1).tolist(), "bbox": list(bbox),
            "area": float(area), "iscrowd": int(iscrowd),
            "num_keypoints": int((v > 0).sum()) if num_keypoints is None else int(num_keypoints)}


def people_of(*ps):
    return np.stack(ps).astype(np.float32) if ps else np.zeros((0, J, 4), np.float32)


def f32(*values):
    return np.array(values, np.float32)


def coco_dict(gt, ids=None):
    """the COCO-format dict of a ``gt`` mapping (image ids from the mapping, or ``ids``)"""
    images = [{"id": int(i)} for i in (gt if ids is None else ids)]
    anns = []
    for i, lst in gt.items():
        for a in lst:
            anns.append(dict(a, image_id=int(i), id=len(anns) + 1))
    return {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}


def hand_cases():
    """name -> (dt, gt, ids, expected statistics); the expected values are derived in the tests' docstrings"""
    one = dict.fromkeys(ALL + MED, 1.0)
    none = dict.fromkeys(LARGE, -1.0)
    cases = {}
    a, b = pose(), pose(300.0, 200.0)
    # every annotation detected exactly, distinct scores; medium annotations only
    cases["exact"] = ({1: (people_of(a, b), f32(.9, .8)), 2: (people_of(b), f32(.7))},
                      {1: [ann_of(a, 5000), ann_of(b, 4000)], 2: [ann_of(b, 5000)]}, [1, 2], dict(one, **none))
    # one annotation of area 5000; score .9 far away, score .8 exact
    cases["fp_first"] = ({1: (people_of(b, a), f32(.9, .8))}, {1: [ann_of(a, 5000)]}, [1],
                         dict({k: 0.5 for k in ("AP", "Ap .5", "AP .75", "AP (M)")}, **{"AR": 1.0, "AR .5": 1.0,
                              "AR .75": 1.0, "AR (M)": 1.0, "AP (L)": -1.0, "AR (L)": -1.0}))
    # two annotations, one exact detection
    half = dict({k: 51 / 101 for k in ("AP", "Ap .5", "AP .75", "AP (M)")},
                **{k: 0.5 for k in ("AR", "AR .5", "AR .75", "AR (M)")})
    cases["one_of_two"] = ({1: (people_of(a), f32(.9))}, {1: [ann_of(a, 5000), ann_of(b, 5000)]}, [1],
                           dict(half, **none))
    # a crowd annotation matched by two detections: neither TP nor FP
    cases["crowd"] = ({1: (people_of(a, b, b), f32(.9, .8, .7))},
                      {1: [ann_of(a, 5000), ann_of(b, 5000, iscrowd=1, num_keypoints=0)]}, [1], dict(one, **none))
    # an unmatched small detection: ignored in `medium`, a false positive in `all`
    small = pose(400.0, 300.0, 1.0, 1.0)                                        # 16 x 4 = 64
    cases["small_unmatched"] = ({1: (people_of(small, a), f32(.95, .9))}, {1: [ann_of(a, 5000)]}, [1],
                                {"AP": 0.5, "Ap .5": 0.5, "AP .75": 0.5, "AP (M)": 1.0, "AP (L)": -1.0, "AR": 1.0,
                                 "AR .5": 1.0, "AR .75": 1.0, "AR (M)": 1.0, "AR (L)": -1.0})
    # an image of the id set without a record: its annotation counts in recall
    cases["no_record"] = ({1: (people_of(a), f32(.9))}, {1: [ann_of(a, 5000)], 2: [ann_of(b, 5000)]}, [1, 2],
                          dict(half, **none))
    return cases


def seeded_set(seed=11):
    """the seeded data of the fault tests and of the GPU tests: ``(dt, gt, ids)``.

    Records with 0, 1, 3, 20, 25 and 30 people; images with 0, 1, 2 and 40 annotations; both k1 branches, crowds, an
    annotation of area 0, areas exactly on range bounds, equal scores at the cut to 20, an image id absent from the
    annotations (77), ids at both ends of the table (3, 99) and an annotated image without a record (60)."""
    rng = np.random.default_rng(seed)

    def random_pose(size):
        cx, cy = rng.uniform(50, 590, 2)
        p = np.zeros((J, 4), np.float32)
        p[:, 0] = cx + rng.uniform(-size / 2, size / 2, J)
        p[:, 1] = cy + rng.uniform(-size / 2, size / 2, J)
        p[:, 2] = rng.random(J)
        return p

    def near(p, area, strength):
        q = p.copy()
        q[:, :2] += rng.normal(0, strength * np.sqrt(area) * 0.1, (J, 2)).astype(np.float32)
        return q

    def random_ann(size_lo, size_hi):
        size = rng.uniform(size_lo, size_hi)
        p = random_pose(size)
        v = rng.integers(0, 3, J)
        v[rng.integers(0, J)] = 2
        return p, ann_of(p, area=float(np.round(size * size * rng.uniform(0.3, 0.6), 2)), v=v)

    gt, dt = {}, {}

    def image(i, n_people, n_ann, size_lo=25.0, size_hi=95.0, extra_anns=(), first_people=()):
        anns, people = list(extra_anns), list(first_people)
        poses, has_record = [], n_people is not None
        n_people = n_people or 0
        while len(anns) < n_ann:
            p, a = random_ann(size_lo, size_hi)
            poses.append((p, a["area"]))
            anns.append(a)
        for p, area in poses:
            if len(people) < n_people:
                people.append(near(p, area, rng.uniform(0.05, 1.2)))
        while len(people) < n_people:
            people.append(random_pose(rng.uniform(20, 200)))
        gt[i] = anns
        if has_record:
            dt[i] = (people_of(*people[:n_people]), rng.random(n_people).astype(np.float32))

    # id 3 (the table's first): A large and B a crowd almost on it; person 0 sits exactly on B (a higher OKS with the
    # ignored B than with A: the scan must stop before B), person 1 near A (only one of the two may have A)
    A = pose(100.0, 100.0, 12.0, 30.0)                                  # 192 x 120
    B = A.copy()
    B[:, 0] += 2.0
    image(3, 3, 2, extra_anns=[ann_of(A, 20000.0), ann_of(B, 20000.0, iscrowd=1, num_keypoints=0)],
          first_people=[B.copy(), near(A, 20000.0, 0.3)])
    dt[3][1][:] = f32(.99, .98, .5)
    # id 10: no people; an annotation of area exactly 1024 (the lower bound of `medium`)
    image(10, 0, 1, extra_anns=[ann_of(pose(50.0, 60.0, 2.0, 8.0), 1024.0)])
    image(11, 1, 0)
    image(12, 20, 40)
    # id 40: 25 people, scores 19 and 20 (by rank) equal: the cut to 20 keeps the first of them
    image(40, 25, 2, size_lo=100.0, size_hi=150.0)
    s = dt[40][1]
    rank = np.argsort(-s, kind="stable")
    s[rank[20]] = s[rank[19]]
    if rank[20] < rank[19]:                                            # (keep the ranks as they were)
        s[rank[19]] = np.nextafter(s[rank[19]], np.float32(2))
    image(41, 30, 40)
    # id 50: an annotation of area 0, 9 of its 17 joints detected exactly (OKS 9/17), the others far away
    Z = pose(300.0, 300.0, 5.0, 5.0)
    zd = Z.copy()
    zd[9:, 0] += 40.0
    image(50, 3, 1, extra_anns=[ann_of(Z, 0.0)], first_people=[zd])
    # id 60: annotated, in the id set, without a record; one area exactly 9216 (`medium` and `large`)
    image(60, None, 2, extra_anns=[ann_of(pose(20.0, 20.0, 9.0, 20.0), 9216.0)])
    # id 77: a record whose image has no entry in the table
    image(77, 3, 0)
    del gt[77]
    # id 99 (the table's last): no visible joint: the bbox branch; the person lies inside the doubled box
    K = pose(200.0, 200.0, 4.0, 6.0)
    image(99, 1, 1, extra_anns=[ann_of(K, 3000.0, v=0, bbox=[190.0, 190.0, 90.0, 50.0])], first_people=[K.copy()])
    ids = sorted(gt)
    return dt, gt, ids


# ---- 1. the restatement against hand-derived cases ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_restatement_on_hand_cases(name):
    """exact: every detection is a true positive, precision 1 at every recall, and no annotation is large.
    fp_first: sorted by score the far detection comes first: tp = [0, 1], fp = [1, 1], precision [0, .5] made
    non-increasing from the right [.5, .5], recall [0, 1]: every recall threshold reads .5, recall ends at 1.
    one_of_two: recall [.5], precision [1]: the 51 thresholds 0 .. .5 read 1, the other 50 read 0.
    crowd: the two detections on the crowd annotation match it (it may be matched again) and are ignored; the crowd
    does not count in npig: one true positive, one annotation.
    small_unmatched: in `medium` the small detection is ignored (precision 1), in `all` it is the first false positive.
    no_record: the second image's annotation is never detected: the numbers of one_of_two."""
    dt, gt, ids, want = hand_cases()[name]
    got = SR.score(dt, gt, ids)
    assert list(got) == list(SR.NAMES)
    for k in SR.NAMES:
        assert abs(got[k] - want[k]) <= 1e-12, (name, k, got[k], want[k])


def test_restatement_crowd_tables():
    dt, gt, ids, _ = hand_cases()["crowd"]
    im = SR.evaluate_image(*dt[1], gt[1])
    assert im["matched"].all()
    assert not im["ignored"][:, :2, 0].any() and im["ignored"][:, :, 1:].all()
    assert im["ignored"][:, 2, 0].all()             # the matched annotation is not large
    assert im["oks"][1, 1] == 1.0 and im["oks"][2, 1] == 1.0


def test_restatement_bbox_branch():
    """num_keypoints == 0: the distance is that to the box doubled about itself ([bx - bw, bx + 2 bw]); inside it every
    term is exp(-0)"""
    p = pose(200.0, 200.0, 4.0, 6.0)                # x 200 .. 264, y 200 .. 224
    a = ann_of(p, 3000.0, v=0, bbox=[190.0, 190.0, 90.0, 50.0])
    assert a["num_keypoints"] == 0
    assert SR.oks(p, a) == 1.0
    far = p.copy()
    far[:, 0] += 300.0                              # x 500 .. 564 > 190 + 180
    assert 0.0 <= SR.oks(far, a) < 1e-6
    edge = p.copy()
    edge[:, 0] = 370.0                              # exactly bx + 2 bw
    assert SR.oks(edge, a) == 1.0
    im = SR.evaluate_image(people_of(p), f32(.5), [a])
    assert im["matched"].all() and im["ignored"].all() and im["gt_ignored"].all()


def test_restatement_cut_and_order():
    """25 people leave the 20 top scores; equal scores keep input order"""
    rng = np.random.default_rng(1)
    people = people_of(*[pose(10.0 * k) for k in range(25)])
    scores = rng.permutation(25).astype(np.float32) / 25
    im = SR.evaluate_image(people, scores, [])
    assert len(im["order"]) == 20 and sorted(scores[im["order"]]) == sorted(np.sort(scores)[5:])
    assert list(im["scores"]) == sorted(im["scores"], reverse=True)
    scores = f32(.5, .7, .5, .7, .5)
    assert SR.evaluate_image(people[:5], scores, [])["order"] == [1, 3, 0, 2, 4]


def test_restatement_range_bounds_are_inclusive():
    p = pose()
    im = SR.evaluate_image(people_of(), f32(), [ann_of(p, 1024.0), ann_of(p, 9216.0), ann_of(p, 1023.99),
                                                ann_of(p, 9216.01)])
    assert im["gt_ignored"].tolist() == [[False, False, False, False], [False, False, True, True],
                                         [True, False, True, False]]


# ---- 2. the seeded data sees seeded faults -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    dt, gt, ids = seeded_set()
    return dt, gt, ids, SR.score(dt, gt, ids)


def test_seeded_set_has_the_shapes_the_kernel_test_needs(seeded):
    dt, gt, ids, stats = seeded
    assert sorted(len(s) for _, s in dt.values()) == [0, 1, 1, 3, 3, 3, 20, 25, 30]
    assert sorted(len(a) for a in gt.values()) == [0, 1, 1, 1, 2, 2, 2, 40, 40]
    assert 77 in dt and 77 not in gt and 60 in gt and 60 not in dt and ids[0] == 3 and ids[-1] == 99
    assert all(-1 < v < 1 for v in stats.values()), stats


@pytest.mark.parametrize("fault", SR.FAULTS)
def test_seeded_set_sees_fault(seeded, fault):
    dt, gt, ids, stats = seeded
    wrong = SR.score(dt, gt, ids, faults=(fault,))
    changed = [k for k in SR.NAMES if wrong[k] != stats[k]]
    print(fault, changed)
    assert changed, fault


# ---- 4. the margin condition of the GPU match-table test -----------------------------------------------------------------
def test_seeded_oks_values_keep_their_distance(seeded):
    """the kernel's OKS may differ from the restatement's by the exp bound (4e-15).  The match
    tables are equal all the same if no value lies within 1e-9 of a threshold, and no two values of one detection
    lie within 1e-9 of each other - except the deliberate exact 1.0 and values below the first threshold less the
    margin, which no comparison of the matching can reach (a value is only ever compared with a running best that is
    at least min(t, 1 - 1e-10) >= .5)."""
    dt, gt, ids, _ = seeded
    images, _ = SR.evaluate(dt, gt, ids)
    checked = 0
    for im in images:
        m = im["oks"]
        assert ((m >= 0) & (m <= 1)).all()
        live = m[(m >= 0.5 - 1e-9) & (m != 1.0)]
        for t in list(SR.THRESHOLDS) + [1 - 1e-10]:
            near_t = np.abs(live - t) < 1e-9
            assert not near_t.any(), (im["image_id"], t, live[near_t])
        for row in m:
            v = np.sort(row[(row >= 0.5 - 1e-9) & (row != 1.0)])
            assert (np.diff(v) >= 1e-9).all(), (im["image_id"], v)
            checked += len(v)
    assert checked >= 20


# ---- 3. data preconditions -----------------------------------------------------------------------------------------------
def test_csr_table_value_for_value():
    from rtpe import scoring
    a, b = pose(), pose(300.0, 200.0)
    gt = {7: [ann_of(a, 5000.0, v=[2, 1, 0] * 5 + [2, 2]), ann_of(b, 77.5, iscrowd=1, num_keypoints=0)], 2: [],
          581929: [ann_of(b, 9216.0, bbox=[1.0, 2.0, 3.0, 4.0])]}
    d = coco_dict(gt)
    d["annotations"].append(dict(ann_of(a, 1.0), image_id=7, category_id=2, id=99))     # not a person
    d["annotations"].append(dict(ann_of(a, 1.0), image_id=12345, id=100))               # not an image of the set
    g = scoring.CocoKeypointGT(d)
    assert g.ids == [7, 2, 581929] and len(g) == 3
    ids, offsets, rows = g.table()
    assert ids.dtype == np.int32 and ids.tolist() == [2, 7, 581929]
    assert offsets.dtype == np.int32 and offsets.tolist() == [0, 0, 2, 3]
    assert rows.dtype == np.float64 and rows.shape == (3, 64)
    first = gt[7][0]
    assert rows[0, :51].tolist() == first["keypoints"] and rows[0, 6:8].tolist() == [0.0, 0.0]
    assert rows[0, 51:55].tolist() == first["bbox"] and rows[0, 55:58].tolist() == [5000.0, 0.0, 12.0]
    assert rows[1, 55:58].tolist() == [77.5, 1.0, 0.0]
    assert rows[2, 51:58].tolist() == [1.0, 2.0, 3.0, 4.0, 9216.0, 0.0, 17.0]
    assert not rows[:, 58:].any()
    assert g.npig().tolist() == [2, 2, 1]
    sub = scoring.CocoKeypointGT(d, image_ids=[581929, 7])
    assert sub.ids == [581929, 7] and sub.table()[0].tolist() == [7, 581929] and sub.table()[1].tolist() == [0, 2, 3]
    for bad in ([], [1, 1], [-1], [(1 << 24) + 1]):
        with pytest.raises(ValueError):
            scoring.CocoKeypointGT(d, image_ids=bad)
    assert scoring.STAT_NAMES == SR.NAMES and scoring.MAX_DETS == SR.MAX_DETS
    assert np.array_equal(scoring.SIGMAS, SR.SIGMAS) and np.array_equal(scoring.THRESHOLDS, SR.THRESHOLDS)
    assert np.array_equal(scoring.AREA_RANGES, SR.AREA_RANGES) and np.array_equal(scoring.REC_THRS, SR.REC_THRS)


def test_json_source_and_results_layout(tmp_path):
    from rtpe import engine, scoring
    a, b = pose(), pose(300.0, 200.0)
    path = tmp_path / "person_keypoints.json"
    path.write_text(json.dumps(coco_dict({5: [ann_of(a, 5000.0)], 6: []})))
    g = scoring.CocoKeypointGT(str(path))
    assert g.ids == [5, 6] and g.table()[1].tolist() == [0, 1, 1]
    rec = engine.pack_records([6, 5], [(people_of(a, b), [np.float32(.75), np.float32(.5)]),
                                       (np.zeros((0,), np.float32), [])], "cpu")
    out = tmp_path / "results.json"
    assert scoring.write_keypoint_results(rec, str(out)) == 2
    text = out.read_text()
    res = json.loads(text)
    assert text == json.dumps(res, sort_keys=True, indent=4)
    assert [sorted(r) for r in res] == [["bbox", "category_id", "image_id", "keypoints", "score"]] * 2
    assert res[0]["image_id"] == 6 and res[0]["category_id"] == 1 and res[0]["score"] == 0.75
    assert res[0]["keypoints"] == a[:, :3].astype(np.float64).reshape(-1).tolist() and len(res[1]["keypoints"]) == 51
    assert res[0]["bbox"] == [100.0, 50.0, 160.0, 28.0] and res[1]["bbox"] == [300.0, 200.0, 160.0, 28.0]
    back = scoring.results_to_records(res)
    assert np.array_equal(back.numpy()[0, :2 + 30], rec.numpy()[0, :2 + 30])
    assert np.array_equal(back.numpy()[0, 32:].reshape(30, 17, 4)[..., :3], rec.numpy()[0, 32:].reshape(30, 17, 4)[..., :3])
    assert scoring.write_keypoint_results(res, str(out)) == 2 and out.read_text() == text


def test_host_accumulation_equals_the_restatement(seeded):
    """``rtpe.scoring.accumulate`` + ``summarize`` on the restatement's match tables give the restatement's numbers,
    for the seeded set and every hand case: what lets the GPU test ask for ``==`` once the tables agree"""
    from rtpe import scoring
    sets = [seeded[:3]] + [c[:3] for c in hand_cases().values()]
    for dt, gt, ids in sets:
        images, npig = SR.evaluate(dt, gt, ids)
        n, T, R, D = len(images), 10, 3, 20
        sc = np.zeros((n, D), np.float32)
        m, ig = np.zeros((n, T, R, D), bool), np.zeros((n, T, R, D), bool)
        for k, im in enumerate(images):
            nd = len(im["order"])
            sc[k, :nd], m[k, :, :, :nd], ig[k, :, :, :nd] = im["scores"], im["matched"], im["ignored"]
        order = np.random.default_rng(0).permutation(n)          # the records come in any order
        got = scoring.summarize(*scoring.accumulate(
            np.array([im["image_id"] for im in images], np.int32)[order],
            np.array([len(im["order"]) for im in images], np.int32)[order], sc[order], m[order], ig[order], npig))
        assert got == SR.score(dt, gt, ids)
        g = scoring.CocoKeypointGT(coco_dict(gt, ids))
        assert g.npig().tolist() == npig.tolist()


def test_parse_result_layout():
    from rtpe import scoring
    T, R, D = 10, 3, 20
    row = np.zeros((2, 1288), np.uint8)
    row[:, :8].view(np.int32)[:] = [[581929, 3], [7, 0]]
    row[0, 8:8 + 12].view(np.float32)[:] = [.75, .5, .25]
    row[0, 88 + (4 * R + 1) * D + 2] = 1
    row[0, 88 + T * R * D + (9 * R + 2) * D + 19] = 1
    ids, n_dt, scores, matched, ignored = scoring.parse_result(row)
    assert ids.tolist() == [581929, 7] and n_dt.tolist() == [3, 0] and scores[0, :4].tolist() == [.75, .5, .25, 0]
    assert matched.sum() == 1 and matched[0, 4, 1, 2] and ignored.sum() == 1 and ignored[0, 9, 2, 19]


def test_scoring_refusals(built):
    from rtpe import engine, scoring
    g = scoring.CocoKeypointGT(coco_dict({1: [ann_of(pose(), 5000.0)]}))
    rec = engine.pack_records([1], [(people_of(pose()), [np.float32(.5)])], "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.score_records(rec, g)
    if not torch.cuda.is_available():           # (evaluate packs on the GPU where there is one)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            g.evaluate([[pose()]], [[.5]], ".", False, False)
    with pytest.raises(ValueError, match="17, >= 4"):
        g.evaluate([[pose()[:16]]], [[.5]], ".", False, False)
    with pytest.raises(ValueError, match="predictions"):
        g.evaluate([[pose()], [pose()]], [[.5], [.5]], ".", False, False)

    L = built.lib()
    fake = ctypes.c_void_p(0x1000)
    rb, sb = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.rtpe_oks_eval_bytes(5, 83, 10, 3, 20, ctypes.byref(rb), ctypes.byref(sb)) == 0
    assert rb.value == 5 * 1288 and sb.value == 83 * (160 + 4 + 30) + 2 and sb.value % 8 == 0
    assert L.rtpe_oks_eval_bytes(1, 0, 1, 1, 1, ctypes.byref(rb), ctypes.byref(sb)) == 0
    assert rb.value == 16 and sb.value == 16
    for bad in ((0, 83, 10, 3, 20), (5, -1, 10, 3, 20), (5, 83, 0, 3, 20), (5, 83, 10, 0, 20), (5, 83, 10, 3, 0),
                (5, 83, 10, 3, 65), (5, 83, 10, 17, 20)):
        assert L.rtpe_oks_eval_bytes(*bad, ctypes.byref(rb), ctypes.byref(sb)) < 0, bad
        assert b"oks_eval_bytes" in L.rtpe_last_error_string()
    assert L.rtpe_oks_eval_bytes(5, 83, 10, 3, 20, None, ctypes.byref(sb)) < 0

    good = dict(rec=fake, n=5, J=17, P=30, ids=fake, off=fake, rows=fake, n_img=4, sig=fake, thr=fake, T=10, rng=fake,
                R=3, D=20, result=fake, rb=5 * 1288, scratch=fake, sb=83 * 194 + 6, stream=None)

    def call(**kw):
        return L.rtpe_oks_eval(*dict(good, **kw).values())
    for kw in ([{k: None} for k in ("rec", "ids", "off", "rows", "sig", "thr", "rng", "result", "scratch")] +
               [{k: v} for k in ("n", "J", "P", "n_img", "T", "R", "D") for v in (0, -1)] +
               [dict(D=31), dict(D=65, P=80), dict(R=17), dict(J=18), dict(rb=5 * 1288 - 1), dict(rb=0), dict(sb=0),
                dict(sb=193), dict(result=ctypes.c_void_p(0x1004)), dict(scratch=ctypes.c_void_p(0x1002))]):
        assert call(**kw) < 0, kw
        assert b"oks_eval" in L.rtpe_last_error_string(), kw
    assert call(D=31) < 0 and b"exceeds max_people" in L.rtpe_last_error_string()
    assert call(rb=8) < 0 and b"result of 8 bytes" in L.rtpe_last_error_string()


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_oks_symbols_are_declared_and_resolve(built):
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_oks.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_oks.h")))
    assert declared == {"rtpe_oks_eval_bytes", "rtpe_oks_eval"} == set(built.EXPORTS_OKS)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR,
             built.EXPORTS_RECORDS, built.EXPORTS_TAGMEAN, built.EXPORTS_NOPROJ, built.EXPORTS_ANYSIZE,
             built.EXPORTS_MIXED, built.EXPORTS_MIXDEC, built.EXPORTS_TRACE, built.EXPORTS_MIXAUX, built.EXPORTS_FRAMES)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6, 5, 4, 4, 4, 2, 1, 3]
    for table in older:
        assert not declared & set(table)
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_OKS[name][1], name
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "rtpe_hip_oks.h")).read()
    for macro, value in (("RTPE_OKS_GT_ROW", built.OKS_GT_ROW), ("RTPE_OKS_MAX_DETS", built.OKS_MAX_DETS),
                         ("RTPE_OKS_MAX_RANGES", built.OKS_MAX_RANGES), ("RTPE_OKS_LDS_DOUBLES", built.OKS_LDS_DOUBLES)):
        assert re.search(r"#define %s (\d+)" % macro, hdr).group(1) == str(value)
    # the 40-annotation case of the GPU test exceeds the LDS budget, the 2-annotation ones do not
    assert 20 * 40 > built.OKS_LDS_DOUBLES >= 20 * 20
