"""Decode inputs for every tag dimension D and for the rare branches of refine, with the structures built in and the
counters that prove they are there (oracle; test infrastructure only, see oracle/__init__.py).

The HIP decode restates numpy's float orders, and they are keyed on D: a float32 mean tag summed pairwise for D == 1
and sequentially otherwise; squared tag distances summed sequentially for D < 8 and in numpy's 8-accumulator pairwise
walk (block loop, tree, tail) from 8 on; float64 distances in the matcher with the same split.  Blob maps do not see
an order - their tags are 3 apart, no distance lies near a half-integer - so the scenes here put tags ON the rounding
boundary: a seeded search finds, per D, pixel tags whose rounded distance to a person's mean differs between the
reference's order and a named wrong one (``decode_ref.FAULTS``), and the heat values are laid out so that the arg-max
pixel differs with it.  Nothing is trusted: every scene has a ``*_structure`` function that COUNTS, on the oracle's CPU
result, what the scene exists for, and the tests assert those counts before they compare anything.

    a  ``blob_cases``       blobs at every D of ``DIMS`` for the full parse (one case with ONE tag map for all joints)
    b  ``boundary_scene``   refine penalties on the rounding boundary, per D of ``(2,) + DIMS``
    c  ``people_scene``     40 and 530 people of one image missing one joint, 200 / 0 / 330 over three images,
                            J = 32 with D = 32, J = 1
    d  ``overflow_scene``   D = 1, every squared distance of a plane overflows
    e  ``foreign_rows``     scene b's people with tag columns that are not the map's values
    f  ``match_cases``      matcher tables at every D, with threshold decisions engineered on the summation order
    g  ``wide_inputs``      network-shaped maps decoded at 16 x 2112: wider than the 2,048 columns one block of the
                            plane-maximum pass owns
"""
import hashlib

import numpy as np
import torch

from . import decode_ref, synth

f32 = np.float32
DIMS = (3, 7, 8, 9, 16, 17, 32)
DIMS_ALL = (1, 2) + DIMS
BOUNDARY_DIMS = (2,) + DIMS
REFINE_GROUP, SCAN_PEOPLE = 16, 512          # csrc/decode.hip kRefineGroup; the people one trip of refine's scan lists
ARGMAX_WIDTH = 2048                          # 256 threads x 8 columns of the plane-maximum pass on fused maps
BATCH_FAULTS = ("first512", "slot16")        # seeded faults of ``refine_rows`` on top of decode_ref.FAULTS
_REF = decode_ref.HeatmapParserRef


def digest(a):
    """sha-256 over dtype, shape and bytes of an array (-0 folded onto +0): the fixture records the bulky results of
    the reference - tag columns are random float32 - as digests, which equal iff the arrays are bit-equal"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a + a.dtype.type(0)
    h = hashlib.sha256(("%s %s " % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def pack_results(arrays):
    """many small arrays as a handful (a zip member costs more than most of them): names, dtypes, shapes, and one
    flat array per dtype with the values in the order of the sorted names"""
    names = sorted(arrays)
    vals = [np.asarray(arrays[k]) for k in names]
    out = {"names": np.array(names), "dtypes": np.array([v.dtype.str for v in vals]),
           "ndims": np.array([v.ndim for v in vals], np.int32),
           "shapes": np.array([n for v in vals for n in v.shape], np.int32)}
    for dt in sorted({v.dtype.str for v in vals}):
        out["data_" + dt.strip("<|>=")] = np.concatenate([v.reshape(-1) for v in vals if v.dtype.str == dt])
    return out


def unpack_results(g):
    shapes, at, res, used = g["shapes"], 0, {}, {}
    for name, dt, nd in zip(g["names"], g["dtypes"], g["ndims"]):
        shape = tuple(int(n) for n in shapes[at:at + nd])
        at += nd
        n = int(np.prod(shape))
        key = "data_" + str(dt).strip("<|>=")
        o = used.get(key, 0)
        res[str(name)] = g[key][o:o + n].reshape(shape)
        used[key] = o + n
    return res


# --------------------------------------------------------------------------- #
# a. blobs at every D
# --------------------------------------------------------------------------- #
def blob_cases():
    cases = []
    for D in DIMS:
        cases.append(dict(name="p4_d%d" % D, persons=4, h=48, w=64, seed=300 + D, D=D, tag_per_joint=True))
        cases.append(dict(name="p6_d%d" % D, persons=6, h=40, w=72, seed=400 + D, D=D, tag_per_joint=True))
    cases.append(dict(name="p4_d3_shared", persons=4, h=48, w=64, seed=350, D=3, tag_per_joint=False))
    return cases


def blob_maps(c):
    """det (1,17,h,w), tag (1,17,h,w,D) - or (1,1,h,w,D), one map for all joints - as torch tensors"""
    det, tag = synth.make_decode_maps(c["persons"], c["h"], c["w"], c["seed"], sigma=1.5, tag_dim=c["D"])
    if not c["tag_per_joint"]:
        tag = np.ascontiguousarray(tag.max(axis=1, keepdims=True))
    return torch.from_numpy(det), torch.from_numpy(tag)


def blob_parser(c, cls=_REF, **kw):
    return cls(17, 30, 0.1, 1.0, True, False, c["tag_per_joint"], 5, 2, **kw)


def blob_structure(c, tk, adjusted, final):
    """people found, live candidates and joints that refine filled"""
    return {"people": len(final), "live": int((tk["val_k"] > 0.1).sum()), "tag_dim": tk["tag_k"].shape[3],
            "filled": int(((adjusted[:, :, 2] == 0) & (final[:, :, 2] > 0)).sum())}


# --------------------------------------------------------------------------- #
# refine over the rows of a batch (what rtpe_adjust_refine does), with the seeded faults
# --------------------------------------------------------------------------- #
def refine_rows(s, fault=None, do_adjust=False, do_refine=True):
    """adjust / refine of every person of a scene ``s`` (det (N,J,h,w), tag (N,J,h,w,D), rows (P,J,3+D), pimg (P))
    by the oracle.  ``fault``: one of decode_ref.FAULTS, or
      first512  only the first 512 people of an image are refined
      slot16    among the people of an image that miss joint j, number i is scored against the mean tag of number
                i + 16 (where there is one)"""
    det, tag, rows, pimg = s["det"], s["tag"], s["rows"], s["pimg"]
    J = det.shape[1]
    hp = _REF(num_joints=J)
    out = rows.copy()
    if do_adjust:
        for p in range(len(out)):
            hp.adjust([out[p:p + 1]], det[pimg[p]:pimg[p] + 1])
    if not do_refine:
        return out
    inner = fault if fault in decode_ref.FAULTS else None
    local = np.concatenate([np.arange(int((pimg == n).sum())) for n in range(det.shape[0])]) if len(out) else []
    means = [None] * len(out)
    if fault == "slot16":
        own = [hp.refine_mean(tag[pimg[p]], rows[p]) if (rows[p, :, 2] > 0).any() else None for p in range(len(out))]
        means = [[own[p]] * J for p in range(len(out))]
        for n in range(det.shape[0]):
            for j in range(J):
                need = [p for p in np.flatnonzero(pimg == n) if rows[p, j, 2] == 0]
                for i, p in enumerate(need[:-REFINE_GROUP] if len(need) > REFINE_GROUP else []):
                    means[p][j] = own[need[i + REFINE_GROUP]]
    for p in range(len(out)):
        if fault == "first512" and local[p] >= SCAN_PEOPLE:
            continue
        if not (rows[p, :, 2] == 0).any():
            continue
        out[p] = hp.refine(det[pimg[p]], tag[pimg[p]], out[p], inner, means[p])
    return out


# --------------------------------------------------------------------------- #
# b. refine penalties on the rounding boundary
# --------------------------------------------------------------------------- #
ORDER_FAULTS = ("sequential", "float64", "fma", "no_tail", "pairwise_mean")
B_HW, B_J, B_FOUND = (24, 40), 17, 8
# (fault, direction) of the missing planes 8..16.  Direction 1: the reference's order rounds the penalty of the
# highest pixel DOWN and the wrong one up; direction 2: the reverse.  Person A's pixels carry the plane maximum (the
# arg-max shortcut evaluates them, then the scan), person B's lie below it (the scan alone).  Dropping the tail only
# ever lowers a sum, so "no_tail" has direction 2 alone.
_PLAN_A = [("sequential", 1), ("sequential", 2), ("float64", 1), ("float64", 2), ("fma", 1), ("fma", 2),
           ("pairwise_mean", 1), ("no_tail", 2), ("pairwise_mean", 2)]
_PLAN_B = [("pairwise_mean", 1), ("pairwise_mean", 2), ("no_tail", 2), ("sequential", 2), ("fma", 2), ("fma", 1),
           ("float64", 2), ("float64", 1), ("sequential", 1)]


def fault_applies(fault, D):
    return {"sequential": D >= 8, "float64": True, "fma": D != 8 and D > 1, "no_tail": D >= 8 and D % 8 != 0,
            "pairwise_mean": D > 1}[fault]


def _penalty(t, mean, fault=None):
    """rounded tag distance of the tags t (N,D) to ``mean`` under the reference's order or a wrong one"""
    return -_REF.refine_score(np.zeros((1, len(t)), f32), np.ascontiguousarray(t[None], f32), mean, fault)[0]


def _find_tag(rng, mean, mean_wrong, fault, k, direction):
    """a tag at distance k + 0.5 of ``mean`` (a random direction, one coordinate moved by up to three ulps) whose
    penalty the reference's order rounds to k and the wrong order (``fault`` on the sum, or the mean ``mean_wrong``)
    to k + 1 - direction 2: the reverse"""
    D = len(mean)
    for _ in range(800):
        u = rng.normal(size=(256, D))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        t = np.repeat((mean + u * (k + 0.5)).astype(f32), 7, axis=0)
        c = rng.integers(0, D)
        t[:, c] = (t[:, c].view(np.int32) + np.tile(np.arange(-3, 4, dtype=np.int32), 256)).view(f32)
        right, wrong = _penalty(t, mean), _penalty(t, mean_wrong, fault)
        hit = (right == k) & (wrong == k + 1) if direction == 1 else (right == k + 1) & (wrong == k)
        if hit.any():
            return t[int(np.argmax(hit))]
    return None


def boundary_scene(D, seed=0):
    """one image, J = 17, 24 x 40, two people A and B with joints 0..7 found and 8..16 missing.  Per missing plane and
    person: X1, a pixel with the tag ``mean + v`` (``_find_tag``) and X2, a lower pixel with the person's mean tag
    (penalty 0), with heat values H1 = H2 + k + 0.5: with the penalty k at X1 the arg-max is X1, with k + 1 it is X2.
    A's pair carries the plane maximum (k = 0, H = 4.5 / 4.0), B's lies below (k in 1..3, H2 = 0.5).  The background
    is >= 50 away from both means in every coordinate.  The 8 found tags of a person are drawn until their
    sequential and pairwise float32 means differ.  Returns the scene with ``plan``: (person, plane, fault, direction)
    of every engineered pair."""
    h, w = B_HW
    rng = np.random.default_rng(7000 + 37 * D + seed)
    det = (rng.integers(0, 64, (1, B_J, h, w)) / 256.0).astype(f32)                # [0, 0.25)
    tag = (-50 - rng.integers(0, 80, (1, B_J, h, w, D)) / 8.0).astype(f32)
    rows = np.zeros((2, B_J, 3 + D), f32)
    means, wrong_means = [], []
    for p in range(2):
        while True:
            found = (3 + 16 * p + rng.uniform(0, 2, D)[None] + rng.normal(0, 0.05, (B_FOUND, D))).astype(f32)
            for j in range(B_FOUND):
                y, x = 2 + 4 * p, 2 + 4 * j
                det[0, j, y, x] = 1.0 - p / 8.0
                tag[0, j, y, x] = found[j]
                rows[p, j] = np.concatenate(([x, y, det[0, j, y, x]], found[j]))
            m = _REF.refine_mean(tag[0], rows[p])
            mw = _REF.refine_mean(tag[0], rows[p], "pairwise_mean")
            if D == 1 or (m != mw).any():
                break
        means.append(m)
        wrong_means.append(mw)
    plan = []
    pix = (((12, 5), (14, 9)), ((18, 25), (20, 33)))                              # (X1, X2) of A and of B
    for i, j in enumerate(range(B_FOUND, B_J)):
        for p, (fault, direction) in enumerate((_PLAN_A[i], _PLAN_B[i])):
            k = 0 if p == 0 else 1 + (i + D) % 3
            h2 = 4.0 if p == 0 else 0.5
            t = None
            if fault_applies(fault, D):
                t = _find_tag(rng, means[p], wrong_means[p] if fault == "pairwise_mean" else means[p],
                              None if fault == "pairwise_mean" else fault, k, direction)
            if t is not None:
                plan.append((p, j, fault, direction))
            (y1, x1), (y2, x2) = pix[p]
            det[0, j, y1, x1], det[0, j, y2, x2] = h2 + k + 0.5, h2
            tag[0, j, y1, x1] = means[p] if t is None else t
            tag[0, j, y2, x2] = means[p]
    return dict(det=det, tag=tag, rows=rows, pimg=np.zeros(2, np.int32), plan=plan, D=D)


def boundary_structure(s):
    """per (fault, direction): the engineered pairs whose refined row under the wrong order differs from the
    reference's; "at_maximum": those of them that carry the plane maximum"""
    right = refine_rows(s)
    counts = {(f, d): 0 for f in ORDER_FAULTS for d in (1, 2)}
    at_max = {f: 0 for f in ORDER_FAULTS}
    cache = {}
    for p, j, fault, direction in s["plan"]:
        if fault not in cache:
            cache[fault] = refine_rows(s, fault)
        if not np.array_equal(cache[fault][p, j], right[p, j]):
            counts[fault, direction] += 1
            at_max[fault] += int(p == 0)
    return {"pairs": counts, "at_maximum": at_max, "filled": int((right[:, :, 2] > 0).sum() - (s["rows"][:, :, 2] > 0).sum())}


# --------------------------------------------------------------------------- #
# c. groups and people
# --------------------------------------------------------------------------- #
C_HW = (12, 20)
_SHARED = 222                                # pixels the first 512 people of an image share; the rest: one each


def _pixel(q):
    """the pixel of person number q of an image: beyond 512 a pixel of their own"""
    return (q * 7) % _SHARED if q < SCAN_PEOPLE else _SHARED + (q - SCAN_PEOPLE)


def people_scene(counts, D, J=4, found=None):
    """``counts[n]`` people in image n of (N, J, 12, 20) maps, joints ``found..J-1`` missing (default: the last one).
    Pixel i carries the tag 4 i + 1 (+ d in coordinate d) on every plane and the heat 0.25 + i / 1024 (+ n / 8 in
    image n); person q of an image was found at pixel ``_pixel(q)``, so on a missing plane that pixel is the only one
    with penalty 0 (every other is >= 4 away) and the answer of a person is its own pixel's."""
    h, w = C_HW
    found = J - 1 if found is None else found
    N = len(counts)
    i = np.arange(h * w)
    det = np.broadcast_to((0.25 + i / 1024.0).reshape(1, 1, h, w), (N, J, h, w)).astype(f32)
    det = det + (np.arange(N) / 8.0).astype(f32).reshape(N, 1, 1, 1)
    tag = np.broadcast_to((4.0 * i + 1).reshape(1, 1, h, w, 1) + np.arange(D), (N, J, h, w, D)).astype(f32)
    rows, pimg = [], []
    for n, c in enumerate(counts):
        for q in range(c):
            y, x = divmod(_pixel(q), w)
            r = np.zeros((J, 3 + D), f32)
            r[:found, 0], r[:found, 1], r[:found, 2] = x, y, det[n, 0, y, x]
            r[:found, 3:] = tag[n, 0, y, x]
            rows.append(r)
            pimg.append(n)
    return dict(det=np.ascontiguousarray(det), tag=np.ascontiguousarray(tag), rows=np.array(rows, f32),
                pimg=np.array(pimg, np.int32), D=D, counts=tuple(counts), found=found)


def people_structure(s):
    """on the oracle's rows: people that miss a joint per image, passes of 16 and trips of 512 they make, and how many
    people beyond the first 512 of an image have an answer no other person of the image has"""
    out = refine_rows(s)
    J, found = s["det"].shape[1], s["found"]
    res = {"missing": [], "passes": [], "trips": [], "beyond_unique": 0, "filled": 0}
    for n, c in enumerate(s["counts"]):
        mine = out[s["pimg"] == n]
        miss = int((s["rows"][s["pimg"] == n][:, J - 1, 2] == 0).sum()) if found < J else 0
        res["missing"].append(miss)
        res["passes"].append(-(-miss // REFINE_GROUP))
        res["trips"].append(-(-c // SCAN_PEOPLE))
        if found < J:
            res["filled"] += int((mine[:, found:, 2] > 0).sum())
            ans = [tuple(r[J - 1, :3]) for r in mine]
            res["beyond_unique"] += sum(ans.count(a) == 1 for a in ans[SCAN_PEOPLE:])
    return res


PEOPLE_SCENES = {                           # name -> (counts, D, J, found)
    "c40_d1": ((40,), 1, 4, None), "c40_d3": ((40,), 3, 4, None),
    "c530_d1": ((530,), 1, 4, None), "c530_d3": ((530,), 3, 4, None),
    "c3img_d1": ((200, 0, 330), 1, 4, None), "c3img_d3": ((200, 0, 330), 3, 4, None),
    "j32_d32": ((3,), 32, 32, 16), "j1_d1": ((3,), 1, 1, 1), "j1_d3": ((3,), 3, 1, 1),
}


def people_case(name):
    counts, D, J, found = PEOPLE_SCENES[name]
    return people_scene(counts, D, J, found)


# --------------------------------------------------------------------------- #
# d. overflow
# --------------------------------------------------------------------------- #
def overflow_scene():
    """D = 1, (1, 4, 12, 20), one person found on planes 0..2 with the tag 2^66.  On plane 3 EVERY pixel is at least
    2^64 from it (2^70 at pixel 0, then 0, 2^65, 2^67, 2^68 in turn), so every squared distance overflows: the
    reference's scores are all -inf and its arg-max is pixel 0.  ``round(|d|)`` without the exact expression is finite
    and takes the first pixel with the smallest distance, a 2^65 one.  Heat values are finite and positive."""
    h, w = C_HW
    rng = np.random.default_rng(66)
    det = (0.25 + rng.integers(0, 128, (1, 4, h, w)) / 256.0).astype(f32)
    tag = np.full((1, 4, h, w, 1), 2.0 ** 66, f32)
    cyc = np.array([0.0, 2.0 ** 65, 2.0 ** 67, 2.0 ** 68], f32)
    tag[0, 3, :, :, 0] = cyc[np.arange(h * w) % 4].reshape(h, w)
    tag[0, 3, 0, 0, 0] = 2.0 ** 70
    rows = np.zeros((1, 4, 4), f32)
    for j in range(3):
        y, x = 5, 3 + 4 * j
        rows[0, j] = (x, y, det[0, j, y, x], 2.0 ** 66)
    return dict(det=det, tag=tag, rows=rows, pimg=np.zeros(1, np.int32), D=1)


def overflow_structure(s):
    with np.errstate(over="ignore"):
        d = s["tag"][0, 3, :, :, 0] - f32(2.0 ** 66)
        sq = d * d
    out, fast = refine_rows(s), refine_rows(s, "no_fallback")
    return {"overflowed": int(np.isinf(sq).sum()), "pixels": int(sq.size), "magnitudes": len(np.unique(np.abs(d))),
            "finite_heat": bool(np.isfinite(s["det"]).all()), "pixel0": bool(out[0, 3, 0] < 1 and out[0, 3, 1] < 1),
            "fast_differs": not np.array_equal(out, fast), "no_nan": not np.isnan(out).any()}


# --------------------------------------------------------------------------- #
# e. refine with tag columns that are not the map's
# --------------------------------------------------------------------------- #
FOREIGN = ("zeros", "other", "half")


def foreign_rows(s, kind):
    """scene b's people with columns 3.. replaced: zeros, the OTHER person's tags, the map's values rounded to fp16.
    The reference takes the mean tag from the map and hands the caller's columns back untouched."""
    rows = s["rows"].copy()
    if kind == "zeros":
        rows[:, :, 3:] = 0
    elif kind == "other":
        rows[:, :, 3:] = s["rows"][::-1, :, 3:]
    else:
        rows[:, :, 3:] = s["rows"][:, :, 3:].astype(np.float16).astype(f32)
    return dict(s, rows=rows)


# --------------------------------------------------------------------------- #
# f. matcher tables
# --------------------------------------------------------------------------- #
F_J, F_K = 17, 30
F_CFGS = ((30, 0.1, 1.0, True, False), (8, 0.1, 1.0, True, False))   # max_num_people, det thr, tag thr, use val, ignore


def _table(tags, vals):
    """(J, K) candidate tables from per-joint lists of tags and values; the other slots are below the threshold"""
    D = len(tags[0][0])
    tag = np.zeros((F_J, F_K, D), f32)
    val = np.zeros((F_J, F_K), f32)
    loc = np.zeros((F_J, F_K, 2), np.int64)
    for j, (tj, vj) in enumerate(zip(tags, vals)):
        tag[j, :len(tj)], val[j, :len(tj)] = tj, vj
        loc[j, :len(tj), 0], loc[j, :len(tj), 1] = 10 * j + np.arange(len(tj)), 3 * j
    return tag, loc, val


def _dist64(t, c, sequential=False):
    d = t.astype(np.float64) - c.astype(np.float64)
    return float(np.sqrt(decode_ref._sum_last_f64((d * d)[None], sequential)[0]))


def _engineered_distance(D, rng):
    """five people founded by joint 0, five candidates of joint 1 each 0.5 from its person; the threshold is the
    larger of candidate 0's two float64 distances (sequential, numpy pairwise), which differ"""
    while True:
        c = (rng.normal(0, 10, (5, D))).astype(f32)
        u = rng.normal(size=(5, D))
        t = (c + 0.5 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(f32)
        a, b = _dist64(t[0], c[0]), _dist64(t[0], c[0], True)
        if a != b:
            v = (0.9 - np.arange(5) / 16.0).astype(f32)
            return _table([c, t], [v, v]), max(a, b)


def _engineered_centre(D, rng):
    """three people, each with one candidate 0.3 away on joints 0..8 (all join); on joint 9 person 0's candidate lies
    0.9 from its centre, the float32 mean of nine tags, whose sequential and pairwise sums differ; the threshold is
    the larger of the candidate's distances to the two"""
    while True:
        c = (rng.normal(0, 10, (3, D))).astype(f32)
        tags = []
        for j in range(10):
            u = rng.normal(size=(3, D))
            tags.append((c + (0.9 if j == 9 else 0.3) * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(f32))
        mine = [tags[j][0] for j in range(9)]
        m, mw = decode_ref._mean_tags_f32(mine), decode_ref._mean_tags_f32(mine, True)
        a, b = _dist64(tags[9][0], m), _dist64(tags[9][0], mw)
        if a != b:
            v = (0.9 - np.arange(3) / 16.0).astype(f32)
            return _table(tags, [v] * 10), max(a, b)


def match_cases():
    """(name, cfg, tag (J,K,D), loc (J,K,2), val (J,K)): per D of DIMS two random tables in the style of the matcher
    tests under two parameter sets; per D >= 8 the two engineered tables, the cost being the distance"""
    cases = []
    for D in DIMS:
        rng = np.random.default_rng(900 + D)
        for trial in range(2):
            val = np.sort(rng.random((F_J, F_K)).astype(f32) * (0.3 if trial else 1.0), axis=1)[:, ::-1]
            loc = rng.integers(0, 640, (F_J, F_K, 2)).astype(np.int64)
            tag = (rng.integers(0, 6, (F_J, F_K, D)) * 1.5 + rng.normal(0, 0.3, (F_J, F_K, D))).astype(f32)
            for cfg in F_CFGS:
                cases.append(("rand_d%d_t%d_mp%d" % (D, trial, cfg[0]), cfg, tag, loc, np.ascontiguousarray(val)))
        if D >= 8:
            for kind, make in (("dist", _engineered_distance), ("centre", _engineered_centre)):
                (tag, loc, val), thr = make(D, rng)
                cases.append(("%s_d%d" % (kind, D), (30, 0.1, thr, False, False), tag, loc, val))
    return cases


def match_params(cfg):
    return decode_ref.Params(F_J, *cfg)


def match_structure(case):
    """engineered tables: 1 if the wrong order named by the table changes the people, else 0"""
    name, cfg, tag, loc, val = case
    fault = {"dist": "sequential", "centre": "pairwise_mean"}.get(name.split("_")[0])
    if fault is None:
        return 0
    right = decode_ref.match_by_tag(tag, loc, val, match_params(cfg))
    wrong = decode_ref.match_by_tag(tag, loc, val, match_params(cfg), fault)
    return int(right.shape != wrong.shape or not np.array_equal(right, wrong))


# --------------------------------------------------------------------------- #
# g. fused maps wider than 2,048 pixels
# --------------------------------------------------------------------------- #
WIDE_HW = (16, 2112)


def wide_inputs():
    """refined (1,17,8,264), tags (1,17,4,132) torch tensors.  Three people, each in a third of the width with the
    tag 3, 6 or 9 there; person p has a peak on every plane but 5 + p and 6.  Plane 5 (A misses it) has its maximum
    at B's peak - penalty 3 for A: the full scan; plane 6 (everybody misses it) has nothing but a weak maximum of 0.09
    (below the detection threshold) in B's third - penalty 0 for B: the shortcut; 3 for A and C: the full scan."""
    rng = np.random.default_rng(2112)
    refined = (rng.random((1, 17, 8, 264)) * 0.03).astype(f32)
    tags = np.zeros((1, 17, 4, 132), f32)
    for p in range(3):
        tags[0, :, :, 44 * p:44 * (p + 1)] = 3.0 * (p + 1)
        for j in range(17):
            if j == 5 + p:
                continue
            refined[0, j, 2 + 2 * p, 88 * p + 20 + 2 * j] = 0.9 - p / 16.0 - j / 64.0
    refined[0, 6] = np.minimum(refined[0, 6], 0.03)            # plane 6: nobody's peak ...
    refined[0, 6, 5, 88 + 50] = 0.09                            # ... but a weak maximum in B's third
    return torch.from_numpy(refined), torch.from_numpy(tags)


def wide_maps():
    """the maps the fused path never builds: ``upsample_bilinear`` of ``wide_inputs`` to 16 x 2112"""
    refined, tags = wide_inputs()
    return (decode_ref.upsample_bilinear(refined, *WIDE_HW),
            decode_ref.upsample_bilinear(tags, *WIDE_HW).unsqueeze(-1))


def wide_structure(hms, aes, adjusted):
    """per (person, missing joint) of the adjusted people: is the penalty at the plane's first maximum zero (the
    shortcut answers) or not (the full scan does)"""
    det, tag = hms[0].numpy(), aes[0].numpy()
    res = {"width": det.shape[2], "people": len(adjusted), "shortcut": 0, "scan": 0}
    for kp in adjusted:
        mean = _REF.refine_mean(tag, kp)
        for j in np.flatnonzero(kp[:, 2] == 0):
            y, x = divmod(int(np.argmax(det[j])), det.shape[2])
            pen = _penalty(tag[j, y, x][None], mean)[0]
            res["shortcut" if pen == 0 else "scan"] += 1
    return res
