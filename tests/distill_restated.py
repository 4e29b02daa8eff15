"""The distillation targets and losses restated in numpy, for reading ("Distillation targets and
losses").  float32 where the reference computes in float32 (every map, resize, normalisation and product: these are
compared bit for bit), float64 with an exactly rounded sum for the loss values (compared within a derived bound).

``fault=`` switches in one deliberate mistake; tests/test_distill_host.py shows that the test data sees each of them.
"""
import math

import numpy as np

f32 = np.float32
SMALL_OUTPUT = 128          # out_h + out_w up to which PyTorch-CPU resizes with its small-output kernel


# --------------------------------------------------------------------------- ground-truth maps
def patch_table(sigma):
    """(S, S) float64, S = len(arange(0, 6 sigma + 3)): a Gaussian around (3 sigma + 1, 3 sigma + 1)"""
    x = np.arange(0, 6 * sigma + 3, 1, float)
    y = x[:, None]
    c = 3 * sigma + 1
    return np.exp(-((x - c) ** 2 + (y - c) ** 2) / (2 * sigma ** 2))


def _rint(v, fault):
    if fault == "half_up":
        return int(math.floor(v + 0.5))
    return int(np.round(v))                     # half to even, in float64


def gt_heatmaps(people, num_joints, hw, sigma, fault=None):
    """(J, H, W) float32 from an iterable of (J, 3) people: per joint with v > 0 the patch is stamped with `maximum`
    into the window [rint(c - 3 sigma - 1), rint(c + 3 sigma + 2)) around c = int(p), clipped to the image"""
    H, W = hw
    g = patch_table(sigma)
    out = np.zeros((num_joints, H, W), f32)
    for person in people:
        for j in range(num_joints):
            px, py, v = (float(t) for t in person[j][:3])
            if not v > 0:
                continue
            x, y = (math.floor(px), math.floor(py)) if fault == "floor" else (int(px), int(py))
            if x < 0 or y < 0 or x >= W or y >= H:
                continue
            ulx, uly = _rint(x - 3 * sigma - 1, fault), _rint(y - 3 * sigma - 1, fault)
            brx, bry = _rint(x + 3 * sigma + 2, fault), _rint(y + 3 * sigma + 2, fault)
            x0, x1 = max(0, ulx), min(brx, W)
            y0, y1 = max(0, uly), min(bry, H)
            src = g[y0 - uly:y1 - uly, x0 - ulx:x1 - ulx]
            if fault == "unclipped":            # the patch is not cut where the image cuts the window at the left / top
                src = g[:y1 - y0, :x1 - x0]
            dst = out[j, y0:y1, x0:x1]
            dst[...] = dst + src.astype(f32) if fault == "sum" else np.maximum(dst, src)
    return out


# --------------------------------------------------------------------------- resizes
def _fma(a, b, c):
    """fused multiply-add in float32: the product of two float32 is exact in float64, the sum rounds once on the cast"""
    return (np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64)
            + np.asarray(c, f32).astype(np.float64)).astype(f32)


def axis(n_in, n_out, align_corners):
    """source indices i0, i1 and weights l0, l1 of one axis of a bilinear resize, PyTorch-CPU's float32 arithmetic"""
    if n_in == n_out:
        i = np.arange(n_out)
        return i, i.copy(), np.ones(n_out, f32), np.zeros(n_out, f32)
    o = np.arange(n_out).astype(f32)
    if align_corners:
        scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
        real = (scale * o).astype(f32)
    else:
        scale = f32(n_in) / f32(n_out)
        real = np.maximum(_fma(np.full(n_out, scale, f32), o + f32(0.5), np.full(n_out, -0.5, f32)), f32(0))
    i0 = np.minimum(real.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(real - i0.astype(f32), 0, 1).astype(f32)
    return i0, i1, (f32(1) - l1).astype(f32), l1


def resize(x, hw, align_corners, fault=None):
    """``F.interpolate(x, hw, mode="bilinear", align_corners=...)`` of a float32 (N, C, H, W) array on PyTorch-CPU: a
    copy when the sizes agree; the generic kernel's ``fma(fma(v00, lx0, v01 lx1), ly0, fma(v10, lx0, v11 lx1) ly1)``;
    or, when out_h + out_w <= 128, the small-output kernel, which multiplies the weights first and adds the four products
    in one order for the channels of full vectors of 16 and in another for the C % 16 channels behind them"""
    x = np.asarray(x, f32)
    if fault == "align":
        align_corners = not align_corners
    C, (H, W), (h, w) = x.shape[1], x.shape[2:], hw
    if (H, W) == (h, w):
        return x.copy()
    y0, y1, ly0, ly1 = axis(H, h, align_corners)
    x0, x1, lx0, lx1 = axis(W, w, align_corners)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    r0, r1 = x[:, :, y0, :], x[:, :, y1, :]
    v00, v01, v10, v11 = r0[..., x0], r0[..., x1], r1[..., x0], r1[..., x1]
    if h + w > SMALL_OUTPUT:
        return _fma(_fma(v00, lx0, v01 * lx1), ly0, _fma(v10, lx0, v11 * lx1) * ly1)
    w00, w01, w10, w11 = ly0 * lx0, ly0 * lx1, ly1 * lx0, ly1 * lx1
    out = _fma(w00, v00, _fma(w01, v01, _fma(w11, v11, w10 * v10)))
    k = C - (C & 15)
    out[:, k:] = _fma(w11, v11, _fma(w10, v10, _fma(w00, v00, w01 * v01)))[:, k:]
    return out


def targets(people_per_image, num_joints, image_hw, det_hw, att_hw=None, teacher=None, mask=None, segm=None, sigma=2.0,
            fault=None):
    """the two-step chain of the reference's dataset and training step: dict of ``gt`` and ``teacher`` (N, J, h, w),
    ``mask`` (N, 1, h, w), ``segm`` (N, 1, ha, wa), ``minmax`` (4,) - None for what was not given.
    ``teacher``: (N, J, ht, wt), resized per image to the image size with align_corners=True, as the dataset does."""
    out = dict(gt=None, teacher=None, mask=None, segm=None)
    if people_per_image is not None:
        maps = np.stack([gt_heatmaps(p, num_joints, image_hw, sigma) for p in people_per_image])
        out["gt"] = resize(maps, det_hw, False, "align" if fault == "align_stage2" else None)
    if teacher is not None:
        at_image = np.concatenate([resize(t[None], image_hw, True, "align" if fault == "align_stage1" else None)
                                   for t in np.asarray(teacher, f32)])
        out["teacher"] = resize(at_image, det_hw, False, "align" if fault == "align_stage2" else None)
    if mask is not None:
        out["mask"] = resize(np.asarray(mask, f32)[:, None], det_hw, False)
    if segm is not None:
        out["segm"] = resize(np.asarray(segm, f32)[:, None], att_hw, False)
    mm = np.zeros(4, f32)
    if out["gt"] is not None:
        mm[0], mm[1] = out["gt"].min(), out["gt"].max()
    if out["teacher"] is not None:
        mm[2], mm[3] = out["teacher"].min(), out["teacher"].max()
    out["minmax"] = mm
    return out


# --------------------------------------------------------------------------- normalisation and losses
def _unit(t, fault):
    """minus the minimum if negative, then over the maximum if above 1: float32, over the whole tensor"""
    t = np.asarray(t, f32)
    if fault == "per_image":
        return np.stack([_unit(u, None) for u in t])
    if t.min() < 0:
        t = t - t.min()
    if t.max() > 1:
        t = t / t.max()
    return t


def normalise(gt, teacher, mask, background_factor, unit=True, fault=None):
    """steps 1 and 2: ``(gt, teacher, effective mask)``; the mask (N, 1 or J, h, w) comes back as (N, J, h, w), None
    stays None.  No argument is written."""
    gt = np.asarray(gt, f32)
    teacher = None if teacher is None else np.asarray(teacher, f32)
    background = gt == 0
    if unit:
        gt = _unit(gt, fault)
        teacher = None if teacher is None else _unit(teacher, fault)
    if fault != "background_first":
        background = gt == 0
    if mask is not None:
        mask = np.broadcast_to(np.asarray(mask, f32), gt.shape).copy()
        mask[background] *= f32(background_factor)
    return gt, teacher, mask


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _mean(terms, keep=None):
    terms = terms.ravel() if keep is None else terms[keep]
    return math.fsum(terms.tolist()) / terms.size          # the float64 sum rounded once


def loss_terms(pred, target, mask, kind, pos_weight=1.0, fault=None):
    """the elements of one masked loss in float64 from the float32 products; BCE-with-logits as
    ``(1 - y) softplus(x) + pos_weight y softplus(-x)``, which has no cancellation and no negative term for y in [0, 1]"""
    pred, target = np.asarray(pred, f32), np.asarray(target, f32)
    if mask is not None:
        pred, target = pred * mask, target * mask
    x, y = pred.astype(np.float64), target.astype(np.float64)
    if kind == "mse":
        return (x - y) ** 2
    pw = float(f32(pos_weight))
    if fault == "pos_weight":
        return pw * (1.0 - y) * _softplus(x) + y * _softplus(-x)
    return (1.0 - y) * _softplus(x) + pw * y * _softplus(-x)


def distillation_loss(pred, teacher, gt, alpha=0.5, mask=None, background_factor=1.0, kind="bce", teacher_pos_weight=1.0,
                      gt_pos_weight=1.0, unit=None, fault=None):
    """``(teacher_loss, gt_loss, mixed)`` as Python floats (float64).  ``pred`` may carry more channels than the
    targets.  ``unit``: normalise the targets first; by default for ``kind="bce"`` only, as the reference's classes do."""
    gt = np.asarray(gt, f32)
    pred = np.asarray(pred, f32)[:, :gt.shape[1]]
    unit = kind == "bce" if unit is None else unit
    gt, teacher, mask = normalise(gt, teacher, mask, background_factor, unit, fault)
    keep = None
    if fault == "drop_masked" and mask is not None:
        keep = mask != 0
    lt = 0.0 if teacher is None else _mean(loss_terms(pred, teacher, mask, kind, teacher_pos_weight, fault), keep)
    lg = _mean(loss_terms(pred, gt, mask, kind, gt_pos_weight, fault), keep)
    if fault == "alpha":
        alpha = 1.0 - alpha
    return lt, lg, alpha * lt + (1.0 - alpha) * lg


def reduction_depth(n, threads=256, max_blocks=256):
    """additions on the longest path of the device's float64 sum of n elements: a thread's run, six wave steps, the
    waves of a workgroup, the workgroups in index order"""
    blocks = min(-(-n // threads), max_blocks)
    return -(-n // (blocks * threads)) + 6 + threads // 64 + blocks


def loss_bound(n):
    """relative bound on the distance between the device's float64 loss and this restatement:
    in units of 2^-52, per element 6 on the device (exp within 1 ulp, log1p within 2, six roundings of half an ulp
    around them) and 8 here (numpy's vector exp and log1p allowed 2 and 3), 5 on either side for the mean and the mix;
    the device's sum adds half a unit per level of its reduction, the restatement's sum is exact.  Relative bounds add
    because every element term is >= 0 (targets in [0, 1], or squares)."""
    return (24 + 0.5 * reduction_depth(n)) * 2.0 ** -52


# --------------------------------------------------------------------------- the test data (tools/gen_golden_distill.py
# runs the reference on it and writes tests/golden/distill.npz; the tests run this restatement and the device on it)
GT_SIGMAS = (0.5, 1.0, 1.5, 2.0)
GT_SHAPES = ((17, (37, 53)), (3, (8, 8)), (17, (8, 8)), (3, (37, 53)))
CROWD = 70                  # people of the third image: two LDS chunks of 64 on the device


def gt_scene(J, hw, seed=0):
    """the people of four images as (P, J, 3) arrays: the edge cases (one labelled joint per person), nobody, a crowd
    of 70, and a pair"""
    H, W = hw
    rng = np.random.default_rng([seed, J, H, W])
    inside = min(12.99, W - 2.01)
    marks = [(0, 0, 0, 1), (1, W - 1, H - 1, 2),                # the two corners
             (2, W, 3, 1), (0, 4, -1.0, 1),                     # outside: right of the image, above it
             (1, -0.5, -0.9, 1),                                # truncates to (0, 0): inside
             (2, inside, 2.5, 1), (0, 3, 3, 0),                 # a fraction that truncates; not labelled
             (1, 5, 5, 1), (1, 6, 5, 1),                        # two people whose windows overlap on one joint
             (2, W - 1, 0, 1), (0, 0, H - 1, 1)]                # the other two corners
    edges = np.zeros((len(marks), J, 3))
    for p, (j, x, y, v) in enumerate(marks):
        edges[p, j % J] = (x, y, v)

    def crowd(P):
        a = np.empty((P, J, 3))
        a[..., 0] = rng.uniform(-2, W + 2, (P, J))
        a[..., 1] = rng.uniform(-2, H + 2, (P, J))
        a[..., 2] = rng.integers(0, 3, (P, J))
        return a
    return [edges, np.zeros((0, J, 3)), crowd(CROWD), crowd(2)]


# (image, detection grid, attention grid, teacher source): the ceil grid, the identity, an upscale, one pixel - each with
# the teacher at its own size and at the image's; the last case leaves PyTorch's small-output kernel on both stages
TARGET_CASES = tuple(((37, 53), det, att, src)
                     for det, att in (((10, 14), (19, 27)), ((37, 53), (37, 53)), ((40, 60), (80, 120)), ((1, 1), (2, 3)))
                     for src in ((19, 27), (37, 53))) + (((20, 120), (3, 130), (5, 124), (19, 27)),)
TARGET_J = 17


def target_inputs(case, seed=1):
    """people, teacher (4, 17, ht, wt), mask and segm (4, H, W) of one case"""
    (H, W), _, _, (ht, wt) = case
    rng = np.random.default_rng([seed, H, W, ht, wt])
    teacher = rng.normal(0.2, 0.4, (4, TARGET_J, ht, wt)).astype(f32)
    planes = []
    for _ in range(2):
        m = np.ones((4, H, W), f32)
        for n in range(4):
            y, x = rng.integers(0, H - 3), rng.integers(0, W - 3)
            m[n, y:y + rng.integers(2, H), x:x + rng.integers(2, W)] = 0
        planes.append(m)
    return gt_scene(TARGET_J, (H, W)), teacher, planes[0], 1 - planes[1]


LOSS_SHAPES = ((2, 17, 10, 14), (1, 1, 1, 1), (3, 17, 33, 35))
LOSS_MODES = ("both", "neither")            # the targets need both normalisations (gt above 1, below 0) / neither
LOSS_MASKS = ("none", "n1", "nj")           # absent, (N, 1, h, w), (N, J, h, w); with "n1" pred has J + 1 channels
LOSS_KINDS = ("bce", "mse")
LOSS_PARAMS = ((0.0, 0.5, 1.0), (0.25, 0.0, 7.0), (1.0, 1.0, 7.0), (0.25, 0.5, 7.0))   # background_factor, alpha, pos_weight


def loss_pos_weights(pw):
    """(teacher_pos_weight, gt_pos_weight): different, so that the two cannot be exchanged unseen"""
    return pw, 8.0 - pw


def loss_inputs(shape, mode, mask_mode, seed=2):
    """pred (N, J or J + 1, h, w), teacher, gt, mask of one case, float32"""
    N, J, h, w = shape
    rng = np.random.default_rng([seed, N, J, h, w, LOSS_MODES.index(mode), LOSS_MASKS.index(mask_mode)])
    blobs = rng.random(shape) ** 4
    blobs[rng.random(shape) < 0.5] = 0
    if mode == "both":
        gt = blobs * 1.7
        gt[rng.random(shape) < 0.02] = -0.25
        gt.flat[0] = -0.25
        teacher = rng.normal(0.3, 0.5, shape)
        teacher.flat[0], teacher.flat[-1] = -0.7, 1.9
    else:
        gt, teacher = blobs, rng.random(shape)
    pred = rng.normal(0, 3, (N, J + (mask_mode == "n1"), h, w))
    pred.flat[::7], pred.flat[3::11], pred.flat[5::13] = 0, 80, -80
    mask = None
    if mask_mode != "none":
        mask = rng.choice(np.array([0, 1, 1, 0.5]), (N, 1 if mask_mode == "n1" else J, h, w)).astype(f32)
    return pred.astype(f32), teacher.astype(f32), gt.astype(f32), mask


def loss_key(shape, mode, mask_mode, kind=None, params=None):
    key = "loss/%s/%s/%s" % ("x".join(str(s) for s in shape), mode, mask_mode)
    return key if kind is None else "%s/%s/%d" % (key, kind, params)


def digest(a):
    """sha-256 of an array's shape, dtype and bytes, as 32 uint8: how the fixture holds a bulky array"""
    import hashlib
    a = np.ascontiguousarray(a)
    head = ("%s %s " % (a.dtype.str, a.shape)).encode()
    return np.frombuffer(hashlib.sha256(head + a.tobytes()).digest(), np.uint8)
