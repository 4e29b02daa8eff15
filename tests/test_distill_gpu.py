"""GPU tests of the distillation targets and losses (csrc/distill.hip): the ground-truth maps, the fused targets, the
normalised tensors and the effective mask bit for bit against the restatement (tests/distill_restated.py, which
tests/test_distill_host.py ties to the reference's results), the loss values within the derived bound.  Every tensor a
native entry writes sits between guard bands that are checked after the call."""
import ctypes
import os

import numpy as np
import pytest
import torch

import distill_restated as R
import test_distill_host as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 64
SENTINEL = -12345.0
measured = {"loss_rel": 0.0, "loss_rel_bound": 0.0, "loss_vs_ref_rel": 0.0}


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    return _native


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(H.ROOT, "tests", "golden", "distill.npz")) as z:
        return {k: z[k] for k in z.files}


class Guarded:
    """a device tensor of `shape` with BAND sentinel elements on either side"""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        fill = 0xA5 if dtype == torch.uint8 else SENTINEL
        self.fill = fill
        self.buf = torch.full((self.n + 2 * BAND,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[BAND:BAND + self.n].view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:BAND] == self.fill).all() and (b[BAND + self.n:] == self.fill).all())

    def numpy(self):
        return self.t.cpu().numpy()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream(nat):
    return nat.stream_ptr(torch.device(DEV))


# ---- 1. ground-truth maps -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,hw", R.GT_SHAPES)
def test_gt_maps_equal_the_reference(nat, golden, J, hw):
    """the scene holds the corner, outside, truncating, unlabelled and overlapping joints, an image without people and
    one with 70: more than one wavefront of people and two LDS chunks of RTPE_DISTILL_CHUNK = 64"""
    from rtpe import dataloaders, distill
    scene = R.gt_scene(J, hw)
    assert len(scene[1]) == 0 and len(scene[2]) == R.CROWD > nat.DISTILL_CHUNK
    table = distill.JointTable(scene, J).to(DEV)
    for sigma in R.GT_SIGMAS:
        want = H.gt_maps(J, hw, sigma)
        out = Guarded(want.shape)
        distill.gt_heatmaps(table, hw, sigma, out=out.t)
        got = out.numpy()
        assert out.intact()
        assert np.array_equal(got, want), (J, hw, sigma, np.argwhere(got != want)[:4])
        assert H.same(got, golden["gt/%d/%dx%d/%g" % (J, hw[0], hw[1], sigma)])
        gen = dataloaders.HWHeatmapGenerator(J, sigma)
        batch = gen.batch(table, hw)
        assert batch.is_cuda and batch.dtype == torch.float32 and np.array_equal(batch.cpu().numpy(), want)
    for n in (0, 1, 3):             # the reference's call, image by image (the last sigma)
        one = gen(scene[n], hw)
        assert isinstance(one, np.ndarray) and one.dtype == np.float32 and np.array_equal(one, want[n])


# ---- 2. targets -----------------------------------------------------------------------------------------------------------
def native_targets(nat, case, table, teacher, mask, segm):
    (Hh, W), (h, w), (ha, wa), (ht, wt) = case
    N, J = len(table), table.num_joints
    from rtpe import distill
    outs = dict(gt=Guarded((N, J, h, w)), teacher=Guarded((N, J, h, w)), mask=Guarded((N, 1, h, w)),
                segm=Guarded((N, 1, ha, wa)), minmax=Guarded((4,)))
    sb = ctypes.c_size_t()
    nat.check(nat.lib().rtpe_distill_targets_scratch_bytes(N, J, h, w, ctypes.byref(sb)))
    scratch = Guarded((sb.value,), torch.uint8)
    patch = distill._patch_on(2.0, torch.device(DEV))
    nat.check(nat.lib().rtpe_distill_targets(
        table.offsets_t.data_ptr(), table.joints_t.data_ptr(), len(table.joints), patch.data_ptr(), patch.shape[0], 2.0,
        teacher.data_ptr(), ht, wt, mask.data_ptr(), segm.data_ptr(), N, J, Hh, W, h, w, ha, wa, outs["gt"].ptr(),
        outs["teacher"].ptr(), outs["mask"].ptr(), outs["segm"].ptr(), outs["minmax"].ptr(), scratch.ptr(), sb.value,
        stream(nat)))
    torch.cuda.synchronize()
    assert all(g.intact() for g in outs.values()) and scratch.intact()
    return {k: g.numpy() for k, g in outs.items()}


@pytest.mark.parametrize("i", range(len(R.TARGET_CASES)))
def test_targets_equal_the_two_step_chain(nat, golden, i):
    """fusing the stamp into the resize and composing the teacher's two resizes changes no bit"""
    from rtpe import distill
    case = R.TARGET_CASES[i]
    image_hw, det_hw, att_hw, _ = case
    people, teacher, mask, segm = R.target_inputs(case)
    want = H.target_maps(i)
    table = distill.JointTable(people, R.TARGET_J).to(DEV)
    t_d, m_d, s_d = dev(teacher), dev(mask), dev(segm)
    got = native_targets(nat, case, table, t_d, m_d, s_d)
    for k in ("gt", "teacher", "mask", "segm"):
        assert np.array_equal(got[k], want[k]), (case, k, np.argwhere(got[k] != want[k])[:4])
        assert H.same(got[k], golden["targets/%d/%s" % (i, k)])
    assert np.array_equal(got["minmax"], want["minmax"]), (got["minmax"], want["minmax"])
    # the Python surface: everything, each input absent, each input alone
    full = dict(table=table, teacher=t_d, mask=m_d, segm=s_d)
    subsets = [set(full)] + [set(full) - {k} for k in full] + [{k} for k in full]
    for present in subsets:
        kw = {k: (v if k in present else None) for k, v in full.items()}
        res = distill.distillation_targets(kw.pop("table"), image_hw, det_hw, att_hw if "segm" in present else None, **kw)
        mm = want["minmax"].copy()
        for k, name in (("table", "gt"), ("teacher", "teacher"), ("mask", "mask"), ("segm", "segm")):
            t = getattr(res, name)
            if k in present:
                assert t.is_cuda and np.array_equal(t.cpu().numpy(), want[name]), (case, present, name)
            else:
                assert t is None
        if "table" not in present:
            mm[:2] = 0
        if "teacher" not in present:
            mm[2:] = 0
        assert np.array_equal(res.minmax.cpu().numpy(), mm), (case, present)
    assert np.array_equal(t_d.cpu().numpy(), teacher) and np.array_equal(m_d.cpu().numpy(), mask)


# ---- 3. normalise and loss ------------------------------------------------------------------------------------------------
def native_loss(nat, kind, unit, pred, teacher, gt, mask, alpha, bf, pw_t, pw_g, minmax=None, keep=False):
    N, J, h, w = gt.shape
    outs = [Guarded(gt.shape) if keep and t is not None else None for t in (gt, teacher, mask)]
    loss, scratch = Guarded((5,), torch.float64), Guarded((nat.DISTILL_SCRATCH_BYTES,), torch.uint8)
    nat.check(nat.lib().rtpe_distill_loss(
        {"bce": nat.DISTILL_BCE, "mse": nat.DISTILL_MSE}[kind], int(unit),
        pred.data_ptr(), pred.shape[1], ptr(teacher), gt.data_ptr(), ptr(mask), mask.shape[1] if mask is not None else 1,
        N, J, h, w, alpha, bf, pw_t, pw_g, ptr(minmax), *[None if g is None else g.ptr() for g in outs], loss.ptr(),
        scratch.ptr(), nat.DISTILL_SCRATCH_BYTES, stream(nat)))
    torch.cuda.synchronize()
    assert loss.intact() and scratch.intact() and all(g is None or g.intact() for g in outs)
    raw = loss.t.cpu()
    return raw.numpy()[:3].copy(), raw.view(torch.float32).numpy()[6:9].copy(), [None if g is None else g.numpy() for g in outs]


def native_normalise(nat, gt, teacher, mask, bf, minmax=None):
    N, J, h, w = gt.shape
    outs = [Guarded(gt.shape) if t is not None else None for t in (gt, teacher, mask)]
    scratch = Guarded((nat.DISTILL_SCRATCH_BYTES,), torch.uint8)
    nat.check(nat.lib().rtpe_distill_normalise(
        gt.data_ptr(), ptr(teacher), ptr(mask), mask.shape[1] if mask is not None else 1, N, J, h, w, bf, ptr(minmax),
        *[None if g is None else g.ptr() for g in outs], scratch.ptr(), nat.DISTILL_SCRATCH_BYTES, stream(nat)))
    torch.cuda.synchronize()
    assert scratch.intact() and all(g is None or g.intact() for g in outs)
    return [None if g is None else g.numpy() for g in outs]


def close32(v, want, n):
    """a float32 scalar of the surface against the restatement: the float64 bound and one float32 rounding"""
    return abs(float(v) - want) <= (R.loss_bound(n) + 2.0 ** -24) * abs(want)


def same_or_none(a, b):
    return (a is None and b is None) or np.array_equal(a, b)


@pytest.mark.parametrize("shape,mode,mask_mode", H.loss_cases())
def test_normalised_tensors_exact_and_losses_within_the_derived_bound(nat, golden, shape, mode, mask_mode):
    pred, teacher, gt, mask = R.loss_inputs(shape, mode, mask_mode)
    assert pred.shape[1] == shape[1] + (mask_mode == "n1")          # a det with J + 1 channels, read in place
    assert (pred == 0).any() or pred.size < 7
    assert pred.size < 13 or ((pred == 80).any() and (pred == -80).any())
    p_d, t_d, g_d, m_d = dev(pred), dev(teacher), dev(gt), dev(mask)
    mm = dev(np.array([gt.min(), gt.max(), teacher.min(), teacher.max()], np.float32))
    n = gt.size
    for bf in (0.0, 0.25, 1.0):
        want = R.normalise(gt, teacher, mask, bf)
        for given in (None, mm):            # the min / max computed by the entry, or handed over from the targets
            got = native_normalise(nat, g_d, t_d, m_d, bf, given)
            assert all(same_or_none(a, b) for a, b in zip(got, want)), (shape, mode, mask_mode, bf)
    got = native_normalise(nat, g_d, None, None, 0.5)
    assert np.array_equal(got[0], R.normalise(gt, None, None, 0.5)[0]) and got[1] is None and got[2] is None
    for kind in R.LOSS_KINDS:
        for pi, (bf, alpha, pw) in enumerate(R.LOSS_PARAMS):
            key = R.loss_key(shape, mode, mask_mode, kind, pi)
            pw_t, pw_g = R.loss_pos_weights(pw)
            unit = kind == "bce"
            want = R.distillation_loss(pred, teacher, gt, alpha, mask, bf, kind, pw_t, pw_g)
            f64, f32, kept = native_loss(nat, kind, unit, p_d, t_d, g_d, m_d, alpha, bf, pw_t, pw_g, keep=True)
            again = native_loss(nat, kind, unit, p_d, t_d, g_d, m_d, alpha, bf, pw_t, pw_g, mm if unit else None)
            assert f64.tobytes() == again[0].tobytes() and f32.tobytes() == again[1].tobytes(), key   # run to run
            assert np.array_equal(f32, f64.astype(np.float32))
            tensors = R.normalise(gt, teacher, mask, bf, unit)
            assert all(same_or_none(a, b) for a, b in zip(kept, tensors)), key
            bound = R.loss_bound(n)
            ref = float(golden[key + "/ref32"][0])
            for name, g, wv in zip(("teacher", "gt", "mixed"), f64, want):
                rel = abs(g - wv) / abs(wv) if wv else abs(g - wv)
                measured["loss_rel"] = max(measured["loss_rel"], rel)
                measured["loss_rel_bound"] = max(measured["loss_rel_bound"], bound)
                print("%s %s: device %.17g restatement %.17g relative distance %.3g (bound %.3g)"
                      % (key, name, g, wv, rel, bound))
                assert abs(g - wv) <= bound * abs(wv), (key, name, g, wv)
            allowance = H.loss_allowance(golden, key, want[2], n)
            measured["loss_vs_ref_rel"] = max(measured["loss_vs_ref_rel"], abs(f64[2] - ref) / max(abs(ref), 1e-300))
            print("%s: device %.17g reference %.9g distance %.3g (allowance %.3g)"
                  % (key, f64[2], ref, abs(f64[2] - ref), allowance))
            assert abs(f64[2] - ref) <= allowance, key
    # nothing that was handed in has been written
    for t, a in ((p_d, pred), (t_d, teacher), (g_d, gt), (m_d, mask)):
        assert t is None or np.array_equal(t.cpu().numpy(), a)
    print("measured so far:", measured)


def test_loss_classes_and_the_two_scalars_of_the_training_step(nat, golden):
    from rtpe import distill, optimization as opt
    shape = R.LOSS_SHAPES[0]
    pred, teacher, gt, mask = R.loss_inputs(shape, "neither", "nj")
    p, t, g, m = dev(pred), dev(teacher), dev(gt), dev(mask)
    n = gt.size
    got = {"mse": opt.MaskedMseLoss()(p, g, m), "mse_nomask": opt.MaskedMseLoss()(p, g),
           "bce7": opt.MaskedBceWithLogits(7)(p, g, m), "bce7_nomask": opt.MaskedBceWithLogits(7, device=DEV)(p, g),
           "distill": opt.DistillationLoss()(p, t, g, 0.25, m)}
    want = H.plain_values(pred, teacher, gt, mask)
    for k, v in got.items():
        assert v.is_cuda and v.dtype == torch.float32 and v.dim() == 0, k
        assert close32(v, want[k], n), (k, float(v), want[k])
        ref = float(golden["plain/%s/ref32" % k][0])
        assert abs(float(v) - ref) <= float(golden["plain/%s/ref_dist" % k][0]) + (R.loss_bound(n) + 2.0 ** -24) * abs(ref)
    # the distillation classes with a det of J + 1 channels and an (N, 1, h, w) mask, on targets that need normalising
    pred, teacher, gt, mask = R.loss_inputs(shape, "both", "n1")
    p, t, g, m = dev(pred), dev(teacher), dev(gt), dev(mask)
    for cls, kind, bf in ((opt.DistillationBceLossKeypointMining(7, 1), "bce", 0.25),
                          (opt.DistillationLossKeypointMining(), "mse", 0.25), (opt.DistillationLoss(), "mse", None)):
        v = cls(p, t, g, 0.5, m) if bf is None else cls(p, t, g, alpha=0.5, mask=m, background_factor=bf)
        wv = R.distillation_loss(pred, teacher, gt, 0.5, mask, 1.0 if bf is None else bf, kind, 7.0, 1.0)[2]
        assert v.is_cuda and v.dim() == 0 and close32(v, wv, n), (kind, bf, float(v), wv)
    assert np.array_equal(m.cpu().numpy(), mask)            # the caller's mask is never written
    # the two scalars from targets computed on the device
    case = R.TARGET_CASES[0]
    image_hw, det_hw, att_hw, _ = case
    people, teacher, mask, segm = R.target_inputs(case)
    tg = distill.distillation_targets(distill.JointTable(people, R.TARGET_J).to(DEV), image_hw, det_hw, att_hw,
                                      dev(teacher), dev(mask), dev(segm))
    w = H.target_maps(0)
    rng = np.random.default_rng(5)
    att = rng.random((4, 1) + att_hw).astype(np.float32)            # the sigmoid output, as the reference feeds it
    det = rng.normal(0, 2, (4, R.TARGET_J + 1) + det_hw).astype(np.float32)
    for kind in R.LOSS_KINDS:
        seg, dl = distill.distillation_losses(dev(att), dev(det), tg, 0.5, 1, 7, 1, kind)
        want_seg = R.distillation_loss(att, None, w["segm"], 0.0, None, 1.0, "bce", 1.0, 7.0, unit=False)[1]
        want_det = R.distillation_loss(det, w["teacher"], w["gt"], 0.5, w["mask"], 1.0, kind, 1.0, 1.0)[2]
        for v, wv in ((seg, want_seg), (dl, want_det)):
            assert v.is_cuda and v.dtype == torch.float32 and v.dim() == 0
            assert close32(v, wv, det.size), (kind, float(v), wv)
