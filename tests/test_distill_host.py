"""Host tests of the distillation targets and losses: the numpy restatement (tests/distill_restated.py) against the
reference's results (tests/golden/distill.npz, tools/gen_golden_distill.py), every seeded fault against the test data,
the ABI table of include/rtpe_hip_distill.h, and every refusal - none of which needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import distill_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's float32 loss against the float64 restatement: about six roundings of 2^-24 per element (relative, the
# terms are >= 0) and a float32 sum in vectors and blocks, at most log2(n) levels; n <= 2^16 here
REF_F32_BOUND = (8 + 16) * 2.0 ** -24


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "distill.npz")) as z:
        return {k: z[k] for k in z.files}


def same(a, d):
    return np.array_equal(R.digest(a), d)


# ---- shared with tests/test_distill_gpu.py: each reference result computed once -----------------------------------------
_cache = {}


def gt_maps(J, hw, sigma):
    key = ("gt", J, hw, sigma)
    if key not in _cache:
        _cache[key] = np.stack([R.gt_heatmaps(p, J, hw, sigma) for p in R.gt_scene(J, hw)])
        _cache[key].setflags(write=False)
    return _cache[key]


def target_maps(i):
    key = ("targets", i)
    if key not in _cache:
        image_hw, det_hw, att_hw, _ = R.TARGET_CASES[i]
        people, teacher, mask, segm = R.target_inputs(R.TARGET_CASES[i])
        _cache[key] = R.targets(people, R.TARGET_J, image_hw, det_hw, att_hw, teacher, mask, segm)
    return _cache[key]


def loss_cases():
    return [(s, m, k) for s in R.LOSS_SHAPES for m in R.LOSS_MODES for k in R.LOSS_MASKS]


def loss_allowance(golden, key, want, n):
    """what the device's float64 value may differ from the reference's float32 scalar by: the reference's own distance
    from the restatement (fixture) plus the derived bound; nothing else"""
    return float(golden[key + "/ref_dist"][0]) + R.loss_bound(n) * abs(want)


# ---- 1. fixture parity ----------------------------------------------------------------------------------------------------
def test_patch_table_and_the_half_sigma_peak(golden):
    for sigma in (0.3, 0.5, 0.7, 1, 1.25, 1.5, 2, 2.5, 3, 4):
        g = R.patch_table(sigma)
        assert g.shape == (len(np.arange(0, 6 * sigma + 3)),) * 2
    for J, hw in R.GT_SHAPES:       # sigma = 0.5: the window misses the table's centre, the peak is exp(-1)
        assert golden["gt/%d/%dx%d/0.5/peak" % (J, hw[0], hw[1])][0] == np.float32(np.exp(-1.0))
        assert gt_maps(J, hw, 0.5).max() == np.float32(np.exp(-1.0))
        assert gt_maps(J, hw, 2.0).max() == 1.0


@pytest.mark.parametrize("J,hw", R.GT_SHAPES)
def test_gt_maps_equal_the_reference(golden, J, hw):
    for sigma in R.GT_SIGMAS:
        key = "gt/%d/%dx%d/%g" % (J, hw[0], hw[1], sigma)
        maps = gt_maps(J, hw, sigma)
        assert same(maps, golden[key]), key
        if key + "/raw" in golden:
            assert np.array_equal(maps, golden[key + "/raw"])
        assert not maps[1].any() and maps[2].any()          # nobody; the crowd


@pytest.mark.parametrize("i", range(len(R.TARGET_CASES)))
def test_targets_equal_the_reference(golden, i):
    got = target_maps(i)
    for k in ("gt", "teacher", "mask", "segm"):
        assert same(got[k], golden["targets/%d/%s" % (i, k)]), (R.TARGET_CASES[i], k)
    assert np.array_equal(got["minmax"], golden["targets/%d/minmax" % i])


def test_target_cases_cover_both_resize_kernels_and_the_copy():
    small = {(sum(c[0]) <= R.SMALL_OUTPUT, sum(c[1]) <= R.SMALL_OUTPUT) for c in R.TARGET_CASES}
    assert small == {(True, True), (False, False)}
    assert any(c[0] == c[1] for c in R.TARGET_CASES) and any(c[0] == c[3] for c in R.TARGET_CASES)
    assert any(sum(c[2]) > R.SMALL_OUTPUT for c in R.TARGET_CASES)


@pytest.mark.parametrize("shape,mode,mask_mode", loss_cases())
def test_normalised_targets_masks_and_losses_equal_the_reference(golden, shape, mode, mask_mode):
    pred, teacher, gt, mask = R.loss_inputs(shape, mode, mask_mode)
    mask_before = None if mask is None else mask.copy()
    gn, tn, _ = R.normalise(gt, teacher, mask, 1.0)
    assert same(gn, golden[R.loss_key(shape, mode, mask_mode) + "/gt"])
    assert same(tn, golden[R.loss_key(shape, mode, mask_mode) + "/teacher"])
    if mode == "both" and gt.size > 1:
        assert gt.min() < 0 and gt.max() > 1 and teacher.min() < 0 and teacher.max() - teacher.min() > 1
        assert gn.min() == 0 and gn.max() == 1 and tn.min() == 0 and tn.max() == 1
    if mode == "neither":
        assert np.array_equal(gn, gt) and np.array_equal(tn, teacher)
    for kind in R.LOSS_KINDS:
        for pi, (bf, alpha, pw) in enumerate(R.LOSS_PARAMS):
            key = R.loss_key(shape, mode, mask_mode, kind, pi)
            pw_t, pw_g = R.loss_pos_weights(pw)
            want = R.distillation_loss(pred, teacher, gt, alpha, mask, bf, kind, pw_t, pw_g)[2]
            ref = float(golden[key + "/ref32"][0])
            print("%s: restatement %.17g reference %.9g distance %.3g (relative %.3g)"
                  % (key, want, ref, abs(ref - want), abs(ref - want) / max(abs(want), 1e-300)))
            assert abs(ref - want) == golden[key + "/ref_dist"][0]          # the restatement the fixture was made with
            assert abs(ref - want) <= REF_F32_BOUND * abs(want) + 1e-45, key
            if kind == "bce" and mask is not None:
                assert same(R.normalise(gt, teacher, mask, bf)[2], golden[key + "/mask"]), key
    if mask is not None:
        assert np.array_equal(mask, mask_before)


def test_plain_classes_equal_the_reference(golden):
    pred, teacher, gt, mask = R.loss_inputs(R.LOSS_SHAPES[0], "neither", "nj")
    want = plain_values(pred, teacher, gt, mask)
    for k, v in want.items():
        ref = float(golden["plain/%s/ref32" % k][0])
        assert abs(ref - v) == golden["plain/%s/ref_dist" % k][0], k
        assert abs(ref - v) <= REF_F32_BOUND * abs(v), k


def plain_values(pred, teacher, gt, mask):
    return {"mse": R.distillation_loss(pred, None, gt, 0.0, mask, 1.0, "mse")[1],
            "mse_nomask": R.distillation_loss(pred, None, gt, 0.0, None, 1.0, "mse")[1],
            "bce7": R.distillation_loss(pred, None, gt, 0.0, mask, 1.0, "bce", 1.0, 7.0, unit=False)[1],
            "bce7_nomask": R.distillation_loss(pred, None, gt, 0.0, None, 1.0, "bce", 1.0, 7.0, unit=False)[1],
            "distill": R.distillation_loss(pred, teacher, gt, 0.25, mask, 1.0, "mse")[2]}


def test_bce_of_masked_out_elements_counts_and_extreme_logits_do_not_cancel():
    z = np.zeros((1, 1, 2, 2), np.float32)
    assert R.distillation_loss(z, z, z, 0.5, z, 1.0, "bce")[2] == pytest.approx(np.log(2.0), rel=1e-15)
    x = np.full((1, 1, 1, 1), -80.0, np.float32)
    assert R.distillation_loss(x, None, z[:, :, :1, :1], 0.0, None, 1.0, "bce", unit=False)[1] == \
        pytest.approx(np.exp(-80.0), rel=1e-14)             # (1 - 0) softplus(-80), not 80 - 80
    assert R.distillation_loss(-x, None, z[:, :, :1, :1] + 1, 0.0, None, 1.0, "bce", 1.0, 7.0, unit=False)[1] == \
        pytest.approx(7 * np.exp(-80.0), rel=1e-14)


# ---- 2. seeded faults -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", ["floor", "half_up", "sum", "unclipped"])
def test_gt_data_sees_each_seeded_fault(golden, fault):
    seen = []
    for J, hw in R.GT_SHAPES:
        for sigma in R.GT_SIGMAS:
            bad = np.stack([R.gt_heatmaps(p, J, hw, sigma, fault=fault) for p in R.gt_scene(J, hw)])
            if not same(bad, golden["gt/%d/%dx%d/%g" % (J, hw[0], hw[1], sigma)]):
                seen.append((J, hw, sigma))
    assert seen, fault
    if fault == "half_up":          # 3 sigma + 1 ends in .5 for these two only
        assert {s for _, _, s in seen} == {0.5, 1.5}
    else:
        assert len(seen) == len(R.GT_SHAPES) * len(R.GT_SIGMAS)


@pytest.mark.parametrize("fault,moved", [("align_stage1", ("teacher",)), ("align_stage2", ("gt", "teacher"))])
def test_target_data_sees_swapped_align_corners(golden, fault, moved):
    for i, case in enumerate(R.TARGET_CASES):
        image_hw, det_hw, att_hw, src = case
        people, teacher, mask, segm = R.target_inputs(case)
        bad = R.targets(people, R.TARGET_J, image_hw, det_hw, att_hw, teacher, mask, segm, fault=fault)
        stage_is_a_copy = (src == image_hw) if fault == "align_stage1" else (det_hw == image_hw)
        for k in moved:
            assert same(bad[k], golden["targets/%d/%s" % (i, k)]) == stage_is_a_copy, (case, k)


FAULT_CASE = ((2, 17, 10, 14), "both", "nj", "bce")
# the parameter set on which each fault shows: 1 = background_factor 0.25, alpha 0; 2 = alpha 1, the teacher's pos_weight 7
FAULT_PARAMS = dict(per_image=1, background_first=1, drop_masked=1, pos_weight=2, alpha=1)


@pytest.mark.parametrize("fault", ["per_image", "background_first", "drop_masked", "pos_weight", "alpha"])
def test_loss_data_sees_each_seeded_fault_by_a_hundred_allowances(golden, fault):
    (shape, mode, mask_mode, kind), pi = FAULT_CASE, FAULT_PARAMS[fault]
    pred, teacher, gt, mask = R.loss_inputs(shape, mode, mask_mode)
    bf, alpha, pw = R.LOSS_PARAMS[pi]
    pw_t, pw_g = R.loss_pos_weights(pw)
    want = R.distillation_loss(pred, teacher, gt, alpha, mask, bf, kind, pw_t, pw_g)[2]
    bad = R.distillation_loss(pred, teacher, gt, alpha, mask, bf, kind, pw_t, pw_g, fault=fault)[2]
    allowance = loss_allowance(golden, R.loss_key(shape, mode, mask_mode, kind, pi), want, gt.size)
    print("%s: %.17g -> %.17g, moved by %.3g = %.3g allowances of %.3g" % (fault, want, bad, abs(bad - want),
                                                                           abs(bad - want) / allowance, allowance))
    assert abs(bad - want) >= 100 * allowance
    if fault in ("per_image", "background_first"):          # these two also move the tensors
        gn, tn, me = R.normalise(gt, teacher, mask, bf)
        gb, tb, mb = R.normalise(gt, teacher, mask, bf, fault=fault)
        assert np.array_equal(me, mb) == (fault == "per_image")            # the same elements are background
        assert np.array_equal(gn, gb) == (fault == "background_first") == np.array_equal(tn, tb)


def test_reduction_depth_and_bound():
    assert R.reduction_depth(1) == 1 + 6 + 4 + 1
    assert R.reduction_depth(58905) == 1 + 6 + 4 + 231          # several workgroups and a ragged tail
    assert R.reduction_depth(256 * 256 * 3 + 1) == 4 + 6 + 4 + 256
    assert R.loss_bound(58905) < 4e-14


# ---- 3. the ABI -----------------------------------------------------------------------------------------------------------
def _declared(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_distill_symbols_are_declared_and_resolve(built):
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_distill.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_distill.h")))
    assert declared == {"rtpe_gt_heatmaps", "rtpe_distill_targets_scratch_bytes", "rtpe_distill_targets",
                        "rtpe_distill_normalise", "rtpe_distill_loss"} == set(built.EXPORTS_DISTILL)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR,
             built.EXPORTS_RECORDS, built.EXPORTS_TAGMEAN, built.EXPORTS_NOPROJ, built.EXPORTS_ANYSIZE,
             built.EXPORTS_MIXED, built.EXPORTS_MIXDEC, built.EXPORTS_TRACE, built.EXPORTS_MIXAUX, built.EXPORTS_FRAMES,
             built.EXPORTS_OKS)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6, 5, 4, 4, 4, 2, 1, 3, 2]
    for table in older:
        assert not declared & set(table)
    assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", main))
    lib = built.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == built._SIGS_DISTILL[name][1], name
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "rtpe_hip_distill.h")).read()
    for macro, value in (("RTPE_DISTILL_CHUNK", built.DISTILL_CHUNK), ("RTPE_DISTILL_MAX_PATCH", built.DISTILL_MAX_PATCH),
                         ("RTPE_DISTILL_MAX_BLOCKS", built.DISTILL_MAX_BLOCKS),
                         ("RTPE_DISTILL_SCRATCH_BYTES", built.DISTILL_SCRATCH_BYTES),
                         ("RTPE_DISTILL_LOSS_BYTES", built.DISTILL_LOSS_BYTES), ("RTPE_DISTILL_BCE", built.DISTILL_BCE),
                         ("RTPE_DISTILL_MSE", built.DISTILL_MSE)):
        assert re.search(r"#define %s (\d+)" % macro, hdr).group(1) == str(value)
    assert built.DISTILL_CHUNK < R.CROWD <= 2 * built.DISTILL_CHUNK      # the crowd image: two LDS chunks
    assert R.reduction_depth(10 ** 9) == -(-10 ** 9 // (256 * built.DISTILL_MAX_BLOCKS)) + 6 + 4 + built.DISTILL_MAX_BLOCKS


# ---- 4. refusals, each before any GPU work --------------------------------------------------------------------------------
def test_c_entries_refuse_before_any_launch(built):
    L = built.lib()
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)

    def refused(rc, *words):
        msg = L.rtpe_last_error_string()
        assert rc < 0 and all(w in msg for w in words), (rc, msg)

    gt = dict(off=fake, joints=fake, P=5, N=2, J=17, H=37, W=53, patch=fake, S=15, sigma=2.0, out=fake, stream=None)
    for kw in ([{k: None} for k in ("off", "joints", "patch", "out")] +
               [{k: v} for k in ("N", "J", "H", "W") for v in (0, -1)] +
               [dict(P=-1), dict(S=14), dict(S=16), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
                dict(sigma=200.0, S=1203), dict(joints=odd), dict(H=1 << 16, W=1 << 16), dict(N=1 << 20, J=1 << 12)]):
        refused(L.rtpe_gt_heatmaps(*dict(gt, **kw).values()), b"gt_heatmaps")
    sb = ctypes.c_size_t()
    assert L.rtpe_distill_targets_scratch_bytes(4, 17, 10, 14, ctypes.byref(sb)) == 0 and sb.value == 4 * 17 * 16
    assert L.rtpe_distill_targets_scratch_bytes(32, 17, 80, 80, ctypes.byref(sb)) == 0 and sb.value == 32 * 17 * 25 * 16
    for bad in ((0, 17, 10, 14), (4, 0, 10, 14), (4, 17, 0, 14), (4, 17, 10, -1), (1 << 20, 1 << 12, 10, 14)):
        refused(L.rtpe_distill_targets_scratch_bytes(*bad, ctypes.byref(sb)), b"distill_targets_scratch_bytes")
    refused(L.rtpe_distill_targets_scratch_bytes(4, 17, 10, 14, None), b"null bytes")

    tg = dict(off=fake, joints=fake, P=5, patch=fake, S=15, sigma=2.0, teacher=fake, ht=19, wt=27, mask=fake, segm=fake,
              N=4, J=17, H=37, W=53, h=10, w=14, ha=19, wa=27, gt_out=fake, t_out=fake, m_out=fake, s_out=fake,
              minmax=fake, scratch=fake, sb=4 * 17 * 16, stream=None)
    for kw in ([{k: None} for k in ("off", "joints", "patch", "gt_out", "teacher", "t_out", "mask", "m_out", "segm", "s_out",
                                    "minmax", "scratch")] +
               [{k: v} for k in ("N", "J", "H", "W", "h", "w", "ht", "wt", "ha", "wa") for v in (0, -1)] +
               [dict(S=14), dict(sigma=0.0), dict(P=-1), dict(sb=4 * 17 * 16 - 1), dict(sb=0), dict(scratch=odd),
                dict(joints=odd)]):
        refused(L.rtpe_distill_targets(*dict(tg, **kw).values()), b"distill_targets")
    refused(L.rtpe_distill_targets(*dict(tg, teacher=None).values()), b"both or neither")
    refused(L.rtpe_distill_targets(*dict(tg, off=None).values()), b"all or none")

    nm = dict(gt=fake, teacher=fake, mask=fake, mc=1, N=2, J=17, h=10, w=14, bf=0.5, minmax=None, gt_out=fake, t_out=fake,
              m_out=fake, scratch=fake, sb=built.DISTILL_SCRATCH_BYTES, stream=None)
    for kw in ([{k: None} for k in ("gt", "gt_out", "scratch")] + [{k: v} for k in ("N", "J", "h", "w") for v in (0, -1)] +
               [dict(mc=2), dict(mc=0), dict(bf=-0.1), dict(bf=1.5), dict(bf=float("nan")),
                dict(sb=built.DISTILL_SCRATCH_BYTES - 1), dict(scratch=odd), dict(teacher=None), dict(mask=None)]):
        refused(L.rtpe_distill_normalise(*dict(nm, **kw).values()), b"distill_normalise")
    refused(L.rtpe_distill_normalise(*dict(nm, teacher=None).values()), b"an output without its input")

    ls = dict(kind=0, unit=1, pred=fake, pc=18, teacher=fake, gt=fake, mask=fake, mc=17, N=2, J=17, h=10, w=14, alpha=0.5,
              bf=0.5, pw_t=1.0, pw_g=7.0, minmax=fake, gt_out=None, t_out=None, m_out=None, loss=fake, scratch=fake,
              sb=built.DISTILL_SCRATCH_BYTES, stream=None)
    for kw in ([{k: None} for k in ("pred", "gt", "loss", "scratch")] +
               [{k: v} for k in ("N", "J", "h", "w") for v in (0, -1)] +
               [dict(kind=2), dict(kind=-1), dict(pc=16), dict(mc=3), dict(alpha=-0.01), dict(alpha=1.01),
                dict(alpha=float("nan")), dict(bf=2.0), dict(loss=odd), dict(sb=100), dict(teacher=None, t_out=fake),
                dict(mask=None, m_out=fake)]):
        refused(L.rtpe_distill_loss(*dict(ls, **kw).values()), b"distill_loss")
    refused(L.rtpe_distill_loss(*dict(ls, alpha=1.5).values()), b"alpha = 1.5 outside [0, 1]")


def _t(*shape, **kw):
    return torch.zeros(shape, **kw)


def test_python_surface_refuses_without_a_gpu(built):
    from rtpe import dataloaders, distill, optimization as opt
    pred, teacher, gt, mask = _t(2, 18, 4, 5), _t(2, 17, 4, 5), _t(2, 17, 4, 5), _t(2, 1, 4, 5)
    bce, mining, plain = opt.DistillationBceLossKeypointMining(1, 7), opt.DistillationLossKeypointMining(), \
        opt.DistillationLoss()
    # parameters first
    for fn in (bce, mining):
        with pytest.raises(ValueError, match="alpha"):
            fn(pred, teacher, gt, alpha=1.5, mask=mask)
        with pytest.raises(ValueError, match="background_factor"):
            fn(pred, teacher, gt, mask=mask, background_factor=-0.5)
        with pytest.raises(NotImplementedError, match="pick_top"):
            fn(pred, teacher, gt, mask=mask, pick_top=8)
    with pytest.raises(ValueError, match="alpha"):
        plain(pred, teacher, gt, alpha=-1)
    # an input that wants a gradient
    live = _t(2, 18, 4, 5, requires_grad=True)
    for call in (lambda: bce(live, teacher, gt), lambda: opt.MaskedMseLoss()(live[:, :17], gt),
                 lambda: opt.MaskedBceWithLogits(7)(_t(2, 17, 4, 5, requires_grad=True), gt)):
        with pytest.raises(NotImplementedError, match="forward value only"):
            call()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):        # grad mode off: on to the device
        bce(live, teacher, gt)
    # dtype, shape, contiguity: judged before the device
    for bad, word in ((dict(student_pred=pred.double()), "student_pred must be float32"),
                      (dict(gt=gt.half()), "gt must be float32"),
                      (dict(student_pred=_t(2, 16, 4, 5)), "student_pred has shape"),
                      (dict(student_pred=_t(2, 18, 4, 6)), "student_pred has shape"),
                      (dict(teacher_pred=_t(2, 18, 4, 5)), "teacher_pred has shape"),
                      (dict(mask=_t(2, 2, 4, 5)), "mask has shape"), (dict(mask=_t(1, 1, 4, 5)), "mask has shape"),
                      (dict(gt=_t(2, 17, 20)), "gt must have 4"), (dict(gt=_t(2, 0, 4, 5)), "gt must have 4"),
                      (dict(student_pred=_t(2, 4, 5, 18).permute(0, 3, 1, 2)), "student_pred must be contiguous"),
                      (dict(teacher_pred=_t(2, 17, 4, 10)[..., ::2]), "contiguous"),
                      (dict(gt=np.zeros((2, 17, 4, 5), np.float32)), "gt must be a tensor")):
        args = dict(dict(student_pred=pred, teacher_pred=teacher, gt=gt, mask=mask), **bad)
        with pytest.raises((ValueError, TypeError), match=word):
            bce(**args)
    with pytest.raises(ValueError, match="student_pred has shape"):           # the masked classes take equal shapes only
        opt.MaskedMseLoss()(pred, gt)
    with pytest.raises(ValueError, match="kind"):
        distill.loss_values("l1", pred, teacher, gt)
    # and then the device
    for call in (lambda: bce(pred, teacher, gt, mask=mask), lambda: mining(pred, teacher, gt), lambda: plain(pred, teacher, gt),
                 lambda: opt.MaskedMseLoss()(teacher, gt, mask), lambda: opt.MaskedBceWithLogits()(teacher, gt),
                 lambda: distill.normalise(gt, teacher, mask, 0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert not mask.any() and mask.shape == (2, 1, 4, 5)
    # the people table
    people = [np.zeros((2, 17, 3)), []]
    table = distill.JointTable(people)
    assert len(table) == 2 and table.offsets.tolist() == [0, 2, 2] and table.joints.shape == (2, 17, 3)
    assert table.offsets.dtype == np.int32 and table.joints.dtype == np.float64
    for bad, word in (([np.zeros((2, 16, 3))], "shape"), ([np.full((1, 17, 3), np.nan)], "not finite"),
                      ([np.full((1, 17, 3), np.inf)], "not finite"), ([], "no images")):
        with pytest.raises(ValueError, match=word):
            distill.JointTable(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        table.to("cpu")
    with pytest.raises(RuntimeError, match="on the host"):
        distill.gt_heatmaps(table, (8, 8))
    with pytest.raises(RuntimeError, match="on the host"):
        distill.distillation_targets(table, (8, 8), (2, 2))
    with pytest.raises(TypeError, match="JointTable"):
        distill.distillation_targets(people, (8, 8), (2, 2))
    with pytest.raises(ValueError, match="nothing to compute"):
        distill.distillation_targets(None, (8, 8), (2, 2))
    for kw, word in ((dict(image_hw=(0, 8)), "image_hw"), (dict(det_hw=(2,)), "det_hw"), (dict(att_hw=(2, -1)), "att_hw"),
                     (dict(segm=_t(2, 8, 8)), "segm needs att_hw"), (dict(stddev_pixels=0), "stddev_pixels"),
                     (dict(stddev_pixels=400), "stddev_pixels"), (dict(teacher=_t(2, 17, 4)), "teacher must have 4"),
                     (dict(mask=_t(3, 8, 8)), "mask has shape"), (dict(mask=_t(2, 8, 9)), "mask has shape"),
                     (dict(mask=_t(2, 1, 8, 8)), "mask must have 3"), (dict(segm=_t(2, 8, 8).double(), att_hw=(4, 4)), "float32"),
                     (dict(teacher=_t(2, 17, 4, 4, requires_grad=True)), "forward value only")):
        args = dict(dict(table=None, image_hw=(8, 8), det_hw=(2, 2), teacher=_t(2, 17, 4, 4)), **kw)
        with pytest.raises((ValueError, NotImplementedError), match=word):
            distill.distillation_targets(**args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distill.distillation_targets(None, (8, 8), (2, 2), teacher=_t(2, 17, 4, 4))
    with pytest.raises(TypeError, match="targets must be"):
        distill.distillation_losses(pred, pred, (gt, teacher))
    gen = dataloaders.HWHeatmapGenerator(17, 0.5)
    assert gen.g.shape == (6, 6) and np.array_equal(gen.g, R.patch_table(0.5)) and gen.sigma == 0.5
    with pytest.raises(AssertionError):
        dataloaders.HWHeatmapGenerator(17, 0)
    with pytest.raises(ValueError, match="generator of 3"):
        dataloaders.HWHeatmapGenerator(3).batch(table, (8, 8))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gen(np.zeros((1, 17, 3)), (8, 8))


def test_from_coco_applies_the_dataset_filter():
    from rtpe import distill, scoring
    kp = [float(v) for v in range(51)]
    anns = [dict(image_id=7, category_id=1, keypoints=kp, num_keypoints=5, iscrowd=0, bbox=[0, 0, 9, 9], area=81.0, id=1),
            dict(image_id=7, category_id=1, keypoints=kp, num_keypoints=0, iscrowd=0, bbox=[0, 0, 9, 9], area=81.0, id=2),
            dict(image_id=7, category_id=1, keypoints=kp, num_keypoints=3, iscrowd=1, bbox=[0, 0, 9, 9], area=81.0, id=3),
            dict(image_id=7, category_id=1, keypoints=kp, num_keypoints=0, iscrowd=1, bbox=[0, 0, 9, 9], area=81.0, id=4),
            dict(image_id=9, category_id=1, keypoints=kp, num_keypoints=2, iscrowd=0, bbox=[0, 0, 9, 9], area=81.0, id=5)]
    gt = scoring.CocoKeypointGT(dict(images=[dict(id=7), dict(id=8), dict(id=9)], annotations=anns))
    table = distill.JointTable.from_coco(gt, [9, 8, 7])
    assert table.offsets.tolist() == [0, 1, 1, 4]               # iscrowd == 0 or num_keypoints > 0: all but the last of 7
    assert np.array_equal(table.people(2)[0], np.array(kp).reshape(17, 3))
