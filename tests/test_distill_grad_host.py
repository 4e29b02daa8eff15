"""Host tests of the backward of the distillation losses: the float64 restatement (tests/distill_grad_restated.py)
against the gradients of the reference's own autograd (tests/golden/distill_grad.npz, tools/gen_golden_distill_grad.py),
every seeded fault against the stored cases, the ABI table of include/rtpe_hip_distill_grad.h, every refusal, and the
autograd wiring of the Python surface with the native calls replaced - none of which needs a GPU."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import distill_grad_restated as GR
import distill_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    return _native


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "distill_grad.npz")) as z:
        return {k: z[k] for k in z.files}


restated, effective_mask = GR.restated, GR.effective_mask


def allowance(golden, case, mag):
    """what the reference's float32 gradient may differ from the restatement by: its own measured rounding, per element"""
    return float(golden[GR.grad_key(*case) + "/ref_units"][0]) * 2.0 ** -24 * mag


# ---- 1. the reference's autograd -------------------------------------------------------------------------------------------
def test_fixture_holds_every_case_and_the_stored_gradients(golden):
    assert len(GR.all_cases()) == 144 and len(GR.stored_cases()) == 24
    for case in GR.all_cases():
        assert golden[GR.grad_key(*case) + "/ref_units"].shape == (1,)
    for case in GR.stored_cases():
        ref = golden[GR.grad_key(*case) + "/ref"]
        assert ref.dtype == np.float32 and ref.shape == GR.case_args(*case)["pred"].shape
    worst = max(float(golden[GR.grad_key(*c) + "/ref_units"][0]) for c in GR.all_cases())
    print("the reference's float32 gradient: at most %.3g units of 2^-24 * mag from the restatement" % worst)
    assert 0 < worst < 2.0 ** 10            # float32 rounding, not another formula (a seeded fault: millions of units)


@pytest.mark.parametrize("case", GR.stored_cases(), ids=lambda c: GR.grad_key(*c))
def test_restatement_equals_the_reference_autograd_within_its_rounding(golden, case):
    ref = golden[GR.grad_key(*case) + "/ref"].astype(np.float64)
    v64, mag = restated(case)
    assert (np.abs(ref - v64) <= allowance(golden, case, mag)).all()
    me = effective_mask(case)
    J = case[0][1]
    if me is not None:
        dead = me == 0
        assert dead.any() and not ref[:, :J][dead].any() and not v64[:, :J][dead].any()
        assert not np.signbit(v64[:, :J][dead]).any()
    if v64.shape[1] > J:                    # the channel without a target
        assert not ref[:, J:].any() and not v64[:, J:].any() and not np.signbit(v64[:, J:]).any()


def test_plain_classes_equal_the_reference_autograd(golden):
    pred, teacher, gt, mask = R.loss_inputs(R.LOSS_SHAPES[0], "neither", "nj")
    for name, (t, m, alpha, kind, pw_g, gl) in plain_args(teacher, mask).items():
        v64, mag = GR.grad(pred, t, gt, alpha, m, 1.0, kind, 1.0, pw_g, unit=False, grad_loss=gl)
        ref = golden["plain/%s/ref" % name].astype(np.float64)
        assert (np.abs(ref - v64) <= float(golden["plain/%s/ref_units" % name][0]) * 2.0 ** -24 * mag).all(), name


def plain_args(teacher, mask):
    """name -> (teacher, mask, alpha, kind, gt_pos_weight, upstream) of the five plain-class calls"""
    return {"mse": (None, mask, 0.0, "mse", 1.0, (0, 1, 0)), "mse_nomask": (None, None, 0.0, "mse", 1.0, (0, 1, 0)),
            "bce7": (None, mask, 0.0, "bce", 7.0, (0, 1, 0)), "bce7_nomask": (None, None, 0.0, "bce", 7.0, (0, 1, 0)),
            "distill": (teacher, mask, 0.25, "mse", 1.0, (0, 0, 1))}


# ---- 2. seeded faults ------------------------------------------------------------------------------------------------------
S = GR.STORED_SHAPE
# per fault the stored case that shows it: a mask with halves for the chain's factor and the sigmoid's argument, a
# background factor of 0.25 for the raw mask, alpha = 0 for the exchange (alpha = 0.5 is its own mirror), a pred with an
# extra channel for n and for that channel, MSE for the factor 2
FAULT_CASE = dict(drop_m=(S, "both", "nj", "bce", 3), raw_mask=(S, "both", "nj", "bce", 3),
                  sigmoid_raw=(S, "both", "nj", "bce", 3), pos_weight=(S, "both", "none", "bce", 3),
                  alpha=(S, "neither", "nj", "bce", 1), n_channels=(S, "both", "n1", "mse", 3),
                  no_upstream=(S, "neither", "none", "bce", 3), extra_nonzero=(S, "both", "n1", "bce", 1),
                  no_factor_2=(S, "neither", "nj", "mse", 3))


def test_every_fault_has_a_case():
    assert set(FAULT_CASE) == set(GR.FAULTS) and all(c in GR.stored_cases() for c in FAULT_CASE.values())


@pytest.mark.parametrize("fault", GR.FAULTS)
def test_stored_cases_see_each_seeded_fault_by_a_thousand_allowances(golden, fault):
    case = FAULT_CASE[fault]
    ref = golden[GR.grad_key(*case) + "/ref"].astype(np.float64)
    v64, mag = restated(case)
    bad, _ = GR.grad(fault=fault, **GR.case_args(*case))
    allow = allowance(golden, case, mag)

    def moved(v):
        d = np.abs(v - ref)
        return (d >= 1000 * allow) & (d > 0)
    n_bad = int(moved(bad).sum())
    print("%s on %s: %d of %d elements move by 1,000 allowances or more" % (fault, GR.grad_key(*case), n_bad, bad.size))
    assert n_bad >= 1
    assert not moved(v64).any()


def test_upstream_gradient_is_linear(golden):
    """grad_loss = (0.3, -1.5, 2.0) is the same combination of the three one-hot runs, within the bound on the sum of
    the runs' magnitudes (the combination's terms are bounded by those, not by the magnitude of their cancelling sum)"""
    for case in ((S, "both", "nj", "bce", 3), (S, "both", "n1", "mse", 3), (S, "neither", "none", "bce", 1)):
        v, _ = restated(case, GR.GRAD_LOSS)
        combo, size = 0.0, 0.0
        for i, c in enumerate(GR.GRAD_LOSS):
            vi, mi = restated(case, tuple(float(k == i) for k in range(3)))
            combo = combo + float(np.float32(c)) * vi
            size = size + abs(c) * mi
        assert (np.abs(v - combo) <= GR.grad_bound(size)).all() and np.abs(v).max() > 0
        assert not np.array_equal(v, restated(case)[0])


def test_bound_is_ten_units_and_the_interval_rule_is_tight():
    assert GR.grad_bound(1.0) == 10 * 2.0 ** -52
    v, mag = np.array([1.0, 1.0, 0.0]), np.array([1.0, 1.0, 0.0])
    up = np.nextafter(np.float32(1), np.float32(2))
    assert GR.within(np.array([1, up, 0], np.float32), v, mag).tolist() == [True, False, True]
    half = np.array([1.0 + 2.0 ** -24])             # a tie between two float32: the bound reaches across it
    assert GR.within(np.array([1, up], np.float32), np.repeat(half, 2), np.ones(2)).all()
    assert not GR.within(np.array([np.nextafter(up, np.float32(2))], np.float32), half, np.ones(1)).any()
    # what a differing element needed: the distance from v64 to the rounding boundary on its side, adjacent or not
    one, up2 = np.float32(1), np.nextafter(up, np.float32(2))
    v = np.array([1.0 + 2.0 ** -26] * 3)
    d = GR.crossed(np.array([one, up, up2], np.float32), np.array([one] * 3, np.float32), v)
    assert d.tolist() == [0.0, 2.0 ** -24 - 2.0 ** -26, 3 * 2.0 ** -24 - 2.0 ** -26]


# ---- 3. the ABI ------------------------------------------------------------------------------------------------------------
def _declared(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_backward_symbol_is_declared_in_its_header_and_resolves(built):
    main = _declared("rtpe_hip.h")
    assert len(re.findall(r'#include "rtpe_hip_distill_grad.h"', main)) == 1
    declared = set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared("rtpe_hip_distill_grad.h")))
    assert declared == {"rtpe_distill_loss_backward"} == set(built.EXPORTS_DISTILL_GRAD)
    older = (built.EXPORTS, built.EXPORTS_SIZES, built.EXPORTS_WARP, built.EXPORTS_SHARED, built.EXPORTS_PAIR,
             built.EXPORTS_RECORDS, built.EXPORTS_TAGMEAN, built.EXPORTS_NOPROJ, built.EXPORTS_ANYSIZE,
             built.EXPORTS_MIXED, built.EXPORTS_MIXDEC, built.EXPORTS_TRACE, built.EXPORTS_MIXAUX, built.EXPORTS_FRAMES,
             built.EXPORTS_OKS, built.EXPORTS_DISTILL)
    assert [len(t) for t in older] == [59, 5, 3, 3, 1, 2, 6, 5, 4, 4, 4, 2, 1, 3, 2, 5]
    for table in older:
        assert not declared & set(table)
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "rtpe_hip_distill_grad.h":
            assert not declared & set(re.findall(r"\b(rtpe_[a-z0-9_]+)\s*\(", _declared(name))), name
    lib = built.lib()
    assert lib.rtpe_distill_loss_backward.argtypes == built._SIGS_DISTILL_GRAD["rtpe_distill_loss_backward"][1]
    assert len(built._SIGS_DISTILL_GRAD["rtpe_distill_loss_backward"][1]) == 16
    assert lib.rtpe_version() == 4 and built.ABI_VERSION == 4


# ---- 4. refusals, each before any GPU work ---------------------------------------------------------------------------------
def test_c_entry_refuses_before_any_launch(built):
    L = built.lib()
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)

    def refused(rc, *words):
        msg = L.rtpe_last_error_string()
        assert rc < 0 and all(w in msg for w in words), (rc, msg)

    ok = dict(kind=0, pred=fake, pc=18, teacher=fake, gt=fake, mask=fake, N=2, J=17, h=10, w=14, alpha=0.5, pw_t=1.0,
              pw_g=7.0, grad_loss=fake, grad_pred=fake, stream=None)
    for kw in ([{k: None} for k in ("pred", "gt", "grad_loss", "grad_pred")] +
               [{k: v} for k in ("N", "J", "h", "w") for v in (0, -1)] +
               [dict(pc=16), dict(kind=2), dict(kind=-1), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float("nan")),
                dict(grad_loss=odd), dict(N=1 << 20, pc=1 << 12, J=1), dict(N=1 << 20, pc=1 << 12, J=1 << 12),
                dict(h=1 << 16, w=1 << 16), dict(N=1 << 15, pc=1 << 15, J=1, h=1 << 15, w=1 << 15)]):
        refused(L.rtpe_distill_loss_backward(*dict(ok, **kw).values()), b"distill_loss_backward")
    refused(L.rtpe_distill_loss_backward(*dict(ok, alpha=1.5).values()), b"alpha = 1.5 outside [0, 1]")
    refused(L.rtpe_distill_loss_backward(*dict(ok, N=1 << 15, pc=1 << 15, J=1, h=1 << 15, w=1 << 15).values()), b"workgroups")
    refused(L.rtpe_distill_loss_backward(*dict(ok, pc=16).values()), b"pred_channels = 16 is below J = 17")


def _t(*shape, **kw):
    return torch.zeros(shape, **kw)


def test_python_surface_refuses_without_a_gpu(built):
    from rtpe import distill, optimization as opt
    pred, teacher, gt, mask = _t(2, 18, 4, 5), _t(2, 17, 4, 5), _t(2, 17, 4, 5), _t(2, 1, 4, 5)
    live = _t(2, 18, 4, 5, requires_grad=True)
    bce = opt.DistillationBceLossKeypointMining(1, 7, differentiable=True)
    mining, plain = opt.DistillationLossKeypointMining(differentiable=True), opt.DistillationLoss(differentiable=True)
    mse, bce1 = opt.MaskedMseLoss(differentiable=True), opt.MaskedBceWithLogits(7, differentiable=True)
    assert all(m.differentiable for m in (bce, mining, plain, mse, bce1))
    assert not any(m.differentiable for m in (opt.DistillationBceLossKeypointMining(1, 7), opt.DistillationLoss(),
                                              opt.DistillationLossKeypointMining(), opt.MaskedMseLoss(),
                                              opt.MaskedBceWithLogits(7, "cpu")))
    # a pred that wants a gradient is taken as far as the device
    live17 = _t(2, 17, 4, 5, requires_grad=True)
    for call in (lambda: bce(live, teacher, gt, mask=mask), lambda: mining(live, teacher, gt), lambda: plain(live, teacher, gt),
                 lambda: mse(live17, gt), lambda: bce1(live17, gt, mask),
                 lambda: distill.loss_values("mse", live, teacher, gt, differentiable=True),
                 lambda: distill.distillation_losses(None, live, distill.DistillTargets(gt, teacher, mask, None, _t(4)),
                                                     differentiable=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # only student_pred gets one: a target or a mask that wants a gradient is refused by name
    for kw, word in ((dict(teacher_pred=_t(2, 17, 4, 5, requires_grad=True)), "teacher_pred requires grad"),
                     (dict(gt=_t(2, 17, 4, 5, requires_grad=True)), "gt requires grad"),
                     (dict(mask=_t(2, 1, 4, 5, requires_grad=True)), "mask requires grad")):
        args = dict(dict(student_pred=live, teacher_pred=teacher, gt=gt, mask=mask), **kw)
        with pytest.raises(NotImplementedError, match=word):
            bce(**args)
    with pytest.raises(NotImplementedError, match="gt requires grad"):
        mse(pred[:, :17].contiguous(), _t(2, 17, 4, 5, requires_grad=True))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):       # grad mode off: nothing to refuse
        bce(live, teacher, _t(2, 17, 4, 5, requires_grad=True))
    # parameters first, then the gradient question, then dtype and shape, then the device
    with pytest.raises(ValueError, match="alpha"):
        bce(live, _t(2, 17, 4, 5, requires_grad=True), gt, alpha=1.5)
    with pytest.raises(ValueError, match="background_factor"):
        mining(live, teacher, gt.double(), background_factor=2)
    with pytest.raises(NotImplementedError, match="pick_top"):
        bce(live, teacher, gt, pick_top=8)
    with pytest.raises(NotImplementedError, match="teacher_pred requires grad"):
        bce(live.double(), _t(2, 17, 4, 5, requires_grad=True), gt)
    for bad, word in ((dict(student_pred=_t(2, 18, 4, 5, dtype=torch.float64, requires_grad=True)), "student_pred must be float32"),
                      (dict(student_pred=_t(2, 16, 4, 5, requires_grad=True)), "student_pred has shape"),
                      (dict(student_pred=_t(2, 4, 5, 18, requires_grad=True).permute(0, 3, 1, 2)), "student_pred must be contiguous"),
                      (dict(gt=gt.half()), "gt must be float32"), (dict(mask=_t(2, 2, 4, 5)), "mask has shape")):
        args = dict(dict(student_pred=live, teacher_pred=teacher, gt=gt, mask=mask), **bad)
        with pytest.raises(ValueError, match=word):
            bce(**args)
    with pytest.raises(ValueError, match="student_pred has shape"):           # the masked classes take equal shapes only
        mse(live, gt)
    # the default is what it was
    for call in (lambda: opt.DistillationBceLossKeypointMining(1, 7)(live, teacher, gt), lambda: opt.MaskedMseLoss()(live17, gt),
                 lambda: opt.MaskedBceWithLogits(7)(live17, gt), lambda: opt.DistillationLoss()(live, teacher, gt),
                 lambda: distill.loss_values("bce", live, teacher, gt),
                 lambda: distill.distillation_losses(None, live, distill.DistillTargets(gt, teacher, mask, None, _t(4)))):
        with pytest.raises(NotImplementedError, match="forward value only"):
            call()
    assert not mask.any() and live.grad is None


# ---- 5. the autograd wiring, with the native calls replaced ----------------------------------------------------------------
class FakeLib:
    """stands in for the library: rtpe_distill_loss_backward writes g0 + 2 g1 + 4 g2 into every element of grad_pred"""

    def __init__(self):
        self.calls = []

    def rtpe_distill_loss_backward(self, kind, pred, pc, teacher, gt, mask, N, J, h, w, alpha, pw_t, pw_g, grad_loss,
                                   grad_pred, stream):
        g = np.ctypeslib.as_array(ctypes.cast(grad_loss, ctypes.POINTER(ctypes.c_float)), (3,))
        out = np.ctypeslib.as_array(ctypes.cast(grad_pred, ctypes.POINTER(ctypes.c_float)), (N * pc * h * w,))
        out[:] = g[0] + 2 * g[1] + 4 * g[2]
        self.calls.append(dict(kind=kind, pc=pc, teacher=teacher, mask=mask, shape=(N, J, h, w), alpha=alpha, pw=(pw_t, pw_g),
                               g=g.copy()))
        return 0


@pytest.fixture()
def wired(monkeypatch):
    from rtpe import _native, distill
    fake = FakeLib()
    kept = []

    def forward(pred, kind, teacher, gt, alpha, mask, background_factor, teacher_pos_weight, gt_pos_weight, unit, minmax,
                keep):
        buf = torch.tensor([1.0, 2.0, 3.0, 0.0, 0.0], dtype=torch.float64)
        buf.view(torch.float32)[6:9] = torch.tensor([1.0, 2.0, 3.0])
        outs = [None, None, None]
        if keep:
            outs = [gt.clone(), None if teacher is None else teacher.clone(), None if mask is None else gt.clone()]
            kept.append(outs)
        return distill.LossValues(buf[:3], buf.view(torch.float32)[6:9], *outs)
    monkeypatch.setattr(distill, "_loss_forward", forward)
    monkeypatch.setattr(distill, "_check_loss_inputs", lambda *a, **k: None)
    monkeypatch.setattr(_native, "lib", lambda: fake)
    monkeypatch.setattr(_native, "on_device", lambda t: contextlib.nullcontext())
    monkeypatch.setattr(_native, "stream_ptr", lambda d: None)
    return fake, kept


def test_autograd_wiring_of_the_differentiable_forward(wired):
    from rtpe import distill, optimization as opt
    fake, kept = wired
    teacher, gt, mask = _t(2, 3, 4, 5), _t(2, 3, 4, 5), _t(2, 1, 4, 5)
    pred = _t(2, 4, 4, 5, requires_grad=True)
    v = distill.loss_values("bce", pred, teacher, gt, 0.25, mask, teacher_pos_weight=7.0, gt_pos_weight=1.0, differentiable=True)
    assert v.f32.grad_fn is not None and v.f32.tolist() == [1.0, 2.0, 3.0]
    assert not v.f64.requires_grad and not v.gt.requires_grad and not v.teacher.requires_grad and not v.mask.requires_grad
    assert len(kept) == 1 and not fake.calls
    v.f32[2].backward(retain_graph=True)
    assert fake.calls[-1]["g"].tolist() == [0.0, 0.0, 1.0] and fake.calls[-1]["shape"] == (2, 3, 4, 5)
    assert fake.calls[-1]["pc"] == 4 and fake.calls[-1]["alpha"] == 0.25 and fake.calls[-1]["pw"] == (7.0, 1.0)
    assert fake.calls[-1]["kind"] == 0 and fake.calls[-1]["teacher"] and fake.calls[-1]["mask"]
    assert pred.grad.shape == pred.shape and (pred.grad == 4).all()
    (0.5 * v.f32[0] - v.f32[1]).backward()              # a sum of several losses; accumulates
    assert fake.calls[-1]["g"].tolist() == [0.5, -1.0, 0.0] and (pred.grad == 4 + 0.5 - 2).all()
    # torch.autograd.grad, and no double backward
    pred2 = _t(2, 3, 4, 5, requires_grad=True)
    loss = opt.MaskedMseLoss(differentiable=True)(pred2, gt)
    scale = torch.ones((), requires_grad=True)          # (a first derivative that depends on something live)
    (g,) = torch.autograd.grad(loss * scale, pred2, create_graph=True)
    assert fake.calls[-1]["g"].tolist() == [0.0, 1.0, 0.0] and fake.calls[-1]["kind"] == 1
    assert fake.calls[-1]["teacher"] is None and fake.calls[-1]["mask"] is None and (g == 2).all()
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    # an in-place write between forward and backward is caught by the version check
    pred3 = _t(2, 3, 4, 5, requires_grad=True)
    x = pred3 * 1.0
    loss = opt.DistillationLoss(differentiable=True)(x, teacher, gt, 0.25)
    with torch.no_grad():
        x.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_without_a_gradient_the_plain_forward_runs(wired):
    from rtpe import distill, optimization as opt
    fake, kept = wired
    teacher, gt = _t(2, 3, 4, 5), _t(2, 3, 4, 5)
    live = _t(2, 3, 4, 5, requires_grad=True)
    with torch.no_grad():
        a = opt.DistillationLoss(differentiable=True)(live, teacher, gt)
    b = opt.DistillationLoss(differentiable=True)(live.detach(), teacher, gt)
    v = distill.loss_values("mse", live.detach(), teacher, gt, differentiable=True)
    assert a.grad_fn is None and b.grad_fn is None and not a.requires_grad and not b.requires_grad
    assert v.gt is None and v.teacher is None and v.mask is None and v.f32.grad_fn is None
    assert not kept and not fake.calls
