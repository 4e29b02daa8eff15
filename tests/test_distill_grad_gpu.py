"""GPU tests of the backward of the distillation losses (csrc/distill_grad.hip): the C entry on every case of the loss
test data, bit for bit against the float64 restatement for MSE and within the derived bound for BCE
(tests/distill_grad_restated.py, which tests/test_distill_grad_host.py ties to the reference's autograd), then the
classes and the order of the training step through PyTorch's autograd.  grad_pred sits between guard bands and is
filled with a sentinel before each call, so an element the kernel does not write shows."""
import numpy as np
import pytest
import torch

import distill_grad_restated as GR
import distill_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 64
SENTINEL = -12345.0
KIND = {"bce": 0, "mse": 1}
# BCE against the rounded restatement: elements compared, elements that differ from float32(v64), and the largest share
# of the bound that such an element needs (the distance from v64 to the rounding boundary it crossed, over the bound)
measured = {"bce_elements": 0, "bce_differ": 0, "bce_bound_used": 0.0}


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as g
    g.build()
    from rtpe import _native
    assert torch.cuda.is_available()
    return _native


class Guarded:
    """a device tensor of `shape` filled with a sentinel, BAND sentinel elements on either side; `skew` moves it that
    many elements off the allocation's alignment"""

    def __init__(self, shape, skew=0, values=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * BAND + skew,), SENTINEL, dtype=torch.float32, device=DEV)
        self.lo = BAND + skew
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        if values is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(values)))
        assert self.t.data_ptr() % 16 == 4 * (skew % 4)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == SENTINEL).all() and (b[self.lo + self.n:] == SENTINEL).all())

    def numpy(self):
        return self.t.cpu().numpy()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def kept_tensors(a):
    """what the forward keeps: the normalised targets and the effective mask (bit for bit what rtpe_distill_loss writes:
    tests/test_distill_gpu.py)"""
    return R.normalise(a["gt"], a["teacher"], a["mask"], a["background_factor"], a["unit"])


def native_backward(nat, a, grad_loss=(0, 0, 1), skew=0, teacher=True):
    """one call of the C entry on the case arguments `a`: grad_pred as numpy"""
    gn, tn, me = kept_tensors(a)
    N, J, h, w = gn.shape
    hold = [Guarded(t.shape, skew, t) if t is not None else None for t in (a["pred"], tn if teacher else None, gn, me)]
    p_d, t_d, g_d, m_d = [None if g is None else g.t for g in hold]
    gl = dev(np.asarray(grad_loss, np.float32))
    out = Guarded(a["pred"].shape, skew)
    nat.check(nat.lib().rtpe_distill_loss_backward(
        KIND[a["kind"]], p_d.data_ptr(), p_d.shape[1], ptr(t_d), g_d.data_ptr(), ptr(m_d), N, J, h, w, float(a["alpha"]),
        float(a["pw_t"]), float(a["pw_g"]), gl.data_ptr(), out.ptr(), nat.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert out.intact() and all(g is None or g.intact() for g in hold)
    for g, src in zip(hold, (a["pred"], tn, gn, me)):           # no input is written
        assert g is None or np.array_equal(g.numpy(), src)
    return out.numpy()


def check_gradient(got, v64, mag, kind, J, me, what):
    """the rule of this file: every element written; MSE equal to float32(v64); BCE within the roundings of the values
    within the derived bound of v64; +0.0 bit for bit behind a zero of the effective mask and in channels >= J"""
    assert got.dtype == np.float32 and got.shape == v64.shape
    assert not (got == SENTINEL).any(), (what, "an element was not written")
    want = v64.astype(np.float32)
    if kind == "mse":
        assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])
    else:
        ok = GR.within(got, v64, mag)
        differ = got != want
        measured["bce_elements"] += got.size
        measured["bce_differ"] += int(differ.sum())
        if differ.any():
            used = GR.crossed(got, want, v64)[differ] / GR.grad_bound(mag)[differ]
            measured["bce_bound_used"] = max(measured["bce_bound_used"], float(used.max()))
        assert ok.all(), (what, np.argwhere(~ok)[:4], got[~ok][:4], v64[~ok][:4], GR.grad_bound(mag)[~ok][:4])
    bits = got.view(np.int32)
    assert not bits[:, J:].any(), what
    if me is not None:
        assert not bits[:, :J][me == 0].any(), what


# ---- 1. the C entry --------------------------------------------------------------------------------------------------------
def test_shapes_take_both_paths_and_a_ragged_last_workgroup():
    hw = [s[2] * s[3] for s in R.LOSS_SHAPES]
    assert [v % 4 == 0 for v in hw] == [True, False, False]
    n, j, h, w = R.LOSS_SHAPES[0]
    assert -(-n * j * h * w // 4 // 256) == 5 and (n * j * h * w // 4) % 256 and -(-n * (j + 1) * h * w // 4 // 256) == 5
    n, j, h, w = R.LOSS_SHAPES[2]
    assert -(-n * j * h * w // 256) > 200 and (n * j * h * w) % 256


@pytest.mark.parametrize("shape,mode,mask_mode", GR.loss_cases())
def test_gradient_exact_for_mse_and_within_the_derived_bound_for_bce(nat, shape, mode, mask_mode):
    for kind in R.LOSS_KINDS:
        for pi in range(len(R.LOSS_PARAMS)):
            case = (shape, mode, mask_mode, kind, pi)
            a = GR.case_args(*case)
            assert a["pred"].shape[1] == shape[1] + (mask_mode == "n1")
            v64, mag = GR.restated(case)
            got = native_backward(nat, a)
            check_gradient(got, v64, mag, kind, shape[1], kept_tensors(a)[2], GR.grad_key(*case))
            if pi == 3:             # run to run
                assert got.tobytes() == native_backward(nat, a).tobytes(), case
    print("measured so far:", measured)


@pytest.mark.parametrize("kind", R.LOSS_KINDS)
@pytest.mark.parametrize("mask_mode", R.LOSS_MASKS)
def test_unaligned_pointers_give_the_bits_of_the_aligned_run(nat, kind, mask_mode):
    """every tensor one element off a 16-byte boundary: the one-pixel form of the kernel on a plane the four-pixel form
    takes when aligned"""
    case = (R.LOSS_SHAPES[0], "both", mask_mode, kind, 3)
    a = GR.case_args(*case)
    aligned, skewed = native_backward(nat, a), native_backward(nat, a, skew=1)
    assert aligned.tobytes() == skewed.tobytes()
    check_gradient(skewed, *GR.restated(case), kind, case[0][1], kept_tensors(a)[2], case)


@pytest.mark.parametrize("shape", R.LOSS_SHAPES)
def test_upstream_gradient_of_all_three_losses(nat, shape):
    for mode, mask_mode, kind, pi in (("both", "nj", "bce", 3), ("both", "n1", "mse", 3), ("neither", "none", "bce", 1),
                                      ("neither", "n1", "bce", 2), ("neither", "nj", "mse", 0)):
        case = (shape, mode, mask_mode, kind, pi)
        a = GR.case_args(*case)
        v64, mag = GR.restated(case, GR.GRAD_LOSS)
        got = native_backward(nat, a, GR.GRAD_LOSS)
        check_gradient(got, v64, mag, kind, shape[1], kept_tensors(a)[2], (case, GR.GRAD_LOSS))
        zero = native_backward(nat, a, (0, 0, 0))
        assert not zero.any()


@pytest.mark.parametrize("shape", R.LOSS_SHAPES)
def test_without_a_teacher_its_term_is_absent(nat, shape):
    for mask_mode, kind, pi in (("nj", "bce", 3), ("n1", "mse", 3), ("none", "bce", 2), ("none", "mse", 1)):
        a = GR.case_args(shape, "both", mask_mode, kind, pi)
        for gl in ((0, 0, 1), GR.GRAD_LOSS):
            v64, mag = GR.grad(grad_loss=gl, **dict(a, teacher=None))
            got = native_backward(nat, a, gl, teacher=False)
            me = R.normalise(a["gt"], None, a["mask"], a["background_factor"], a["unit"])[2]
            check_gradient(got, v64, mag, kind, shape[1], me, (shape, mask_mode, kind, pi, gl))
        if a["alpha"] > 0:
            assert not np.array_equal(got, native_backward(nat, a, gl))


# ---- 2. the classes --------------------------------------------------------------------------------------------------------
def test_each_class_gives_the_forward_bits_and_the_restated_gradient(nat):
    from rtpe import optimization as opt
    shape = R.LOSS_SHAPES[0]
    J = shape[1]
    pred, teacher, gt, mask = R.loss_inputs(shape, "neither", "nj")
    pred2, teacher2, gt2, mask2 = R.loss_inputs(shape, "both", "n1")
    # (class, constructor arguments, forward arguments after student_pred, the arguments of the restatement)
    calls = [(opt.MaskedMseLoss, (), (gt, mask), dict(pred=pred, teacher=None, gt=gt, alpha=0.0, mask=mask,
                                                      background_factor=1.0, kind="mse", pw_t=1.0, pw_g=1.0, unit=False,
                                                      grad_loss=(0, 1, 0))),
             (opt.MaskedBceWithLogits, (7,), (gt, mask), dict(pred=pred, teacher=None, gt=gt, alpha=0.0, mask=mask,
                                                              background_factor=1.0, kind="bce", pw_t=1.0, pw_g=7.0,
                                                              unit=False, grad_loss=(0, 1, 0))),
             (opt.MaskedBceWithLogits, (7,), (gt, None), dict(pred=pred, teacher=None, gt=gt, alpha=0.0, mask=None,
                                                              background_factor=1.0, kind="bce", pw_t=1.0, pw_g=7.0,
                                                              unit=False, grad_loss=(0, 1, 0))),
             (opt.DistillationLoss, (), (teacher, gt, 0.25, mask), dict(pred=pred, teacher=teacher, gt=gt, alpha=0.25,
                                                                        mask=mask, background_factor=1.0, kind="mse",
                                                                        pw_t=1.0, pw_g=1.0, unit=False)),
             (opt.DistillationLossKeypointMining, (), (teacher2, gt2, 0.5, mask2, 0.25),
              dict(pred=pred2, teacher=teacher2, gt=gt2, alpha=0.5, mask=mask2, background_factor=0.25, kind="mse", pw_t=1.0,
                   pw_g=1.0, unit=False)),
             (opt.DistillationBceLossKeypointMining, (7, 1), (teacher2, gt2, 0.5, mask2, 0.25),
              dict(pred=pred2, teacher=teacher2, gt=gt2, alpha=0.5, mask=mask2, background_factor=0.25, kind="bce", pw_t=7.0,
                   pw_g=1.0, unit=True))]
    for cls, ctor, args, rest in calls:
        d_args = [dev(x) if isinstance(x, np.ndarray) else x for x in args]
        p = dev(rest["pred"]).requires_grad_()
        plain = cls(*ctor)(p.detach(), *d_args)
        loss = cls(*ctor, differentiable=True)(p, *d_args)
        assert plain.grad_fn is None and loss.grad_fn is not None and loss.dim() == 0 and loss.dtype == torch.float32
        assert loss.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), cls.__name__
        loss.backward()
        v64, mag = GR.grad(**rest)
        me = R.normalise(rest["gt"], rest["teacher"], rest["mask"], rest["background_factor"], rest["unit"])[2]
        assert p.grad.is_contiguous() and p.grad.shape == p.shape
        check_gradient(p.grad.cpu().numpy(), v64, mag, rest["kind"], J, me, cls.__name__)
        for x, src in zip(d_args, args):                    # the caller's tensors, the mask among them, are never written
            assert not isinstance(src, np.ndarray) or np.array_equal(x.cpu().numpy(), src)
    print("measured so far:", measured)


def test_training_step_order_and_parameter_gradients(nat):
    """att = wa xa and det = wd xd + bd with per-channel leaf parameters, the two scalars of the training step, first the
    segmentation loss's backward with the graph retained, then the detection loss's"""
    from rtpe import distill
    case = R.TARGET_CASES[0]
    image_hw, det_hw, att_hw, _ = case
    people, teacher, mask, segm = R.target_inputs(case)
    tg = distill.distillation_targets(distill.JointTable(people, R.TARGET_J).to(DEV), image_hw, det_hw, att_hw,
                                      dev(teacher), dev(mask), dev(segm))
    w = GR.target_maps(0)
    J = R.TARGET_J
    rng = np.random.default_rng(7)
    xa = rng.normal(0, 2, (4, 1) + att_hw).astype(np.float32)
    xd = rng.normal(0, 2, (4, J + 1) + det_hw).astype(np.float32)
    for kind in R.LOSS_KINDS:
        wa = dev(np.array(0.8, np.float32).reshape(1, 1, 1, 1)).requires_grad_()
        wd = dev(rng.uniform(0.5, 1.5, (1, J + 1, 1, 1)).astype(np.float32)).requires_grad_()
        bd = dev(rng.normal(0, 0.3, (1, J + 1, 1, 1)).astype(np.float32)).requires_grad_()
        att = wa * dev(xa)
        det = wd * dev(xd) + bd
        att.retain_grad()
        det.retain_grad()
        seg, dl = distill.distillation_losses(att, det, tg, 0.5, 1, 7, 0.25, kind, differentiable=True)
        plain = distill.distillation_losses(att.detach(), det.detach(), tg, 0.5, 1, 7, 0.25, kind)
        assert seg.item() == plain[0].item() and dl.item() == plain[1].item()
        seg.backward(retain_graph=True)
        assert det.grad is None and wd.grad is None
        dl.backward(retain_graph=True)
        att_np, det_np = att.detach().cpu().numpy(), det.detach().cpu().numpy()
        ga, ma = GR.grad(att_np, None, w["segm"], 0.0, None, 1.0, "bce", 1.0, 7.0, unit=False, grad_loss=(0, 1, 0))
        gd, md = GR.grad(det_np, w["teacher"], w["gt"], 0.5, w["mask"], 0.25, kind, 1.0, 1.0)
        me = R.normalise(w["gt"], w["teacher"], w["mask"], 0.25, kind == "bce")[2]
        check_gradient(att.grad.cpu().numpy(), ga, ma, "bce", 1, None, "att")
        check_gradient(det.grad.cpu().numpy(), gd, md, kind, J, me, "det")
        assert not det.grad[:, J:].cpu().numpy().view(np.int32).any()          # the tag channel
        # the parameters: float32 sums over n_terms products against the float64 sums of the restated terms
        for name, param, t64 in (("wa", wa, ga * xa.astype(np.float64)), ("wd", wd, gd * xd.astype(np.float64)),
                                 ("bd", bd, gd)):
            want = t64.sum(axis=(0, 2, 3), keepdims=True)
            n_terms = t64.size // t64.shape[1]
            allow = n_terms * 2.0 ** -24 * np.abs(t64).sum(axis=(0, 2, 3), keepdims=True)
            got = param.grad.cpu().numpy().astype(np.float64)
            print("%s %s: largest distance %.3g of the allowance" % (kind, name, (np.abs(got - want) / np.maximum(allow, 1e-300)).max()))
            assert (np.abs(got - want) <= allow).all(), (kind, name)
        assert wd.grad[0, J].item() == 0 and bd.grad[0, J].item() == 0 and wd.grad[0, :J].abs().min().item() > 0
        once = [p.grad.clone() for p in (wa, wd, bd)]
        seg.backward()
        dl.backward()
        for p, g in zip((wa, wd, bd), once):
            assert torch.equal(p.grad, g + g)


class Spy:
    """the loaded library, remembering which entries were asked for"""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self.lib, name)


def test_without_a_gradient_it_is_the_plain_forward(nat, monkeypatch):
    from rtpe import distill, optimization as opt
    pred, teacher, gt, mask = (dev(a) for a in R.loss_inputs(R.LOSS_SHAPES[0], "both", "n1"))
    spy = Spy(nat.lib())
    monkeypatch.setattr(nat, "lib", lambda: spy)
    fn = opt.DistillationBceLossKeypointMining(7, 1, differentiable=True)
    live = pred.clone().requires_grad_()
    with torch.no_grad():
        a = fn(live, teacher, gt, 0.5, mask, 0.25)
        va = distill.loss_values("bce", live, teacher, gt, 0.5, mask, 0.25, differentiable=True)
    b = fn(pred, teacher, gt, 0.5, mask, 0.25)
    vb = distill.loss_values("bce", pred, teacher, gt, 0.5, mask, 0.25, differentiable=True)
    for v in (a, b, va.f32, vb.f32):
        assert v.grad_fn is None and not v.requires_grad
    assert va.gt is None and va.teacher is None and va.mask is None and vb.gt is None and vb.mask is None
    assert spy.names == ["rtpe_distill_loss"] * 4
    c = fn(live, teacher, gt, 0.5, mask, 0.25)
    assert spy.names == ["rtpe_distill_loss"] * 5 and c.grad_fn is not None         # the backward launches in backward()
    c.backward()
    assert spy.names[5:] == ["rtpe_distill_loss_backward"] and a.item() == b.item() == c.item()
    assert torch.equal(mask, dev(R.loss_inputs(R.LOSS_SHAPES[0], "both", "n1")[3]))


def test_an_in_place_write_before_backward_is_caught(nat):
    from rtpe import optimization as opt
    pred, teacher, gt, mask = (dev(a) for a in R.loss_inputs(R.LOSS_SHAPES[0], "neither", "nj"))
    leaf = pred.clone().requires_grad_()
    x = leaf * 1.0
    loss = opt.DistillationLoss(differentiable=True)(x, teacher, gt, 0.25, mask)
    with torch.no_grad():
        x.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    assert leaf.grad is None
