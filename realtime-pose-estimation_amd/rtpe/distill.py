"""Distillation targets and the forward values of the distillation losses on the device.

What the reference's dataset and training step do per image on the host - Gaussian ground-truth maps stamped by numpy
loops, the teacher's maps resized to the image, three more resizes down to the students' output grids, the masked and
normalised loss - as launches of csrc/distill.hip (include/rtpe_hip_distill.h; the rules: DESIGN.md section 4,
"Distillation targets and losses").  The teacher's maps come from the live teacher and never exist at image resolution.

By default forward values only: validation and monitoring.  ``loss_values`` and ``distillation_losses`` take
``differentiable=True`` for the gradient with respect to the student's output, one launch of csrc/distill_grad.hip
(include/rtpe_hip_distill_grad.h; DESIGN.md section 4, "Distillation losses: backward"); no gradient flows to a target,
a mask, or through any other function here.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _native

KINDS = {"bce": _native.DISTILL_BCE, "mse": _native.DISTILL_MSE}
DistillTargets = namedtuple("DistillTargets", "gt teacher mask segm minmax")
LossValues = namedtuple("LossValues", "f64 f32 gt teacher mask")

_patches = {}           # (sigma, device) -> the uploaded patch table


def patch_table(sigma):
    """the (S, S) float64 table of a sigma: S = len(arange(0, 6 sigma + 3)), a Gaussian around 3 sigma + 1"""
    sigma = float(sigma)
    if not 0 < sigma or not 6 * sigma + 3 <= _native.DISTILL_MAX_PATCH:
        raise ValueError("distill: stddev_pixels = %r must be positive with a table of at most %d entries per side"
                         % (sigma, _native.DISTILL_MAX_PATCH))
    x = np.arange(0, 6 * sigma + 3, 1, float)
    y = x[:, np.newaxis]
    c = 3 * sigma + 1
    return np.exp(-((x - c) ** 2 + (y - c) ** 2) / (2 * sigma ** 2))


def _patch_on(sigma, device):
    key = (float(sigma), device)
    if key not in _patches:
        _patches[key] = torch.from_numpy(patch_table(sigma).astype(np.float32)).to(device)
    return _patches[key]


class JointTable:
    """the people of a batch as a CSR table: ``offsets (N + 1) int32``, ``joints (P, J, 3) float64`` = (x, y, v) per
    joint, the people of image n in rows ``offsets[n]:offsets[n + 1]``.  Built from one (P_n, J, 3) array per image (an
    image without people: an empty list or a (0, J, 3) array).  ``to(device)`` returns the table on a GPU."""

    def __init__(self, people_per_image, num_joints=17):
        self.num_joints = int(num_joints)
        rows, counts = [], []
        for n, people in enumerate(people_per_image):
            a = np.asarray(people, np.float64)
            if a.size == 0:
                a = np.zeros((0, self.num_joints, 3))
            if a.ndim != 3 or a.shape[1:] != (self.num_joints, 3):
                raise ValueError("JointTable: the people of image %d have shape %s, (P, %d, 3) is needed"
                                 % (n, a.shape, self.num_joints))
            if not np.isfinite(a).all():
                raise ValueError("JointTable: image %d has a joint that is not finite" % n)
            rows.append(a)
            counts.append(len(a))
        if not counts:
            raise ValueError("JointTable: no images")
        self.offsets = np.zeros(len(counts) + 1, np.int32)
        self.offsets[1:] = np.cumsum(counts)
        self.joints = np.concatenate(rows) if rows else np.zeros((0, self.num_joints, 3))
        self.device = None
        self.offsets_t = self.joints_t = None

    def __len__(self):
        return len(self.offsets) - 1

    def people(self, n):
        return self.joints[self.offsets[n]:self.offsets[n + 1]]

    @classmethod
    def from_coco(cls, gt, image_ids):
        """the people the reference's dataset draws for each image id of a ``CocoKeypointGT``: the annotations with
        ``iscrowd == 0 or num_keypoints > 0``, in source order"""
        per_image = []
        for i in image_ids:
            anns = gt.anns[int(i)]
            per_image.append([np.asarray(a["keypoints"], np.float64).reshape(-1, 3) for a in anns
                              if a.get("iscrowd", 0) == 0 or a["num_keypoints"] > 0])
        return cls(per_image, 17)

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("rtpe: a JointTable moves to a GPU only, not to %s (there is deliberately no CPU "
                               "fallback in the product path)" % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = JointTable.__new__(JointTable)
        t.num_joints, t.offsets, t.joints, t.device = self.num_joints, self.offsets, self.joints, device
        t.offsets_t = torch.from_numpy(self.offsets).to(device)
        pad = self.joints if len(self.joints) else np.zeros((1, self.num_joints, 3))   # (a pointer the entry accepts)
        t.joints_t = torch.from_numpy(np.ascontiguousarray(pad)).to(device)
        return t


def _hw(name, hw):
    try:
        h, w = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError("distill: %s = %r is not a (height, width) pair" % (name, hw)) from None
    if h <= 0 or w <= 0:
        raise ValueError("distill: %s = %r must be positive" % (name, hw))
    return h, w


def _check_table(table, who):
    if not isinstance(table, JointTable):
        raise TypeError("%s: the people table must be a JointTable, not %s" % (who, type(table).__name__))
    if table.device is None:
        raise RuntimeError("%s: the JointTable is on the host; move it with .to(device) (there is deliberately no CPU "
                           "fallback in the product path)" % who)


def _check_tensor(t, name, who, shape=None, ndim=4):
    """dtype, shape and contiguity (which need no GPU to judge); the device is checked after them"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a tensor, not %s" % (who, name, type(t).__name__))
    if t.dtype != torch.float32:
        raise ValueError("%s: %s must be float32, not %s" % (who, name, t.dtype))
    if t.dim() != ndim or not t.numel():
        raise ValueError("%s: %s must have %d non-empty dimensions, not shape %s" % (who, name, ndim, tuple(t.shape)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %s has shape %s, %s is needed" % (who, name, tuple(t.shape), tuple(shape)))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))


def _wants_grad(t):
    return torch.is_grad_enabled() and bool(getattr(t, "requires_grad", False))


def _no_grad(who, *tensors):
    if any(_wants_grad(t) for t in tensors):
        raise NotImplementedError("%s: forward value only - an input requires grad and grad mode is on; call it under "
                                  "torch.no_grad() or detach the input (the losses take differentiable=True for a "
                                  "gradient with respect to student_pred)" % who)


def _no_grad_but_pred(who, **named):
    """differentiable=True: only ``student_pred`` gets a gradient"""
    for name, t in named.items():
        if _wants_grad(t):
            raise NotImplementedError("%s: %s requires grad and grad mode is on; differentiable=True gives the gradient "
                                      "with respect to student_pred only - detach %s" % (who, name, name))


def _ptr(t):
    return None if t is None else t.data_ptr()


def gt_heatmaps(table, image_hw, stddev_pixels=2.0, out=None):
    """(N, J, H, W) float32 ground-truth maps of a ``JointTable`` on its device: one launch"""
    who = "gt_heatmaps"
    _check_table(table, who)
    H, W = _hw("image_hw", image_hw)
    patch = patch_table(stddev_pixels)
    N, J = len(table), table.num_joints
    if out is None:
        out = torch.empty((N, J, H, W), dtype=torch.float32, device=table.device)
    else:
        _check_tensor(out, "out", who, (N, J, H, W))
        _native.require_gpu(out, who)
        _native.same_device(who, table.joints_t, out)
    with _native.on_device(out):
        _native.check(_native.lib().rtpe_gt_heatmaps(
            table.offsets_t.data_ptr(), table.joints_t.data_ptr(), len(table.joints), N, J, H, W,
            _patch_on(stddev_pixels, table.device).data_ptr(), len(patch), float(stddev_pixels), out.data_ptr(),
            _native.stream_ptr(out.device)))
    return out


def distillation_targets(table, image_hw, det_hw, att_hw=None, teacher=None, mask=None, segm=None, stddev_pixels=2.0):
    """The targets of one batch of N images of one size ``image_hw`` as a ``DistillTargets`` of device tensors:

    * ``gt (N, J, h, w)``: the ground-truth maps of ``table`` (a ``JointTable`` on the device, or None) at ``det_hw``;
    * ``teacher (N, J, h, w)``: ``teacher`` (N, J, ht, wt), the live teacher's ``refined`` map at its own size, resized
      to the image with align_corners=True and on to ``det_hw`` with align_corners=False;
    * ``mask (N, 1, h, w)`` from ``mask`` (N, H, W) and ``segm (N, 1, ha, wa)`` from ``segm`` (N, H, W), ``att_hw``;
    * ``minmax (4,)``: min and max of ``gt`` and of ``teacher``, which the BCE loss normalises by.

    Every input may be None, and so is its output.  Bit-identical to the reference's chain of host loops and
    ``F.interpolate`` calls on PyTorch-CPU; nothing is read back."""
    who = "distillation_targets"
    H, W = _hw("image_hw", image_hw)
    h, w = _hw("det_hw", det_hw)
    ha, wa = _hw("att_hw", att_hw) if att_hw is not None else (0, 0)
    if segm is not None and att_hw is None:
        raise ValueError("%s: segm needs att_hw" % who)
    patch = patch_table(stddev_pixels)
    if table is not None:
        _check_table(table, who)
    given = [t for t in (teacher, mask, segm) if t is not None]
    if table is None and not given:
        raise ValueError("%s: nothing to compute: table, teacher, mask and segm are all None" % who)
    _no_grad(who, *given)
    N = len(table) if table is not None else given[0].shape[0]
    J = table.num_joints if table is not None else (teacher.shape[1] if teacher is not None and teacher.dim() == 4 else 1)
    if teacher is not None:
        _check_tensor(teacher, "teacher", who)
        if tuple(teacher.shape[:2]) != (N, J):
            raise ValueError("%s: teacher has shape %s, (%d, %d, ht, wt) is needed" % (who, tuple(teacher.shape), N, J))
    if mask is not None:
        _check_tensor(mask, "mask", who, (N, H, W), ndim=3)
    if segm is not None:
        _check_tensor(segm, "segm", who, (N, H, W), ndim=3)
    for t in given:
        _native.require_gpu(t, who)
    device = table.device if table is not None else given[0].device
    first = table.joints_t if table is not None else given[0]
    _native.same_device(who, first, *given)
    L = _native.lib()

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=device)
    gt_out = new(N, J, h, w) if table is not None else None
    teacher_out = new(N, J, h, w) if teacher is not None else None
    mask_out = new(N, 1, h, w) if mask is not None else None
    segm_out = new(N, 1, ha, wa) if segm is not None else None
    minmax = new(4)
    sb = ctypes.c_size_t()
    _native.check(L.rtpe_distill_targets_scratch_bytes(N, J, h, w, ctypes.byref(sb)))
    scratch = torch.empty((sb.value,), dtype=torch.uint8, device=device)
    ht, wt = teacher.shape[2:] if teacher is not None else (0, 0)
    with _native.on_device(minmax):
        _native.check(L.rtpe_distill_targets(
            _ptr(table.offsets_t) if table is not None else None, _ptr(table.joints_t) if table is not None else None,
            len(table.joints) if table is not None else 0,
            _patch_on(stddev_pixels, device).data_ptr() if table is not None else None,
            len(patch) if table is not None else 0, float(stddev_pixels), _ptr(teacher), ht, wt, _ptr(mask), _ptr(segm),
            N, J, H, W, h, w, ha, wa, _ptr(gt_out), _ptr(teacher_out), _ptr(mask_out), _ptr(segm_out), minmax.data_ptr(),
            scratch.data_ptr(), sb.value, _native.stream_ptr(device)))
    return DistillTargets(gt_out, teacher_out, mask_out, segm_out, minmax)


def _check_loss_inputs(who, pred, teacher, gt, mask, alpha, background_factor, minmax=None, more_channels=True,
                       differentiable=False):
    if not 0 <= alpha <= 1:
        raise ValueError("%s: alpha = %r outside [0, 1]" % (who, alpha))
    if not 0 <= background_factor <= 1:
        raise ValueError("%s: background_factor = %r outside [0, 1]" % (who, background_factor))
    if differentiable:
        _no_grad_but_pred(who, teacher_pred=teacher, gt=gt, mask=mask, minmax=minmax)
    else:
        _no_grad(who, pred, teacher, gt, mask)
    _check_tensor(gt, "gt", who)
    N, J, h, w = gt.shape
    if pred is not None:
        _check_tensor(pred, "student_pred", who)
        ok = pred.shape[0] == N and tuple(pred.shape[2:]) == (h, w) and \
            (pred.shape[1] >= J if more_channels else pred.shape[1] == J)
        if not ok:
            raise ValueError("%s: student_pred has shape %s, (%d, %s%d, %d, %d) is needed"
                             % (who, tuple(pred.shape), N, ">= " if more_channels else "", J, h, w))
    if teacher is not None:
        _check_tensor(teacher, "teacher_pred", who, (N, J, h, w))
    if mask is not None:
        _check_tensor(mask, "mask", who)
        if tuple(mask.shape) not in ((N, 1, h, w), (N, J, h, w)):
            raise ValueError("%s: mask has shape %s, (%d, 1 or %d, %d, %d) is needed" % (who, tuple(mask.shape), N, J, h, w))
    if minmax is not None:
        _check_tensor(minmax, "minmax", who, (4,), ndim=1)
    tensors = [t for t in (pred, teacher, gt, mask, minmax) if t is not None]
    for t in tensors:
        _native.require_gpu(t, who)
    _native.same_device(who, gt, *tensors)


def normalise(gt, teacher=None, mask=None, background_factor=1.0, minmax=None):
    """steps 1 to 3 of the BCE distillation loss without the products: ``(gt, teacher, mask)`` with both targets
    shifted and scaled into [0, 1] where they leave it (over the whole tensor) and the mask, expanded to (N, J, h, w),
    times ``background_factor`` where the normalised ``gt`` is 0.  None stays None; no input is written."""
    who = "normalise"
    _check_loss_inputs(who, None, teacher, gt, mask, 0.0, background_factor, minmax)
    N, J, h, w = gt.shape
    outs = [torch.empty_like(gt), None if teacher is None else torch.empty_like(gt),
            None if mask is None else torch.empty_like(gt)]
    scratch = torch.empty((_native.DISTILL_SCRATCH_BYTES,), dtype=torch.uint8, device=gt.device)
    with _native.on_device(gt):
        _native.check(_native.lib().rtpe_distill_normalise(
            gt.data_ptr(), _ptr(teacher), _ptr(mask), mask.shape[1] if mask is not None else 1, N, J, h, w,
            float(background_factor), _ptr(minmax), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), scratch.data_ptr(),
            scratch.numel(), _native.stream_ptr(gt.device)))
    return tuple(outs)


class _LossWithGrad(torch.autograd.Function):
    """the float32 loss vector of ``loss_values`` as a differentiable function of ``student_pred`` alone.  The forward
    is the plain one with ``keep``; the backward is one launch of rtpe_distill_loss_backward on what the forward kept
    ("Distillation losses: backward")."""

    @staticmethod
    def forward(ctx, pred, spec):
        v = _loss_forward(pred, keep=True, **spec)
        # the scalars only: the caller's tensors in `spec` must not live as long as the graph does
        ctx.scalars = (KINDS[spec["kind"]], float(spec["alpha"]), float(spec["teacher_pos_weight"]),
                       float(spec["gt_pos_weight"]))
        ctx.save_for_backward(pred, v.gt, v.teacher, v.mask)       # (the version check sees a write in between)
        ctx.mark_non_differentiable(*[t for t in (v.f64, v.gt, v.teacher, v.mask) if t is not None])
        return v.f32, v.f64, v.gt, v.teacher, v.mask

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_f32, *_):
        pred, gt_n, teacher_n, mask_eff = ctx.saved_tensors
        kind, alpha, pw_t, pw_g = ctx.scalars
        # (a missing upstream gradient arrives as zeros: autograd materialises it)
        grad_f32 = grad_f32.to(device=pred.device, dtype=torch.float32).contiguous()
        grad_pred = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
        N, J, h, w = gt_n.shape
        with _native.on_device(pred):
            _native.check(_native.lib().rtpe_distill_loss_backward(
                kind, pred.data_ptr(), pred.shape[1], _ptr(teacher_n), gt_n.data_ptr(), _ptr(mask_eff),
                N, J, h, w, alpha, pw_t, pw_g, grad_f32.data_ptr(), grad_pred.data_ptr(), _native.stream_ptr(pred.device)))
        return grad_pred, None


def loss_values(kind, pred, teacher, gt, alpha=0.5, mask=None, background_factor=1.0, teacher_pos_weight=1.0,
                gt_pos_weight=1.0, unit=None, minmax=None, keep=False, more_channels=True, who="loss_values",
                differentiable=False):
    """One masked distillation loss: a ``LossValues`` whose ``f64`` and ``f32`` are device tensors
    ``[teacher_loss, gt_loss, alpha * teacher_loss + (1 - alpha) * gt_loss]``.  ``kind``: "bce" (with logits and a
    pos_weight per term) or "mse"; ``unit``: normalise the targets first (default: for "bce"); ``teacher`` None: its
    loss is 0; ``keep``: also return the normalised targets and the effective mask.  The host waits for nothing.

    ``differentiable``: with a ``pred`` that requires grad while grad mode is on, ``f32`` (the same bits) carries a
    gradient with respect to ``pred`` - and to nothing else; the normalised targets and the effective mask are kept for
    the backward, three (N, J, h, w) float32 tensors at most.  Otherwise, and by default, forward value only."""
    if kind not in KINDS:
        raise ValueError("%s: kind = %r is neither 'bce' nor 'mse'" % (who, kind))
    _check_loss_inputs(who, pred, teacher, gt, mask, alpha, background_factor, minmax, more_channels, differentiable)
    unit = kind == "bce" if unit is None else bool(unit)
    spec = dict(kind=kind, teacher=teacher, gt=gt, alpha=alpha, mask=mask, background_factor=background_factor,
                teacher_pos_weight=teacher_pos_weight, gt_pos_weight=gt_pos_weight, unit=unit, minmax=minmax)
    if differentiable and _wants_grad(pred):
        f32, f64, gt_n, teacher_n, mask_eff = _LossWithGrad.apply(pred, spec)
        return LossValues(f64, f32, gt_n, teacher_n, mask_eff)
    return _loss_forward(pred, keep=keep, **spec)


def _loss_forward(pred, kind, teacher, gt, alpha, mask, background_factor, teacher_pos_weight, gt_pos_weight, unit, minmax,
                  keep):
    """the launches of ``loss_values`` on checked inputs"""
    N, J, h, w = gt.shape
    outs = [None, None, None]
    if keep:
        outs = [torch.empty_like(gt), None if teacher is None else torch.empty_like(gt),
                None if mask is None else torch.empty_like(gt)]
    buf = torch.empty((_native.DISTILL_LOSS_BYTES // 8,), dtype=torch.float64, device=gt.device)
    scratch = torch.empty((_native.DISTILL_SCRATCH_BYTES,), dtype=torch.uint8, device=gt.device)
    with _native.on_device(gt):
        _native.check(_native.lib().rtpe_distill_loss(
            KINDS[kind], int(unit), pred.data_ptr(), pred.shape[1], _ptr(teacher), gt.data_ptr(), _ptr(mask),
            mask.shape[1] if mask is not None else 1, N, J, h, w, float(alpha), float(background_factor),
            float(teacher_pos_weight), float(gt_pos_weight), _ptr(minmax) if unit else None, _ptr(outs[0]),
            _ptr(outs[1]), _ptr(outs[2]), buf.data_ptr(), scratch.data_ptr(), scratch.numel(),
            _native.stream_ptr(gt.device)))
    return LossValues(buf[:3], buf.view(torch.float32)[6:9], *outs)


def distillation_losses(att, det, targets, alpha=0.5, det_pos_weight=1, att_pos_weight=7, background_factor=1,
                        kind="bce", differentiable=False):
    """``(segmentation_loss, detection_loss)``, the two scalars of the reference's training step, as 0-d float32 device
    tensors: BCE-with-logits (pos_weight ``att_pos_weight``) of ``att`` against ``targets.segm``, and the keypoint-mining
    distillation loss of ``det`` (its channels [0, J), read in place) against ``targets.teacher`` and ``targets.gt``
    under ``targets.mask``.  ``kind="mse"`` is ``DistillationLossKeypointMining``.  A loss whose targets are absent is
    None.  ``differentiable``: an ``att`` / ``det`` that requires grad gets its gradient from the scalar's
    ``.backward()`` (a tag channel of ``det``: zeros); by default such an input is refused."""
    who = "distillation_losses"
    if not isinstance(targets, DistillTargets):
        raise TypeError("%s: targets must be what distillation_targets returned" % who)
    seg = None
    if att is not None and targets.segm is not None:
        seg = loss_values("bce", att, None, targets.segm, 0.0, None, 1.0, 1.0, att_pos_weight, unit=False,
                          more_channels=False, who=who, differentiable=differentiable).f32[1]
    det_loss = None
    if det is not None and targets.gt is not None:
        det_loss = loss_values(kind, det, targets.teacher, targets.gt, alpha, targets.mask, background_factor,
                               det_pos_weight, det_pos_weight, minmax=targets.minmax, who=who,
                               differentiable=differentiable).f32[2]
    return seg, det_loss
