"""The reference's loss classes (its ``rtpe/optimization.py``) on the device.

Constructors and ``forward`` signatures are the reference's.  ``forward`` takes contiguous float32 CUDA tensors of
shape (N, C, h, w) and returns a 0-d float32 CUDA tensor without a host synchronisation; the elements and their sum
are float64 on the device (csrc/distill.hip, DESIGN.md section 4, "Distillation targets and losses").  Differences, all
deliberate: the gradient is opt-in and goes to the student's output only - a class constructed as the reference
constructs it gives forward values and refuses an input that requires grad while grad mode is on; constructed with
``differentiable=True`` its result carries a gradient with respect to ``pred`` / ``student_pred`` (one launch of
csrc/distill_grad.hip in the backward, DESIGN.md section 4, "Distillation losses: backward"), and a target or mask that
requires grad is still refused; the caller's mask is never written (the reference multiplies the background factor
into it in place); and ``student_pred`` of the distillation classes may carry more channels than the targets -
channels [0, J) are read in place, the others get a zero gradient.  Optimisers and schedulers of the reference's
module are out of scope.
"""
import torch

from . import distill


def _pick_top(pick_top):
    if pick_top is not None:
        raise NotImplementedError("pick_top is not implemented (nor is it in the reference)")


class MaskedMseLoss(torch.nn.Module):
    """``MSELoss()(pred * mask, gt * mask)``; without a mask the plain mean squared error"""

    def __init__(self, differentiable=False):
        super().__init__()
        self.differentiable = bool(differentiable)

    def forward(self, pred, gt, mask=None):
        return distill.loss_values("mse", pred, None, gt, 0.0, mask, more_channels=False, who="MaskedMseLoss",
                                   differentiable=self.differentiable).f32[1]


class MaskedBceWithLogits(torch.nn.Module):
    """``BCEWithLogitsLoss(pos_weight)(pred * mask, gt * mask)``.  ``device`` is accepted and not used: the loss runs
    where its inputs are."""

    def __init__(self, pos_weight=1, device="cpu", differentiable=False):
        super().__init__()
        self.pos_weight = float(pos_weight)
        self.differentiable = bool(differentiable)

    def forward(self, pred, gt, mask=None):
        return distill.loss_values("bce", pred, None, gt, 0.0, mask, gt_pos_weight=self.pos_weight, unit=False,
                                   more_channels=False, who="MaskedBceWithLogits",
                                   differentiable=self.differentiable).f32[1]


class DistillationLoss(torch.nn.Module):
    """``alpha * MSE(student, teacher) + (1 - alpha) * MSE(student, gt)``, each masked; alpha is the teacher's weight"""
    kind = "mse"
    teacher_pos_weight = gt_pos_weight = 1.0

    def __init__(self, differentiable=False):
        super().__init__()
        self.differentiable = bool(differentiable)

    def forward(self, student_pred, teacher_pred, gt, alpha=0.5, mask=None):
        return self._value(student_pred, teacher_pred, gt, alpha, mask, 1.0, False)

    def _value(self, student_pred, teacher_pred, gt, alpha, mask, background_factor, unit):
        return distill.loss_values(self.kind, student_pred, teacher_pred, gt, alpha, mask, background_factor,
                                   self.teacher_pos_weight, self.gt_pos_weight, unit=unit,
                                   who=type(self).__name__, differentiable=self.differentiable).f32[2]


class DistillationLossKeypointMining(DistillationLoss):
    """DistillationLoss with the mask times ``background_factor`` wherever ``gt == 0``"""

    def forward(self, student_pred, teacher_pred, gt, alpha=0.5, mask=None, background_factor=0, pick_top=None):
        _pick_top(pick_top)
        return self._value(student_pred, teacher_pred, gt, alpha, mask, background_factor, False)


class DistillationBceLossKeypointMining(DistillationLoss):
    """the same with BCE-with-logits terms; the targets are first brought into [0, 1]: minus the minimum if it is
    negative, then over the maximum if it exceeds 1, each over the whole tensor; the background test sees the result"""
    kind = "bce"

    def __init__(self, teacher_pos_weight=1, gt_pos_weight=1, device="cpu", differentiable=False):
        super().__init__(differentiable)
        self.teacher_pos_weight, self.gt_pos_weight = float(teacher_pos_weight), float(gt_pos_weight)

    def forward(self, student_pred, teacher_pred, gt, alpha=0.5, mask=None, background_factor=0, pick_top=None):
        _pick_top(pick_top)
        return self._value(student_pred, teacher_pred, gt, alpha, mask, background_factor, True)
