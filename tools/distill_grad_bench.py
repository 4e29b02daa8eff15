#!/usr/bin/env python
"""The two losses of the training step with their gradients: the device path against torch ops with torch's autograd.

    python tools/distill_grad_bench.py [--out profiles/distill_grad_bench.json] [--batch 32] [--reps 20]

The batch of tools/distill_bench.py: 32 images of 320x320 with the seeded people, `det` at 80x80 with a tag channel,
`att` at 160x160.  The targets are computed once on the device (distillation_targets) and are not timed.  One step, timed
to a device synchronise, starts from leaf tensors `att` and `det` that require grad and ends with both gradients:

  A  rtpe.distill.distillation_losses(..., differentiable=True), then seg.backward() and det_loss.backward()
  B  the same two scalars from torch ops on the GPU - the normalisation and the background weighting of the reference's
     class, F.binary_cross_entropy_with_logits on the masked products - and the same two .backward() calls

run A B B A.  The device time of A's two backward launches is taken with events around the two launches alone: the C
entry called directly on the tensors the forwards kept, in a separate loop.  B's arithmetic is float32 in another order, so the distance between the gradients is information, not a
check.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import distill_bench as B0  # noqa: E402  (the batch)

ALPHA, PW, ATT_PW, BF = 0.5, 1.0, 7.0, 1.0


def leaves(t):
    return t["att"].detach().clone().requires_grad_(), t["det"].detach().clone().requires_grad_()


def step_a(t, tg):
    from rtpe import distill
    att, det = leaves(t)
    seg, dl = distill.distillation_losses(att, det, tg, ALPHA, PW, ATT_PW, BF, "bce", differentiable=True)
    seg.backward()
    dl.backward()
    return seg, dl, att.grad, det.grad


def step_b(t, tg):
    att, det = leaves(t)
    J = tg.gt.shape[1]
    gt, teacher = B0._unit(tg.gt), B0._unit(tg.teacher)
    mask = tg.mask.expand(gt.shape).clone()
    mask[gt == 0] *= BF
    pred = det[:, :J] * mask
    seg = F.binary_cross_entropy_with_logits(att, tg.segm, pos_weight=torch.full((1,), ATT_PW, device=att.device))
    weight = torch.full((1,), PW, device=att.device)
    dl = ALPHA * F.binary_cross_entropy_with_logits(pred, teacher * mask, pos_weight=weight) + \
        (1 - ALPHA) * F.binary_cross_entropy_with_logits(pred, gt * mask, pos_weight=weight)
    seg.backward()
    dl.backward()
    return seg, dl, att.grad, det.grad


def timed(fn, reps, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def backward_device_ms(t, tg, reps):
    """events around the two rtpe_distill_loss_backward launches alone (the C entry on the tensors the two forwards
    kept, back to back on one stream): no autograd, no accumulate kernels"""
    from rtpe import _native, distill
    att, det = t["att"], t["det"]
    seg = distill.loss_values("bce", att, None, tg.segm, 0.0, None, 1.0, 1.0, ATT_PW, unit=False, keep=True,
                              more_channels=False)
    dl = distill.loss_values("bce", det, tg.teacher, tg.gt, ALPHA, tg.mask, BF, PW, PW, minmax=tg.minmax, keep=True)
    up_seg = torch.tensor([0.0, 1.0, 0.0], device=att.device)
    up_det = torch.tensor([0.0, 0.0, 1.0], device=att.device)
    g_att, g_det = torch.empty_like(att), torch.empty_like(det)
    L, stream = _native.lib(), _native.stream_ptr(att.device)

    def launch(pred, v, alpha, pw_t, pw_g, up, out):
        N, J, h, w = v.gt.shape
        _native.check(L.rtpe_distill_loss_backward(
            _native.DISTILL_BCE, pred.data_ptr(), pred.shape[1], None if v.teacher is None else v.teacher.data_ptr(),
            v.gt.data_ptr(), None if v.mask is None else v.mask.data_ptr(), N, J, h, w, alpha, pw_t, pw_g, up.data_ptr(),
            out.data_ptr(), stream))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    total = 0.0
    for i in range(reps + 2):
        ev[0].record()
        launch(att, seg, 0.0, 1.0, ATT_PW, up_seg, g_att)
        launch(det, dl, ALPHA, PW, PW, up_det, g_det)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= 2:
            total += ev[0].elapsed_time(ev[1])
    return total / reps, g_att, g_det


def ulps(a, b):
    """largest distance between two float32 arrays in units of the spacing of the larger magnitude"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    unit = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return float((np.abs(a - b) / unit).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_grad_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_grad_bench: needs a GPU; nothing is measured without one")
    import __graft_entry__ as g
    g.build()
    from rtpe import distill
    people, t = B0.make_batch(a.batch)
    tg = distill.distillation_targets(distill.JointTable(people, B0.J).to("cuda:0"), B0.IMAGE, B0.DET, B0.ATT, t["teacher"],
                                      t["mask"], t["segm"], B0.SIGMA)
    for fn in (step_a, step_b, step_a, step_b):             # warm-up: code objects, the allocator, autograd's thread
        fn(t, tg)
    runs = []
    outs = {}
    for name, fn in (("A", step_a), ("B", step_b), ("B", step_b), ("A", step_a)):
        s, out = timed(fn, a.reps, t, tg)
        outs[name] = out
        runs.append(dict(path=name, ms_per_step=s * 1e3, segmentation_loss=float(out[0]), detection_loss=float(out[1])))
    ga = [x.cpu().numpy() for x in outs["A"][2:]]
    gb = [x.cpu().numpy() for x in outs["B"][2:]]
    launches_ms, g_att, g_det = backward_device_ms(t, tg, a.reps)
    same = bool(np.array_equal(g_att.cpu().numpy(), ga[0]) and np.array_equal(g_det.cpu().numpy(), ga[1]))
    res = dict(batch=a.batch, image_hw=B0.IMAGE, det_hw=B0.DET, att_hw=B0.ATT, det_channels=B0.J + 1, order="A B B A",
               reps=a.reps, runs=runs,
               A_ms_per_step=float(np.mean([r["ms_per_step"] for r in runs if r["path"] == "A"])),
               B_ms_per_step=float(np.mean([r["ms_per_step"] for r in runs if r["path"] == "B"])),
               A_backward_device_ms=dict(both_launches=launches_ms,
                                         how="events around the two rtpe_distill_loss_backward launches alone, the C entry "
                                             "called directly on the kept tensors, back to back on one stream",
                                         gradients_equal_those_of_backward=same),
               gradient_distance_A_vs_B_float32_ulps=dict(att=ulps(ga[0], gb[0]), det=ulps(ga[1], gb[1]),
                                                          note="B rounds in float32 in another order: information, not a check"),
               tag_channel_gradient_is_zero=bool(not ga[1][:, B0.J:].any()),
               device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
