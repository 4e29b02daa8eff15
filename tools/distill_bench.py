#!/usr/bin/env python
"""Distillation targets and losses: the one-call device path against the pieces a user had before it.

    python tools/distill_bench.py [--out profiles/distill_bench.json] [--batch 32] [--reps 20]

One batch: 32 images of 320x320 with 0-20 people each, the teacher's maps at 160x160, `det` at 80x80 with a tag channel,
`att` at 160x160.  Both paths start from the people on the host and the teacher's maps, masks and student outputs on the
device, and end with the two loss scalars on the device (timed to a device synchronise):

  A  rtpe.distill: JointTable (+ upload), distillation_targets, distillation_losses
  B  the host stamp loops per image (numpy, as the reference's dataset does), one upload of the (N, 17, H, W) maps,
     F.interpolate on the GPU for the five resizes, and the reference's loss formula in torch ops

run A B B A; the rates are batches of images per second.  The device times of A's two native stages are taken with
events in a separate loop.  Needs a GPU; there is no fallback.
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
for p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

J, IMAGE, DET, ATT, SRC, SIGMA = 17, (320, 320), (80, 80), (160, 160), (160, 160), 2.0


def make_batch(n, seed=0):
    rng = np.random.default_rng(seed)
    people = []
    for _ in range(n):
        p = int(rng.integers(0, 21))
        a = np.empty((p, J, 3))
        a[..., 0] = rng.uniform(-5, IMAGE[1] + 5, (p, J))
        a[..., 1] = rng.uniform(-5, IMAGE[0] + 5, (p, J))
        a[..., 2] = rng.integers(0, 3, (p, J))
        people.append(a)
    dev = "cuda:0"
    t = dict(teacher=torch.from_numpy(rng.normal(0.1, 0.3, (n, J) + SRC).astype(np.float32)).to(dev),
             mask=torch.from_numpy((rng.random((n,) + IMAGE) > 0.1).astype(np.float32)).to(dev),
             segm=torch.from_numpy((rng.random((n,) + IMAGE) > 0.7).astype(np.float32)).to(dev),
             att=torch.from_numpy(rng.random((n, 1) + ATT).astype(np.float32)).to(dev),
             det=torch.from_numpy(rng.normal(0, 2, (n, J + 1) + DET).astype(np.float32)).to(dev))
    return people, t


def path_a(people, t, alpha, pw):
    from rtpe import distill
    table = distill.JointTable(people, J).to("cuda:0")
    tg = distill.distillation_targets(table, IMAGE, DET, ATT, t["teacher"], t["mask"], t["segm"], SIGMA)
    return distill.distillation_losses(t["att"], t["det"], tg, alpha, pw, 7, 1, "bce")


def _unit(x):
    if x.min() < 0:
        x = x - x.min()
    if x.max() > 1:
        x = x / x.max()
    return x


def path_b(people, t, alpha, pw):
    import distill_restated as R
    maps = np.stack([R.gt_heatmaps(p, J, IMAGE, SIGMA) for p in people])
    hms = torch.from_numpy(maps).to("cuda:0")
    teacher = F.interpolate(t["teacher"], IMAGE, mode="bilinear", align_corners=True)
    segm = F.interpolate(t["segm"][:, None], ATT, mode="bilinear")
    gt = _unit(F.interpolate(hms, DET, mode="bilinear"))
    teacher = _unit(F.interpolate(teacher, DET, mode="bilinear"))
    mask = F.interpolate(t["mask"][:, None], DET, mode="bilinear").expand(gt.shape).clone()
    mask[gt == 0] *= 1.0
    weight = torch.full((1,), float(pw), device="cuda:0")
    pred = t["det"][:, :J] * mask
    seg = F.binary_cross_entropy_with_logits(t["att"], segm, pos_weight=torch.full((1,), 7.0, device="cuda:0"))
    det = alpha * F.binary_cross_entropy_with_logits(pred, teacher * mask, pos_weight=weight) + \
        (1 - alpha) * F.binary_cross_entropy_with_logits(pred, gt * mask, pos_weight=weight)
    return seg, det


def timed(fn, reps, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def device_times(people, t, alpha, pw, reps):
    from rtpe import distill
    table = distill.JointTable(people, J).to("cuda:0")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tt = tl = 0.0
    for _ in range(reps):
        ev[0].record()
        tg = distill.distillation_targets(table, IMAGE, DET, ATT, t["teacher"], t["mask"], t["segm"], SIGMA)
        ev[1].record()
        distill.distillation_losses(t["att"], t["det"], tg, alpha, pw, 7, 1, "bce")
        ev[2].record()
        torch.cuda.synchronize()
        tt += ev[0].elapsed_time(ev[1])
        tl += ev[1].elapsed_time(ev[2])
    return tt / reps, tl / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-b", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_bench: needs a GPU; nothing is measured without one")
    import __graft_entry__ as g
    g.build()
    import distill_restated as R
    people, t = make_batch(a.batch)
    alpha, pw = 0.5, 1.0
    for fn in (path_a, path_b):                 # warm-up: code objects, the allocator, the patch table
        fn(people, t, alpha, pw)
    runs = []
    for name, fn, reps in (("A", path_a, a.reps), ("B", path_b, a.reps_b), ("B", path_b, a.reps_b), ("A", path_a, a.reps)):
        s, out = timed(fn, reps, people, t, alpha, pw)
        runs.append(dict(path=name, seconds_per_batch=s, images_per_second=a.batch / s,
                         segmentation_loss=float(out[0]), detection_loss=float(out[1])))
    t_targets, t_losses = device_times(people, t, alpha, pw, a.reps)
    # the same two scalars from the float64 restatement (the targets at the grids from the device path itself)
    from rtpe import distill
    tg = distill.distillation_targets(distill.JointTable(people, J).to("cuda:0"), IMAGE, DET, ATT, t["teacher"], t["mask"],
                                      t["segm"], SIGMA)
    det64 = distill.loss_values("bce", t["det"], tg.teacher, tg.gt, alpha, tg.mask, 1.0, pw, pw, minmax=tg.minmax).f64
    want = R.distillation_loss(t["det"].cpu().numpy(), tg.teacher.cpu().numpy(), tg.gt.cpu().numpy(), alpha,
                               tg.mask.cpu().numpy(), 1.0, "bce", pw, pw)[2]
    n = tg.gt.numel()
    res = dict(batch=a.batch, image_hw=IMAGE, det_hw=DET, att_hw=ATT, teacher_source_hw=SRC, people_per_image="0-20",
               people_total=int(sum(len(p) for p in people)), order="A B B A", runs=runs,
               A_images_per_second=float(np.mean([r["images_per_second"] for r in runs if r["path"] == "A"])),
               B_images_per_second=float(np.mean([r["images_per_second"] for r in runs if r["path"] == "B"])),
               A_device_ms=dict(distillation_targets=t_targets, distillation_losses=t_losses, how="events around the calls"),
               detection_loss_float64=float(det64[2]), detection_loss_restatement=want,
               detection_loss_relative_distance=abs(float(det64[2]) - want) / abs(want),
               detection_loss_derived_bound=R.loss_bound(n), device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
