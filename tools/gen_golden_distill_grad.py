#!/usr/bin/env python
"""Writes tests/golden/distill_grad.npz: the gradients the reference's loss classes give with PyTorch-CPU's autograd on
the loss test data of tests/distill_restated.py.

Build-container only: imports the reference checkout (read-only, never copied; REF below or argv[1]) the way
tools/gen_golden_distill.py does, runs its classes (rtpe/optimization.py) with ``pred.requires_grad_()`` and
``.backward()``, and compares ``pred.grad`` with the float64 restatement (tests/distill_grad_restated.py).

Per case the fixture holds ``ref_units``: the largest distance of the reference's float32 gradient from the restatement
in units of ``2^-24 * mag`` - the reference's own rounding, which is what the host test allows it.  For the shape
(2, 17, 10, 14) and rows 1 and 3 of LOSS_PARAMS (24 cases) and for the five plain-class calls it also holds the
reference's gradient itself.  Same inputs, same bytes.

    python tools/gen_golden_distill_grad.py [/path/to/reference]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_distill as G  # noqa: E402  (the stubbed import of the reference, the byte-stable npz writer)

sys.path.insert(0, os.path.join(G.ROOT, "tests"))
import distill_grad_restated as GR  # noqa: E402
import distill_restated as R  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "distill_grad.npz")


def ref_units(ref, v64, mag, key):
    d, den = np.abs(ref.astype(np.float64) - v64), 2.0 ** -24 * mag
    assert not d[den == 0].any(), key              # where the restatement is an exact zero, so is the reference
    u = float((d[den > 0] / den[den > 0]).max()) if (den > 0).any() else 0.0
    while not (d <= u * den).all():                # the quotient rounded down: the stored number satisfies its own test
        u = float(np.nextafter(u, np.inf))
    return u


def plain_calls(opt):
    """the five plain-class calls of tools/gen_golden_distill.py: name -> (class instance, takes a teacher, the
    arguments of the restatement)"""
    return {"mse": (opt.MaskedMseLoss(), False, True, dict(alpha=0.0, kind="mse", pw_g=1.0)),
            "mse_nomask": (opt.MaskedMseLoss(), False, False, dict(alpha=0.0, kind="mse", pw_g=1.0)),
            "bce7": (opt.MaskedBceWithLogits(7), False, True, dict(alpha=0.0, kind="bce", pw_g=7.0)),
            "bce7_nomask": (opt.MaskedBceWithLogits(7), False, False, dict(alpha=0.0, kind="bce", pw_g=7.0)),
            "distill": (opt.DistillationLoss(), True, True, dict(alpha=0.25, kind="mse", pw_g=1.0))}


def main():
    _, opt = G.import_reference()
    out, worst = {}, (0.0, None)
    for shape, mode, mask_mode, kind, pi in GR.all_cases():
        a = GR.case_args(shape, mode, mask_mode, kind, pi)
        J = shape[1]
        p = torch.from_numpy(a["pred"].copy()).requires_grad_()
        m = None if a["mask"] is None else torch.from_numpy(a["mask"]).expand(shape).clone()
        fn = opt.DistillationBceLossKeypointMining(a["pw_t"], a["pw_g"]) if kind == "bce" else \
            opt.DistillationLossKeypointMining()
        loss = fn(p[:, :J], torch.from_numpy(a["teacher"].copy()), torch.from_numpy(a["gt"].copy()), alpha=a["alpha"],
                  mask=m, background_factor=a["background_factor"])
        loss.backward()
        ref = p.grad.numpy()
        v64, mag = GR.grad(**a)
        key = GR.grad_key(shape, mode, mask_mode, kind, pi)
        u = ref_units(ref, v64, mag, key)
        out[key + "/ref_units"] = np.array([u], np.float64)
        worst = max(worst, (u, key))
        if shape == GR.STORED_SHAPE and pi in GR.STORED_PARAMS:
            out[key + "/ref"] = ref.astype(np.float32)
    # the plain classes on the first shape: MaskedMseLoss and MaskedBceWithLogits return the gt term, DistillationLoss the mix
    pred, teacher, gt, mask = R.loss_inputs(R.LOSS_SHAPES[0], "neither", "nj")
    for name, (fn, with_teacher, with_mask, kw) in plain_calls(opt).items():
        p = torch.from_numpy(pred.copy()).requires_grad_()
        tm = torch.from_numpy(mask.copy()) if with_mask else None
        tg = torch.from_numpy(gt.copy())
        loss = fn(p, torch.from_numpy(teacher.copy()), tg, kw["alpha"], tm) if with_teacher else fn(p, tg, tm)
        loss.backward()
        ref = p.grad.numpy()
        v64, mag = GR.grad(pred, teacher if with_teacher else None, gt, kw["alpha"], mask if with_mask else None, 1.0,
                           kw["kind"], 1.0, kw["pw_g"], unit=False, grad_loss=(0, 0, 1) if with_teacher else (0, 1, 0))
        u = ref_units(ref, v64, mag, name)
        out["plain/%s/ref_units" % name] = np.array([u], np.float64)
        out["plain/%s/ref" % name] = ref.astype(np.float32)
        worst = max(worst, (u, "plain/" + name))
    G.write_npz(OUT, out)
    print("distill_grad.npz: %d entries, %d bytes; %d cases; the reference's float32 gradient against the float64 "
          "restatement: at most %.3g units of 2^-24 * mag (%s)"
          % (len(out), os.path.getsize(OUT), len(GR.all_cases()), worst[0], worst[1]))


if __name__ == "__main__":
    main()
