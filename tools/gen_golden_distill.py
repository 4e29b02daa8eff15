#!/usr/bin/env python
"""Writes tests/golden/distill.npz: what the reference computes for the distillation targets and losses on the test data
of tests/distill_restated.py.

Build-container only: imports the reference checkout (read-only, never copied; REF below or argv[1]) and runs its own
``HWHeatmapGenerator`` (rtpe/dataloaders.py), its loss classes (rtpe/optimization.py) and the ``F.interpolate`` calls of
its dataset and training step on PyTorch-CPU.  The packages the reference imports and this data path never touches
(torchvision, skimage, pycocotools, cv2, json_tricks) are stubbed in ``sys.modules``.

Bulky arrays go in as sha-256 digests (``distill_restated.digest``); a digest that agrees is ``array_equal``.  Per loss
case the fixture holds the reference's float32 scalar and its distance from the float64 restatement - the reference's
own rounding, which is the only margin the device test adds to the derived bound.  Same inputs, same bytes.

    python tools/gen_golden_distill.py [/path/to/reference]
"""
import io
import os
import sys
import types
import zipfile
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "distill.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distill_restated as R  # noqa: E402


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return mock.MagicMock(name=self.__name__ + "." + name)


def import_reference():
    for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.datasets",
                 "skimage", "skimage.color", "skimage.transform", "pycocotools", "pycocotools.coco", "pycocotools.cocoeval",
                 "pycocotools.mask", "cv2", "json_tricks"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = _Stub(name)
    sys.path.insert(0, REF)
    from rtpe import dataloaders, optimization
    return dataloaders, optimization


def write_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same results give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def interp(x, hw, align_corners):
    return F.interpolate(torch.from_numpy(np.ascontiguousarray(x)), tuple(hw), mode="bilinear",
                         align_corners=align_corners).numpy()


def main():
    dl, opt = import_reference()
    out = {}
    # ground-truth maps: the reference's generator, image by image
    for J, hw in R.GT_SHAPES:
        scene = R.gt_scene(J, hw)
        for sigma in R.GT_SIGMAS:
            gen = dl.HWHeatmapGenerator(J, sigma)
            maps = np.stack([gen(p, hw) for p in scene])
            key = "gt/%d/%dx%d/%g" % (J, hw[0], hw[1], sigma)
            out[key] = R.digest(maps)
            if maps.size <= 4096:
                out[key + "/raw"] = maps
            out[key + "/peak"] = np.array([maps.max()], np.float32)
    # targets: dataset (teacher to the image, align_corners=True, per image) and training step (everything to the grids)
    for i, case in enumerate(R.TARGET_CASES):
        image_hw, det_hw, att_hw, _ = case
        people, teacher, mask, segm = R.target_inputs(case)
        gen = dl.HWHeatmapGenerator(R.TARGET_J, 2.0)
        hms = np.stack([gen(p, image_hw) for p in people])
        t_img = np.stack([interp(t[None], image_hw, True)[0] for t in teacher])
        res = dict(gt=interp(hms, det_hw, False), teacher=interp(t_img, det_hw, False),
                   mask=interp(mask[:, None], det_hw, False), segm=interp(segm[:, None], att_hw, False))
        for k, v in res.items():
            out["targets/%d/%s" % (i, k)] = R.digest(v)
        out["targets/%d/minmax" % i] = np.array([res["gt"].min(), res["gt"].max(), res["teacher"].min(),
                                                 res["teacher"].max()], np.float32)
    # normalisation and losses: the reference's classes on PyTorch-CPU
    n_loss = 0
    for shape in R.LOSS_SHAPES:
        for mode in R.LOSS_MODES:
            for mask_mode in R.LOSS_MASKS:
                pred, teacher, gt, mask = R.loss_inputs(shape, mode, mask_mode)
                J = shape[1]
                tp, tt, tg = torch.from_numpy(pred[:, :J].copy()), torch.from_numpy(teacher), torch.from_numpy(gt)
                for kind in R.LOSS_KINDS:
                    for pi, (bf, alpha, pw) in enumerate(R.LOSS_PARAMS):
                        pw_t, pw_g = R.loss_pos_weights(pw)
                        fn = opt.DistillationBceLossKeypointMining(pw_t, pw_g) if kind == "bce" else \
                            opt.DistillationLossKeypointMining()
                        m = None if mask is None else torch.from_numpy(mask).expand(shape).clone()
                        with torch.no_grad():
                            ref = np.float32(fn(tp.clone(), tt.clone(), tg.clone(), alpha=alpha, mask=m,
                                                background_factor=bf).item())
                        r64 = R.distillation_loss(pred, teacher, gt, alpha, mask, bf, kind, pw_t, pw_g)[2]
                        key = R.loss_key(shape, mode, mask_mode, kind, pi)
                        out[key + "/ref32"] = np.array([ref], np.float32)
                        out[key + "/ref_dist"] = np.array([abs(float(ref) - r64)], np.float64)
                        n_loss += 1
                        if kind == "bce":           # the reference's mask after the call is the effective mask
                            gn, tn, me = R.normalise(gt, teacher, mask, bf)
                            if m is not None:
                                assert np.array_equal(m.numpy(), me), key
                                out[key + "/mask"] = R.digest(m.numpy())
                # the normalised targets as the reference's arithmetic in torch gives them
                g2, t2 = tg.clone(), tt.clone()
                if g2.min() < 0:
                    g2 = g2 - g2.min()
                if g2.max() > 1:
                    g2 = g2 / g2.max()
                if t2.min() < 0:
                    t2 = t2 - t2.min()
                if t2.max() > 1:
                    t2 = t2 / t2.max()
                out[R.loss_key(shape, mode, mask_mode) + "/gt"] = R.digest(g2.numpy())
                out[R.loss_key(shape, mode, mask_mode) + "/teacher"] = R.digest(t2.numpy())
    # the three plain classes on the first shape
    shape = R.LOSS_SHAPES[0]
    pred, teacher, gt, mask = R.loss_inputs(shape, "neither", "nj")
    tp, tt, tg, tm = (torch.from_numpy(a) for a in (pred, teacher, gt, mask))
    with torch.no_grad():
        plain = {"mse": opt.MaskedMseLoss()(tp, tg, tm), "mse_nomask": opt.MaskedMseLoss()(tp, tg),
                 "bce7": opt.MaskedBceWithLogits(7)(tp, tg, tm), "bce7_nomask": opt.MaskedBceWithLogits(7)(tp, tg),
                 "distill": opt.DistillationLoss()(tp, tt, tg, 0.25, tm)}
    want = {"mse": R.distillation_loss(pred, None, gt, 0.0, mask, 1.0, "mse")[1],
            "mse_nomask": R.distillation_loss(pred, None, gt, 0.0, None, 1.0, "mse")[1],
            "bce7": R.distillation_loss(pred, None, gt, 0.0, mask, 1.0, "bce", 1.0, 7.0, unit=False)[1],
            "bce7_nomask": R.distillation_loss(pred, None, gt, 0.0, None, 1.0, "bce", 1.0, 7.0, unit=False)[1],
            "distill": R.distillation_loss(pred, teacher, gt, 0.25, mask, 1.0, "mse")[2]}
    for k, v in plain.items():
        ref = np.float32(v.item())
        out["plain/%s/ref32" % k] = np.array([ref], np.float32)
        out["plain/%s/ref_dist" % k] = np.array([abs(float(ref) - want[k])], np.float64)
    write_npz(OUT, out)
    rel = [float(out[k][0]) / max(abs(float(out[k[:-8] + "ref32"][0])), 1e-300) for k in out if k.endswith("/ref_dist")]
    print("distill.npz: %d entries, %d bytes; %d loss cases, reference vs float64 restatement: relative distance max %.3g"
          % (len(out), os.path.getsize(OUT), n_loss, max(rel)))


if __name__ == "__main__":
    main()
