#!/usr/bin/env python3
"""Generate tests/golden/student_half.npz: the REFERENCE's AttentionStudent with a half-precision BODY on the CPU.

Build-container only, like tools/gen_golden_student_sizes.py: imports the reference from its read-only tree (never copied;
nothing at test time reads it).  The half model is the reference module prepared as DESIGN.md section 4 ("half body")
states it:

    stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False)      # half-wrapped stem, fp32 body
    stu = BN_convert_float(stu.half())                                      # every parameter fp16, every BatchNorm fp32
    stu.stem[2] = torch.nn.Identity()                                       # no tofp32 between stem and body (exact)
    stu.load_state_dict(fp32_checkpoint)                                    # BatchNorm keeps the checkpoint's fp32 values

and the outputs are ``(att.float(), det.float())``.  Cases: the seeded W1 weights of student_shapes.json at 2 x 33 x 47
(make_images seed 101) and 2 x 64 x 96 (seed 104), the bundled attention weights (assets/pretrained_segm_4MB) at
1 x 100 x 140 (seed 102).  Per case and per map (att, det) only arrays are written:

  <case>_<map>_half      the half outputs, float16 (every value is one)
  <case>_<map>_alt       the same model and input with oneDNN disabled (PyTorch-CPU's other kernels), float16
  <case>_<map>_f32       the fp32-body reference (half stem, as student_sizes.npz), float32
  <case>_<map>_spread    (max, mean) of |half - alt|: the reference's distance from itself

and tests/golden/student_half_bundled_{a,b,c}.npz: the bundled mid_stem and att_* parameters as the half model stores them
(the seeded W1 weights stay in det_*), by their state-dict keys.

    python tools/gen_golden_student_half.py
"""
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle import synth  # noqa: E402

CASES = (("w1_33x47", "W1", 2, 33, 47, 101), ("w1_64x96", "W1", 2, 64, 96, 104), ("bundled_100x140", "bundled", 1, 100, 140, 102))


def main():
    torch.set_num_threads(8)
    sys.path.insert(0, REF)
    from rtpe.students import AttentionStudent
    from rtpe.third_party.fp16_utils.fp16util import BN_convert_float
    shapes = json.load(open(os.path.join(OUT, "student_shapes.json")))["shapes"]
    sd = synth.make_state_dict({k: tuple(v) for k, v in shapes.items()}, 3, "W1")
    pre = glob.glob(os.path.join(REF, "assets", "pretrained_segm_4MB", "*mid_stem.statedict"))[0][:-len("mid_stem.statedict")]
    out = {}
    for name, weights, n, h, w, seed in CASES:
        f32 = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False).eval()
        f32.load_state_dict(sd, strict=True)
        if weights == "bundled":
            f32.load_state_dicts(pre)
        # the weights are loaded AFTER the conversion, as a user of ``AttentionStudent(body_half=True).load_state_dict`` loads
        # them: every BatchNorm then holds the checkpoint's fp32 values.  (Converting a loaded model would send the BatchNorm
        # parameters and statistics through fp16 on the way - ``.half()`` rounds them before ``BN_convert_float`` widens them
        # again - which moves det by 1.1e-4 on average, twice the reference's distance from itself.)
        half = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False).eval()
        half = BN_convert_float(half.half())
        half.stem[2] = torch.nn.Identity()
        half.load_state_dict(f32.state_dict(), strict=True)
        assert all(torch.equal(v, f32.state_dict()[k]) for k, v in half.state_dict().items() if v.dtype == torch.float32)
        x = synth.make_images(n, h, w, seed=seed)
        with torch.no_grad():
            ra, rd = f32(x)
            ha, hd = half(x)
            with torch.backends.mkldnn.flags(enabled=False):
                aa, ad = half(x)
        for key, r, a, b in (("att", ra, ha, aa), ("det", rd, hd, ad)):
            c = 1 if key == "att" else 18
            assert a.dtype == torch.float16 and b.dtype == torch.float16 and r.dtype == torch.float32
            assert a.shape == b.shape == r.shape == (n, c, -(-h // 4), -(-w // 4)), (a.shape, r.shape)
            assert torch.isfinite(a).all() and torch.isfinite(b).all() and torch.isfinite(r).all()
            d = (a.float() - b.float()).abs()
            e = (a.float() - r).abs()
            out["%s_%s_half" % (name, key)] = a.numpy()
            out["%s_%s_alt" % (name, key)] = b.numpy()
            out["%s_%s_f32" % (name, key)] = r.numpy()
            out["%s_%s_spread" % (name, key)] = np.array([float(d.max()), float(d.mean())], np.float64)
            print("%s %s %s: range +-%.3f; half vs itself (oneDNN off) max %.3e mean %.3e; half vs fp32 body max %.3e mean %.3e"
                  % (name, key, tuple(a.shape), float(r.abs().max()), float(d.max()), float(d.mean()), float(e.max()), float(e.mean())))
    path = os.path.join(OUT, "student_half.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    # the bundled attention weights as the half model holds them (fp16 parameters, fp32 BatchNorm), so that the case can run
    # where the reference's assets are not: three files, each below the size limit of a committed file
    bundled = {k: v for k, v in half.state_dict().items() if k.split(".")[0] in ("mid_stem", "att_lo", "att_mid", "att_hi", "att_top")
               and not k.endswith("num_batches_tracked")}
    assert all(v.dtype == (torch.float32 if v.dim() == 1 and "fc" not in k and "att_top" not in k else torch.float16)
               for k, v in bundled.items())
    parts = {"a": lambda k: k == "mid_stem.0.weight",
             "b": lambda k: k != "mid_stem.0.weight" and k.split(".")[0] in ("mid_stem", "att_top", "att_hi"),
             "c": lambda k: k.split(".")[0] in ("att_mid", "att_lo")}
    n = 0
    for part, pick in parts.items():
        path = os.path.join(OUT, "student_half_bundled_%s.npz" % part)
        sel = {k: v.numpy() for k, v in bundled.items() if pick(k)}
        n += len(sel)
        np.savez_compressed(path, **sel)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20
    assert n == len(bundled)


if __name__ == "__main__":
    main()
