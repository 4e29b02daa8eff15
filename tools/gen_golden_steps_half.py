#!/usr/bin/env python3
"""Generate tests/golden/steps_half.npz: the REFERENCE's AttentionStudentSteps with a half-precision BODY on the CPU, and
tests/golden/steps_program_default.json: the op list the fp32 AttentionStudentSteps of THIS tree compiles to.

Build-container only, like tools/gen_golden_student_half.py: imports the reference from its read-only tree (never copied;
nothing at test time reads it).  The half model is the reference module prepared as DESIGN.md section 4 ("Half body: the
Steps student") states it:

    m = AttentionStudentSteps(None, "cpu", P, 17, 1, True, None, False).eval()
    m = BN_convert_float(m.half()); m.stem[2] = torch.nn.Identity()
    m.load_state_dict(fp32_checkpoint)                  # after the conversion: BatchNorm keeps the fp32 values
    att, det = m(x, alt=alt.half(), att_divisor=d)      # -> (att.float(), det.float())

Cases (CASES): seeded W1 weights made from the parameter shapes (never stored), ``alt`` a seeded image in LAB.  Per case and
per map (att, det) only arrays are written:

  <case>_<map>_half      the half outputs, float16 (every value is one)
  <case>_<map>_alt       the same model and inputs with oneDNN disabled, float16
  <case>_<map>_f32       the fp32-body reference (half stem), float32
  <case>_<map>_spread    (max, mean) of |half - alt|: the reference's distance from itself

and tests/golden/student_steps80_shapes.json: the parameter shapes of inplanes = 80.

    python tools/gen_golden_steps_half.py              # the fixture
    python tools/gen_golden_steps_half.py --program    # the op list of the fp32 class (recorded before the half class existed)
"""
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

from oracle import student_ref, synth  # noqa: E402

# name, inplanes, seed of the weights, N, H, W, seed of the images, seed of alt, att_divisor
CASES = (("p48_33x47_nodiv", 48, 4, 2, 33, 47, 121, 122, None), ("p48_33x47_div20", 48, 4, 2, 33, 47, 121, 122, 20.0),
         ("p48_64x96_nodiv", 48, 4, 2, 64, 96, 123, 124, None), ("p48_64x96_div20", 48, 4, 2, 64, 96, 123, 124, 20.0),
         ("p80_64x64_div20", 80, 5, 1, 64, 64, 125, 126, 20.0))


def steps_alt(n, h, w, seed):
    """the alt image of a case: a seeded RGB image in LAB (as tools/gen_golden_student_sizes.py)"""
    rgb = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))
    lab = student_ref.rgb2lab(rgb.permute(0, 2, 3, 1).numpy()).astype(np.float32)
    return torch.from_numpy(lab).permute(0, 3, 1, 2).contiguous()


def program_rows(prog):
    """the field set of tests/test_student_half_host.py program_rows"""
    ch = lambda t: prog.tensors[t].channels if t >= 0 else -1
    return [[int(d.kind), int(d.flags), int(d.cin), int(d.cout), int(d.ksize), int(d.stride), int(d.reserved[1]), int(d.reserved[2]),
             ch(d.in_t), ch(d.out_t), int(d.out_coff), ch(d.res_t)] for d in prog.ops]


def record_program():
    sys.path.insert(0, os.path.join(ROOT, "realtime-pose-estimation_amd"))
    from rtpe.students import AttentionStudentSteps
    out = {}
    for P in (48, 80):
        m = AttentionStudentSteps(None, "cpu", P, 17, 1, True, None, False)
        for div in (None, 20.0):
            p = m.compile_program(("att_divisor", div))
            out["steps%d_%s" % (P, "nodiv" if div is None else "div20")] = {
                "rows": program_rows(p),
                "divisor_bits": [int(d.reserved[0]) for d, n in zip(p.ops, p.names) if n.startswith("gate_mul")],
                "tensors": [[int(t.channels), int(t.ds_log2), int(t.reserved)] for t in p.tensors]}
    path = os.path.join(OUT, "steps_program_default.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    torch.set_num_threads(8)
    sys.path.insert(0, REF)
    from rtpe.students import AttentionStudentSteps
    from rtpe.third_party.fp16_utils.fp16util import BN_convert_float
    out, sds = {}, {}
    for name, P, wseed, n, h, w, seed, alt_seed, div in CASES:
        f32 = AttentionStudentSteps(None, "cpu", P, 17, 1, True, None, False).eval()
        if P not in sds:
            shapes = {k: tuple(v.shape) for k, v in f32.state_dict().items()}
            if P == 48:
                have = json.load(open(os.path.join(OUT, "student_steps_shapes.json")))["shapes"]
                assert {k: tuple(v) for k, v in have.items()} == shapes
            else:
                with open(os.path.join(OUT, "student_steps%d_shapes.json" % P), "w") as f:
                    json.dump({"shapes": {k: list(v) for k, v in shapes.items()}}, f, separators=(",", ":"))
                    f.write("\n")
            sds[P] = synth.make_state_dict(shapes, wseed, "W1")
        f32.load_state_dict(sds[P], strict=True)
        # loaded AFTER the conversion, as a user of the half class loads a checkpoint (see tools/gen_golden_student_half.py)
        half = AttentionStudentSteps(None, "cpu", P, 17, 1, True, None, False).eval()
        half = BN_convert_float(half.half())
        half.stem[2] = torch.nn.Identity()
        half.load_state_dict(f32.state_dict(), strict=True)
        assert all(torch.equal(v, f32.state_dict()[k]) for k, v in half.state_dict().items() if v.dtype == torch.float32)
        x, alt = synth.make_images(n, h, w, seed=seed), steps_alt(n, h, w, alt_seed)
        kw = {} if div is None else {"att_divisor": div}
        with torch.no_grad():
            ra, rd = f32(x, alt=alt, **kw)
            ha, hd = half(x, alt=alt.half(), **kw)
            with torch.backends.mkldnn.flags(enabled=False):
                aa, ad = half(x, alt=alt.half(), **kw)
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
    path = os.path.join(OUT, "steps_half.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    record_program() if "--program" in sys.argv else main()
