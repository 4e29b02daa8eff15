#!/usr/bin/env python3
"""Generate tests/golden/student_sizes.npz: the REFERENCE's two students on the CPU at input sizes that are not
multiples of 32 (the sizes its minival feeds them: native COCO images, batch 1).

Build-container only, like tools/gen_golden.py: imports the reference from its read-only tree (never copied; nothing at
test time reads it).  Same seeded state dicts as student.npz / student_steps.npz (``synth.make_state_dict(shapes, 3 | 4,
"W1")``), same image generator; the bundled attention weights (assets/pretrained_segm_4MB) validate the oracle
restatement at one ragged size too, as they do in student.npz.  Only arrays are written:

  s100_33x47_{att,det}     AttentionStudent(inplanes=100), x = make_images(2, 33, 47, seed=101)
  s100_100x140_{att,det}   ... make_images(1, 100, 140, seed=102)
  s100_427x640_{att,det}_s4, ..._{sum,abs}   ... make_images(1, 427, 640, seed=103): every 4th row and column + checksums
  steps_33x47_{att,det}    AttentionStudentSteps(inplanes=48), x = make_images(1, 33, 47, seed=111), alt = LAB of
                           torch.rand(seed 112), no att_divisor
  steps_100x140_{att,det}  ... make_images(1, 100, 140, seed=113), alt of seed 114, att_divisor = 20
  oracle_vs_reference_maxdiff   (case, att | det): oracle/student_ref.py against the reference on the same inputs
  bundled_oracle_vs_reference_maxdiff   the same with the bundled attention weights at 100 x 140

    python tools/gen_golden_student_sizes.py
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

from oracle import student_ref, synth  # noqa: E402

S100_CASES = (("33x47", 2, 33, 47, 101), ("100x140", 1, 100, 140, 102), ("427x640", 1, 427, 640, 103))
STEPS_CASES = (("33x47", 1, 33, 47, 111, 112, None), ("100x140", 1, 100, 140, 113, 114, 20.0))


def steps_alt(n, h, w, seed):
    """the alt image of a case: a seeded RGB image in LAB (as tools/gen_golden.py gen_student_steps)"""
    rgb = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))
    lab = student_ref.rgb2lab(rgb.permute(0, 2, 3, 1).numpy()).astype(np.float32)
    return torch.from_numpy(lab).permute(0, 3, 1, 2).contiguous()


def main():
    torch.set_num_threads(8)
    sys.path.insert(0, REF)
    from rtpe.students import AttentionStudent, AttentionStudentSteps
    out, diffs = {}, []

    shapes = json.load(open(os.path.join(OUT, "student_shapes.json")))["shapes"]
    sd = synth.make_state_dict({k: tuple(v) for k, v in shapes.items()}, 3, "W1")
    stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False).eval()
    stu.load_state_dict(sd, strict=True)
    for name, n, h, w, seed in S100_CASES:
        x = synth.make_images(n, h, w, seed=seed)
        with torch.no_grad():
            att, det = stu(x)
        assert att.shape == (n, 1, -(-h // 4), -(-w // 4)) and det.shape == (n, 18, -(-h // 4), -(-w // 4))
        assert torch.isfinite(att).all() and torch.isfinite(det).all()
        oa, od = student_ref.student_forward(sd, x, half_stem=True)
        diffs.append([float((oa - att).abs().max()), float((od - det).abs().max())])
        print("student100 %s: att %s det %s |det| max %.3f; oracle vs reference %s" % (name, tuple(att.shape), tuple(det.shape),
                                                                                    float(det.abs().max()), diffs[-1]))
        if h * w > 100000:          # a strided sample + checksums, in the style of hrnet_640.npz
            for key, t in (("att", att), ("det", det)):
                out["s100_%s_%s_s4" % (name, key)] = t.numpy()[:, :, ::4, ::4]
                out["s100_%s_%s_sum" % (name, key)] = np.float64(t.double().sum())
                out["s100_%s_%s_abs" % (name, key)] = np.float64(t.double().abs().sum())
        else:
            out["s100_%s_att" % name], out["s100_%s_det" % name] = att.numpy(), det.numpy()
    # the bundled trained attention weights
    pre = glob.glob(os.path.join(REF, "assets", "pretrained_segm_4MB", "*mid_stem.statedict"))[0][:-len("mid_stem.statedict")]
    stu.load_state_dicts(pre)
    x = synth.make_images(1, 100, 140, seed=102)
    with torch.no_grad():
        att_b, det_b = stu(x)
    ob_a, ob_d = student_ref.student_forward(stu.state_dict(), x, half_stem=True)
    d_b = [float((ob_a - att_b).abs().max()), float((ob_d - det_b).abs().max())]
    print("student100 bundled weights 100x140: oracle vs reference", d_b)

    shapes = json.load(open(os.path.join(OUT, "student_steps_shapes.json")))["shapes"]
    sd = synth.make_state_dict({k: tuple(v) for k, v in shapes.items()}, 4, "W1")
    stu = AttentionStudentSteps(None, "cpu", 48, 17, 1, True, None, False).eval()
    stu.load_state_dict(sd, strict=True)
    for name, n, h, w, seed, alt_seed, div in STEPS_CASES:
        x, alt = synth.make_images(n, h, w, seed=seed), steps_alt(n, h, w, alt_seed)
        with torch.no_grad():
            att, det = stu(x, alt=alt) if div is None else stu(x, alt=alt, att_divisor=div)
        assert att.shape == (n, 1, -(-h // 4), -(-w // 4)) and det.shape == (n, 18, -(-h // 4), -(-w // 4))
        assert torch.isfinite(att).all() and torch.isfinite(det).all()
        oa, od = student_ref.student_steps_forward(sd, x, alt, div, half_stem=True)
        diffs.append([float((oa - att).abs().max()), float((od - det).abs().max())])
        print("steps48 %s: att %s det %s |det| max %.3f; oracle vs reference %s" % (name, tuple(att.shape), tuple(det.shape),
                                                                                 float(det.abs().max()), diffs[-1]))
        out["steps_%s_att" % name], out["steps_%s_det" % name] = att.numpy(), det.numpy()
    out["oracle_vs_reference_maxdiff"] = np.array(diffs)
    out["bundled_oracle_vs_reference_maxdiff"] = np.array(d_b)
    path = os.path.join(OUT, "student_sizes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
