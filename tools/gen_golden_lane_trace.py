#!/usr/bin/env python3
"""Generate tests/golden/lane_trace_teacher_64.json: what one forward of the W48 teacher (fp16 program, seeded W0
weights, 1 x 3 x 64 x 64, option "lanes" = 1, every other option at its default, default launch shapes) enqueued - the
trace of include/rtpe_hip_trace.h - together with the op and tensor descs of the program.

Needs an MI355X and the built library.  The file is the realistic input of the seeded faults of
tests/test_schedule_host.py and nothing else: routes are allowed to change, so no test compares a live trace with it.

    python tools/gen_golden_lane_trace.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
for p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd")):
    sys.path.insert(0, p)
os.environ["RTPE_AUTOTUNE"] = "0"       # the default launch shapes: the same trace on every run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lane_trace_teacher_64.json"))
    args = ap.parse_args()
    import torch
    from oracle import schedule, synth
    from rtpe import _native as nat
    from rtpe.helpers import build_hrnet_w48_teacher
    from rtpe.third_party import pose_higher_hrnet as phh
    with open(os.path.join(ROOT, "tests", "golden", "w48_shapes.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
    sd = synth.make_state_dict(shapes, 0, "W0")
    dev = torch.device("cuda:0")
    model = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(dev)
    eng = model[1]._engine(dev)
    nat.check(nat.lib().rtpe_set_option(b"lanes", 1))
    x = synth.make_images(1, 64, 64, seed=7).half().to(dev)
    prev = phh.set_forward_flags(phh.FWD_TRACE)
    try:
        eng.forward(x)
    finally:
        phh.set_forward_flags(prev)
    torch.cuda.synchronize()
    ops, tensors = schedule.descs(eng.program)
    trace = eng.read_trace()
    findings = schedule.check(ops, tensors, trace)
    counts = schedule.structure(ops, tensors, trace)
    print("ops %d tensors %d records %d findings %d" % (len(ops), len(tensors), len(trace), len(findings)))
    print("structure:", json.dumps(counts, sort_keys=True))
    for f in findings:
        print("finding:", f["text"])
    with open(args.out, "w") as f:
        json.dump({"what": "W48 teacher, fp16, 1x3x64x64, lanes=1, default options and launch shapes", "shape": [1, 64, 64],
                   "ops": ops, "tensors": tensors, "trace": trace}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
