"""Throughput of the dual-head student (bench.py's config 4: AttentionStudent(inplanes=100), seeded W1 weights, batch
32, 320 x 320) through its three decode paths, on one GPU and in one process:

  (a) sync_expand     the synchronous step exactly as ``bench.py --config 4`` runs it: forward, the heat maps copied,
                      the tag map copied to 17 planes, ``parse_lowres``;
  (b) sync_shared     the same step with ``parse_lowres_shared`` on the channel slices of ``det`` (no copies);
  (c) stream_host /   ``StudentPipeline.stream`` (two forwards in flight, decode on the side stream) with the
      stream_device   candidates grouped on the host / on the device.

Everything is warmed up first, then timed in the order A B B A (--repeats runs of --steps steps each, every run ends
in a device synchronise); per path the median, every run and the spread (max - min) of the runs are reported.  Also,
for (a) and (b), the GPU time of the decode of one batch alone, every phase by itself: [the copies +] top-k, and adjust +
refine (device events; the host matching between them is not counted).  Prints one JSON line and writes it to --out.
Needs a GPU; there is no fallback.

    python tools/student_bench.py [--steps 12] [--warmup 3] [--repeats 4] [--decode-reps 5]

``--body-half`` measures something else: the student with a half-precision body (``AttentionStudent(body_half=True)``)
against the fp32 body, same weights, same input, one process - the forward alone and the synchronous step (a) - both
warmed up (autotuned), order A B B A; written to profiles/student_half_bench.json.

    python tools/student_bench.py --body-half [--steps 12] [--warmup 3] [--repeats 4]

``--steps-half`` is the same protocol for the Steps student: ``AttentionStudentSteps`` (fp32 body) against
``AttentionStudentStepsHalf``, inplanes 48 and 80, seeded W1 weights, ``alt`` a seeded image of a LAB image's span,
``att_divisor`` 20; one JSON line per inplanes, written to profiles/steps_half_bench.json.

    python tools/student_bench.py --steps-half [--steps 12] [--warmup 3] [--repeats 4]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=4, help="timed runs per path, interleaved A B B A ...")
    ap.add_argument("--decode-reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--body-half", action="store_true", help="the half body against the fp32 body (see the module docstring)")
    ap.add_argument("--steps-half", action="store_true", help="AttentionStudentStepsHalf against AttentionStudentSteps (see the module docstring)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "steps_half_bench.json" if args.steps_half else
                                "student_half_bench.json" if args.body_half else "student_pipeline_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("student_bench: no GPU (the students run on the HIP path only)")
    import __graft_entry__ as entry
    entry.build()
    if args.steps_half:
        return steps_half_bench(args)
    from oracle import synth
    from rtpe import _native as nat
    from rtpe import engine
    from rtpe.students import AttentionStudent
    from rtpe.third_party.group import HeatmapParser
    torch.set_num_threads(nat.host_threads(8))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "tests", "golden", "student_shapes.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
    stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False).eval()
    stu.load_state_dict(synth.make_state_dict(shapes, 3, "W1"), strict=True)
    stu = stu.to(dev)
    B, S, J = args.batch, args.size, engine.NUM_HEATMAPS
    x = torch.randn(B, 3, S, S, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))

    def new_parser(match_on="host"):
        return HeatmapParser(num_joints=J, match_on=match_on, **engine.HM_PARSER_PARAMS)

    def count(res):
        return sum(len(p) if getattr(p, "ndim", 0) == 3 else 0 for p, _ in res)

    def expand_args(det):
        return det[:, :J].contiguous(), det[:, J:J + 1].expand(-1, J, -1, -1).contiguous()

    def sync_rate(decode):
        def run(steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.no_grad():
                for _ in range(steps):
                    att, det = stu(x)
                    res = decode(det.float())
            torch.cuda.synchronize(dev)
            return B * steps / (time.perf_counter() - t0), count(res)
        return run

    def stream_rate(match_on):
        pipe = engine.StudentPipeline(stu, new_parser(), dev, match_on=match_on)

        def run(steps):
            res = []
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for res in pipe.stream((x for _ in range(steps)), (S, S)):
                pass
            torch.cuda.synchronize(dev)
            return B * steps / (time.perf_counter() - t0), count(res)
        return run

    if args.body_half:
        return body_half_bench(args, stu, x, shapes, new_parser, expand_args, count)

    p_a, p_b = new_parser(), new_parser()
    paths = {"sync_expand": sync_rate(lambda det: p_a.parse_lowres(*expand_args(det), (S, S))),
             "sync_shared": sync_rate(lambda det: p_b.parse_lowres_shared(det[:, :J], det[:, J:], (S, S))),
             "stream_host": stream_rate("host"),
             "stream_device": stream_rate("device")}
    for run in paths.values():
        run(args.warmup)
    runs = {key: [] for key in paths}
    people = {}
    order = list(paths)
    for r in range(args.repeats):
        for key in (order if r % 2 == 0 else order[::-1]):
            v, people[key] = paths[key](args.steps)
            runs[key].append(round(v, 1))

    # the decode of one batch alone, phase by phase
    L = nat.lib()
    spans = []

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a)
        e1.record()
        return out, (e0, e1)

    class Timed:                        # the library with device events around the adjust / refine entries
        def __getattr__(self, name):
            fn = getattr(L, name)
            if not name.startswith("rtpe_adjust_refine_fused"):
                return fn

            def call(*a):
                rc, ev = timed(fn, *a)
                spans.append(ev)
                return rc
            return call

    def decode_times(parser, phase1):
        topk_ms, refine_ms = [], []
        with torch.no_grad():
            att, det = stu(x)
            det = det.float()
            for r in range(args.decode_reps + 1):
                torch.cuda.synchronize(dev)
                st, tk = timed(phase1, parser, det)
                real, nat._lib = nat._lib, Timed()
                spans.clear()
                try:
                    parser.lowres_match(st)
                    parser.lowres_finish(st)
                finally:
                    nat._lib = real
                torch.cuda.synchronize(dev)
                if r:
                    topk_ms.append(tk[0].elapsed_time(tk[1]))
                    refine_ms.append(sum(a.elapsed_time(b) for a, b in spans))
        med = lambda v: round(float(np.median(v)), 3)      # noqa: E731
        return {"copies_topk": med(topk_ms), "adjust_refine": med(refine_ms),
                "total": med(np.array(topk_ms) + np.array(refine_ms))}

    decode = {"sync_expand": decode_times(p_a, lambda p, det: p.lowres_topk(*expand_args(det), (S, S))),
              "sync_shared": decode_times(p_b, lambda p, det: p.lowres_topk_shared(det[:, :J], det[:, J:], (S, S)))}

    out = {"metric": "student_pipeline_throughput", "model": "AttentionStudent(inplanes=100)", "weights": "W1", "batch": B,
           "size": S, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(dev), "order": "A B B A over " + ", ".join(order)}
    for key in order:
        out[key] = {"img_s": round(float(np.median(runs[key])), 1), "img_s_runs": runs[key],
                    "img_s_spread": round(max(runs[key]) - min(runs[key]), 1),
                    "ms_per_step": round(1e3 * B / float(np.median(runs[key])), 3)}
        if key in decode:
            out[key]["decode_gpu_ms_per_batch"] = decode[key]
    base = out["sync_expand"]["img_s"]
    for key in order[1:]:
        out[key]["over_sync_expand"] = round(out[key]["img_s"] / base, 4)
    out["people_last_batch"] = people
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def body_half_bench(args, stu32, x, shapes, new_parser, expand_args, count):
    """fp32 body against half body: forward alone and forward + ``parse_lowres`` on the expanded maps (bench.py's config-4
    step), A B B A"""
    from oracle import synth
    from rtpe.students import AttentionStudent
    dev, B, S = x.device, args.batch, args.size
    stu16 = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False, body_half=True).eval()
    stu16.load_state_dict(synth.make_state_dict(shapes, 3, "W1"), strict=True)
    stu16 = stu16.to(dev)
    models = {"fp32_body": stu32, "half_body": stu16}
    parsers = {k: new_parser() for k in models}

    def forward(key):
        def run(steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.no_grad():
                for _ in range(steps):
                    models[key](x)
            torch.cuda.synchronize(dev)
            return B * steps / (time.perf_counter() - t0), 0
        return run

    def step(key):
        def run(steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.no_grad():
                for _ in range(steps):
                    att, det = models[key](x)
                    res = parsers[key].parse_lowres(*expand_args(det.float()), (S, S))
            torch.cuda.synchronize(dev)
            return B * steps / (time.perf_counter() - t0), count(res)
        return run

    paths = {"forward_fp32_body": forward("fp32_body"), "forward_half_body": forward("half_body"),
             "step_fp32_body": step("fp32_body"), "step_half_body": step("half_body")}
    with torch.no_grad():
        a32, d32 = stu32(x)
        a16, d16 = stu16(x)
    diff = {"att_max": float((a32 - a16).abs().max()), "det_max": float((d32 - d16).abs().max()),
            "det_mean": float((d32 - d16).abs().mean()), "det_range": float(d32.abs().max())}
    for run in paths.values():
        run(args.warmup)
    runs = {key: [] for key in paths}
    order = list(paths)
    for r in range(args.repeats):
        for key in (order if r % 2 == 0 else order[::-1]):
            runs[key].append(round(paths[key](args.steps)[0], 1))
    out = {"metric": "student_half_body_throughput", "model": "AttentionStudent(inplanes=100)", "weights": "W1", "batch": B,
           "size": S, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(dev), "order": "A B B A over " + ", ".join(order),
           "half_vs_fp32_outputs": diff}
    for key in order:
        out[key] = {"img_s": round(float(np.median(runs[key])), 1), "img_s_runs": runs[key],
                    "img_s_spread": round(max(runs[key]) - min(runs[key]), 1),
                    "ms_per_step": round(1e3 * B / float(np.median(runs[key])), 3)}
    out["forward_half_over_fp32"] = round(out["forward_half_body"]["img_s"] / out["forward_fp32_body"]["img_s"], 4)
    out["step_half_over_fp32"] = round(out["step_half_body"]["img_s"] / out["step_fp32_body"]["img_s"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def steps_half_bench(args):
    """``AttentionStudentSteps`` against ``AttentionStudentStepsHalf``: forward alone and forward + ``parse_lowres`` on the
    expanded maps, both models warmed up (autotuned through the aux entry), A B B A; one line per inplanes"""
    from oracle import synth
    from rtpe import _native as nat
    from rtpe import engine
    from rtpe.students import AttentionStudentSteps, AttentionStudentStepsHalf
    from rtpe.third_party.group import HeatmapParser
    torch.set_num_threads(nat.host_threads(8))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, S, J, div = args.batch, args.size, engine.NUM_HEATMAPS, 20.0
    x = torch.randn(B, 3, S, S, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    alt = torch.rand(B, 3, S, S, device=dev, generator=torch.Generator(device=dev).manual_seed(1235)) * 130.0 - 30.0
    lines = []
    for P, shapes_file in ((48, "student_steps_shapes.json"), (80, "student_steps80_shapes.json")):
        with open(os.path.join(ROOT, "tests", "golden", shapes_file)) as f:
            shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
        sd = synth.make_state_dict(shapes, 4, "W1")
        models = {}
        for key, cls in (("fp32_body", AttentionStudentSteps), ("half_body", AttentionStudentStepsHalf)):
            m = cls(None, "cpu", P, 17, 1, True, None, False).eval()
            m.load_state_dict(sd, strict=True)
            models[key] = m.to(dev)
        parsers = {k: HeatmapParser(num_joints=J, **engine.HM_PARSER_PARAMS) for k in models}

        def forward(key):
            def run(steps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                with torch.no_grad():
                    for _ in range(steps):
                        models[key](x, alt=alt, att_divisor=div)
                torch.cuda.synchronize(dev)
                return B * steps / (time.perf_counter() - t0)
            return run

        def step(key):
            def run(steps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                with torch.no_grad():
                    for _ in range(steps):
                        att, det = models[key](x, alt=alt, att_divisor=div)
                        det = det.float()
                        parsers[key].parse_lowres(det[:, :J].contiguous(), det[:, J:J + 1].expand(-1, J, -1, -1).contiguous(), (S, S))
                torch.cuda.synchronize(dev)
                return B * steps / (time.perf_counter() - t0)
            return run

        paths = {"forward_fp32_body": forward("fp32_body"), "forward_half_body": forward("half_body"),
                 "step_fp32_body": step("fp32_body"), "step_half_body": step("half_body")}
        with torch.no_grad():
            a32, d32 = models["fp32_body"](x, alt=alt, att_divisor=div)
            a16, d16 = models["half_body"](x, alt=alt, att_divisor=div)
        diff = {"att_max": float((a32 - a16).abs().max()), "det_max": float((d32 - d16).abs().max()),
                "det_mean": float((d32 - d16).abs().mean()), "det_range": float(d32.abs().max())}
        for run in paths.values():
            run(args.warmup)
        runs = {key: [] for key in paths}
        order = list(paths)
        for r in range(args.repeats):
            for key in (order if r % 2 == 0 else order[::-1]):
                runs[key].append(round(paths[key](args.steps), 1))
        out = {"metric": "steps_half_body_throughput", "model": "AttentionStudentSteps(inplanes=%d)" % P, "weights": "W1",
               "att_divisor": div, "batch": B, "size": S, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
               "device": torch.cuda.get_device_name(dev), "order": "A B B A over " + ", ".join(order),
               "half_vs_fp32_outputs": diff}
        for key in order:
            out[key] = {"img_s": round(float(np.median(runs[key])), 1), "img_s_runs": runs[key],
                        "img_s_spread": round(max(runs[key]) - min(runs[key]), 1),
                        "ms_per_step": round(1e3 * B / float(np.median(runs[key])), 3)}
        out["forward_half_over_fp32"] = round(out["forward_half_body"]["img_s"] / out["forward_fp32_body"]["img_s"], 4)
        out["step_half_over_fp32"] = round(out["step_half_body"]["img_s"] / out["step_fp32_body"]["img_s"], 4)
        lines.append(json.dumps(out))
        print(lines[-1])
        del models
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
