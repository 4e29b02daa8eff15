"""The decode with the grouping on the host cores (the default) beside the decode with the grouping kernel
(HeatmapParser(match_on="device"), csrc/match_dev.hip), on one GPU.

In one process: seeded synthetic W0 weights, resident synthetic batches (batch 32, 640 x 640), then for the plain
pipeline and the flip pipeline:
  * img/s of TeacherPipeline.stream with match_on="host" and "device": both warmed up first, then timed in the order
    A B B A ... (--repeats runs each), the median reported beside every run and their spread;
  * the CPU time of the process (all threads) per step, as bench.py computes host_cpu_ms_per_step;
  * host_threads: the matcher threads the process uses (rtpe._native.host_threads follows the cores the process may run
    on: start it under `taskset -c 0,1` for the share a rank gets on a full node).
Prints one JSON line (--out FILE also writes it).  Needs a GPU; there is no fallback.

    python tools/match_bench.py [--steps 20] [--warmup 3] [--repeats 4] [--out profiles/match_device_bench.json]

GPU time per kernel (a run of its own, the timing above is not taken under the profiler):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/host -o t -- python tools/match_bench.py --only host --steps 10
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/device -o t -- python tools/match_bench.py --only device --steps 10
    python tools/match_bench.py --summarize DIR --csv profiles/match_device_kernel_stats.csv

--only MODE runs `--warmup + --steps` batches of the plain and of the flip pipeline in that mode and nothing else;
--summarize reads the two *_kernel_stats.csv and writes, per mode, the decode kernels (grouping, compaction, adjust +
refine) with calls and microseconds per batch (each of them runs once per batch), and prints the sums per pipeline.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DECODE_KERNELS = ("match_by_tag_kernel", "match_compact_kernel", "adjust_prepare_kernel", "plane_key_from_topk_kernel",
                  "plane_argmax_kernel", "refine_shortcut_kernel", "refine_scan_kernel", "refine_finalize_kernel")


def summarize(args):
    rows = []
    for mode in ("host", "device"):
        files = glob.glob(os.path.join(args.summarize, mode, "**", "*kernel_stats.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit("match_bench: expected one *kernel_stats.csv under %s/%s, found %d"
                             % (args.summarize, mode, len(files)))
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                kernel = next((k for k in DECODE_KERNELS if k in r["Name"]), None)
                if kernel is None:
                    continue
                # every decode kernel is launched once per batch; the maps in its template arguments name the pipeline
                pipeline = "flip" if "Flip" in r["Name"] else "plain" if "Bilinear" in r["Name"] else "both"
                rows.append({"match_on": mode, "pipeline": pipeline, "kernel": kernel, "calls": int(r["Calls"]),
                             "total_ns": int(r["TotalDurationNs"]),
                             "us_per_batch": round(int(r["TotalDurationNs"]) / 1e3 / int(r["Calls"]), 2),
                             "name": r["Name"]})
    with open(args.csv, "w", newline="") as f:
        w = csv.DictWriter(f, ["match_on", "pipeline", "kernel", "calls", "total_ns", "us_per_batch", "name"])
        w.writeheader()
        w.writerows(rows)
    out = {"metric": "match_device_kernel_time", "unit": "us of GPU time per batch"}
    for mode in ("host", "device"):
        mine = [r for r in rows if r["match_on"] == mode]
        res = {"grouping": round(sum(r["us_per_batch"] for r in mine if r["kernel"].startswith("match_")), 2)}
        for pipeline in ("plain", "flip"):
            res["adjust_refine_" + pipeline] = round(sum(r["us_per_batch"] for r in mine if not r["kernel"].startswith(
                "match_") and r["pipeline"] in (pipeline, "both")), 2)
        out[mode] = res
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=4, help="timed runs per mode, interleaved A B B A ...")
    ap.add_argument("--only", choices=("host", "device"), help="run this mode alone (for a profiler), no timing")
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--summarize", metavar="DIR", help="DIR/host and DIR/device: rocprofv3 --kernel-trace --stats output")
    ap.add_argument("--csv", default=os.path.join(ROOT, "profiles", "match_device_kernel_stats.csv"))
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("match_bench: no GPU (the decode runs on the HIP path only)")
    import __graft_entry__ as entry
    entry.build()
    from oracle import synth
    from rtpe import _native as nat
    from rtpe import engine
    from rtpe.helpers import build_hrnet_w48_teacher
    from rtpe.third_party import group
    torch.set_num_threads(nat.host_threads(8))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "tests", "golden", "w48_shapes.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
    sd = synth.make_state_dict(shapes, 0, "W0")
    model = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(dev)
    B, S = args.batch, args.size
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    data = [torch.randn(B, 3, S, S, generator=g, device=dev) for _ in range(2)]

    def run(pipe, steps):
        """(img/s, CPU ms of the process per step, people of the last batch)"""
        people = 0
        torch.cuda.synchronize(dev)
        t0, c0 = time.perf_counter(), time.process_time()
        for res in pipe.stream((data[k % 2] for k in range(steps)), (S, S)):
            people = sum(len(p) if p.ndim == 3 else 0 for p, _ in res)
        torch.cuda.synchronize(dev)
        dt, cpu = time.perf_counter() - t0, time.process_time() - c0
        return B * steps / dt, cpu / steps * 1e3, people

    def pipeline(mode, flip):
        parser = group.HeatmapParser(num_joints=engine.NUM_HEATMAPS, **engine.HM_PARSER_PARAMS)
        return engine.TeacherPipeline(model, parser, device=dev, flip_test=flip, match_on=mode)

    if args.only:
        for flip in (False, True):
            run(pipeline(args.only, flip), args.warmup + args.steps)
        print(json.dumps({"metric": "match_device_profile_run", "match_on": args.only,
                          "batches": 2 * (args.warmup + args.steps)}))
        return
    out = {"metric": "match_device_throughput", "batch": B, "size": S, "steps": args.steps, "repeats": args.repeats,
           "weights": "W0", "device": torch.cuda.get_device_name(dev), "host_threads": group._HOST_THREADS,
           "cores_allowed": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None}
    for name, flip in (("plain", False), ("flip", True)):
        pipes = {mode: pipeline(mode, flip) for mode in ("host", "device")}
        for pipe in pipes.values():
            run(pipe, args.warmup)
        runs = {mode: [] for mode in pipes}
        people = {}
        for r in range(args.repeats):
            for mode in (("host", "device") if r % 2 == 0 else ("device", "host")):
                v, cpu, people[mode] = run(pipes[mode], args.steps)
                runs[mode].append((round(v, 1), round(cpu, 2)))
        res = {}
        for mode, rr in runs.items():
            v, cpu = [a for a, _ in rr], [b for _, b in rr]
            res[mode] = {"img_s": round(float(np.median(v)), 1), "img_s_runs": v,
                         "img_s_spread": round(max(v) - min(v), 1),
                         "host_cpu_ms_per_step": round(float(np.median(cpu)), 2), "host_cpu_ms_per_step_runs": cpu,
                         "people_last_batch": people[mode]}
        res["device_over_host"] = round(res["device"]["img_s"] / res["host"]["img_s"], 4)
        out[name] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
