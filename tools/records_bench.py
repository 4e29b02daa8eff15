"""The keypoint records of the teacher loop by two paths, on one GPU and in one process (batch 32, 640 x 640, W0
weights, ``match_on="device"``, a one-rank ``nccl`` group so that the all-gather really runs):

  (a) list     ``TeacherPipeline.stream`` yielding the per-image lists, then ``gather(ids, results,
               force_collective=True)``: rows to pinned memory, a host wait, Python objects, ``pack_records``, upload;
  (b) records  ``stream(records=...)``, then ``gather(None, rec, force_collective=True)``: the record kernel behind
               adjust + refine, nothing read by the host.

Everything is warmed up first, then the two paths alternate A B B A (--repeats runs of --steps steps each, every run
ends in a device synchronise).  Per path: images / s and the CPU time of the process per step (all threads,
``time.process_time``, as ``bench.py`` measures ``host_cpu_ms_per_step``) - once with the host thread pool as
``bench.py`` sets it and once held to 2 threads, the budget of 8 ranks on 16 CPUs.  No threshold: the figures are for
comparing (b) with (a) in this process.  Prints one JSON line and writes it to --out.  Needs a GPU; there is no fallback.

    python tools/records_bench.py [--steps 12] [--warmup 3] [--repeats 4]
"""
import argparse
import json
import os
import socket
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
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=4, help="timed runs per path and thread setting, interleaved A B B A")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "records_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("records_bench: no GPU (the pipeline runs on the HIP path only)")
    import torch.distributed as dist
    import __graft_entry__ as entry
    entry.build()
    from oracle import synth
    from rtpe import _native as nat
    from rtpe import engine
    from rtpe.helpers import build_hrnet_w48_teacher
    from rtpe.third_party import group
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=dev)
    try:
        with open(os.path.join(ROOT, "tests", "golden", "w48_shapes.json")) as f:
            shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
        sd = synth.make_state_dict(shapes, 0, "W0")
        model = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(dev)
        B, S = args.batch, args.size
        x = synth.make_images(B, S, S).to(dev)
        ids = list(range(B))
        pipe = engine.TeacherPipeline(model, device=dev, match_on="device")

        def run_list(steps):
            out = None
            for res in pipe.stream(x for _ in range(steps)):
                out = pipe.gather(ids, res, equal_counts=True, force_collective=True)
            return out

        def run_records(steps):
            out = None
            for rec in pipe.stream((x for _ in range(steps)), records=lambda k: (ids, None)):
                out = pipe.gather(None, rec, equal_counts=True, force_collective=True)
            return out

        paths = {"list": run_list, "records": run_records}

        def timed(run, steps):
            torch.cuda.synchronize(dev)
            t0, c0 = time.perf_counter(), time.process_time()
            out = run(steps)
            torch.cuda.synchronize(dev)
            dt, cpu = time.perf_counter() - t0, time.process_time() - c0
            return B * steps / dt, cpu / steps * 1e3, out

        last = {}
        for key, run in paths.items():
            last[key] = timed(run, args.warmup)[2]
        same = bool(torch.equal(last["list"], last["records"]))        # the same records by both paths
        default_threads = nat.host_threads(8)
        out = {"metric": "records_path_throughput", "model": "HRNet-W48 teacher", "weights": "W0", "batch": B, "size": S,
               "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "match_on": "device",
               "device": torch.cuda.get_device_name(dev), "order": "A B B A over list, records",
               "records_equal_list_path": same, "people_last_batch": int(last["records"][:, 1].sum().item())}
        for label, threads in (("default_threads", default_threads), ("two_threads", 2)):
            torch.set_num_threads(threads)
            group._HOST_THREADS = threads           # (the host matcher's pool; idle with device grouping)
            runs = {key: {"img_s": [], "cpu_ms": []} for key in paths}
            order = list(paths)
            for r in range(args.repeats):
                for key in (order if r % 2 == 0 else order[::-1]):
                    v, cpu, _ = timed(paths[key], args.steps)
                    runs[key]["img_s"].append(round(v, 1))
                    runs[key]["cpu_ms"].append(round(cpu, 2))
            sec = {"host_threads": threads}
            for key in order:
                sec[key] = {"img_s": round(float(np.median(runs[key]["img_s"])), 1), "img_s_runs": runs[key]["img_s"],
                            "host_cpu_ms_per_step": round(float(np.median(runs[key]["cpu_ms"])), 2),
                            "host_cpu_ms_per_step_runs": runs[key]["cpu_ms"]}
            sec["records_over_list_img_s"] = round(sec["records"]["img_s"] / sec["list"]["img_s"], 4)
            sec["records_over_list_host_cpu"] = round(sec["records"]["host_cpu_ms_per_step"] /
                                                      max(sec["list"]["host_cpu_ms_per_step"], 1e-9), 4)
            out[label] = sec
    finally:
        dist.destroy_process_group()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
