"""What decoding every image of a batch at its own size buys on a list of images of many sizes, and what it costs
when the sizes are all equal, on one GPU.

In one process: seeded synthetic W0 weights (noise maps: the decode's worst case, 30 people per image), then

--what mix (default)   a seeded mix of COCO-like image sizes (70 % landscape of width 640 and height 360..480, 20 %
    portrait, 10 % of width 500 and height 300..400; numpy.random.default_rng(2017)), random uint8 pixels, through
      A  rtpe.inference.plain_inference: batches share the network input size only, every image decoded at its own
         (h, w);
      B  what a decode with ONE size per batch allows: the same images grouped by (input size, original size), each
         group streamed through TeacherPipeline.stream with its (h, w) tuple.
    Both are run once first (every (N, H, W) they use is autotuned there; the duration of that pass is reported
    separately), then timed A B B A ... (--repeats passes each): images/s, batches (= forwards) per pass, CPU ms of
    the process per pass, medians beside every run and their spread.  The results of A and B are compared bit for bit.

--what equal   batch 32, 640 x 640, all sizes equal: TeacherPipeline.stream with the list form (A) against the tuple
    form (B), --steps batches per run, the same order and statistics.

Prints one JSON line per --what (--out FILE also writes them).  Needs a GPU; there is no fallback.

    python tools/mixed_size_bench.py [--what mix equal] [--images 256] [--repeats 4] [--out profiles/mixed_size_bench.json]

GPU time of the decode kernels (a run of its own, the timing above is not taken under the profiler):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/list -o t -- python tools/mixed_size_bench.py --only list --steps 10
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/tuple -o t -- python tools/mixed_size_bench.py --only tuple --steps 10
    python tools/mixed_size_bench.py --summarize DIR --csv profiles/mixed_size_kernel_stats.csv

--only FORM runs `--warmup + --steps` batches of the equal-size stream in that form and nothing else; --summarize reads
the two *_kernel_stats.csv and writes the decode kernels of either form with calls and microseconds per call.
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

DECODE_KERNELS = ("topk_tile_kernel", "topk_merge_kernel", "adjust_prepare_kernel", "plane_key_from_topk_kernel",
                  "plane_argmax_kernel", "refine_shortcut_kernel", "refine_scan_kernel", "refine_finalize_kernel")


def mix_sizes(n):
    import numpy as np
    rng = np.random.default_rng(2017)
    sizes = []
    for _ in range(n):
        r = rng.uniform()
        if r < 0.7:
            sizes.append((int(rng.integers(360, 481)), 640))
        elif r < 0.9:
            sizes.append((640, int(rng.integers(360, 481))))
        else:
            sizes.append((int(rng.integers(300, 401)), 500))
    return sizes


def summarize(args):
    rows = []
    for form in ("list", "tuple"):
        files = glob.glob(os.path.join(args.summarize, form, "**", "*kernel_stats.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit("mixed_size_bench: expected one *kernel_stats.csv under %s/%s, found %d"
                             % (args.summarize, form, len(files)))
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                kernel = next((k for k in DECODE_KERNELS if k in r["Name"]), None)
                if kernel is None:
                    continue
                rows.append({"out_hw": form, "kernel": kernel, "calls": int(r["Calls"]),
                             "total_ns": int(r["TotalDurationNs"]),
                             "us_per_call": round(int(r["TotalDurationNs"]) / 1e3 / int(r["Calls"]), 2),
                             "name": r["Name"]})
    with open(args.csv, "w", newline="") as f:
        w = csv.DictWriter(f, ["out_hw", "kernel", "calls", "total_ns", "us_per_call", "name"])
        w.writeheader()
        w.writerows(rows)
    out = {"metric": "mixed_size_kernel_time", "unit": "us of GPU time per batch, decode kernels (one call each per batch)"}
    for form in ("list", "tuple"):
        mine = [r for r in rows if r["out_hw"] == form]
        out[form] = {"decode_us_per_batch": round(sum(r["us_per_call"] for r in mine), 2),
                     "kernels": {r["kernel"]: r["us_per_call"] for r in mine}}
    print(json.dumps(out))


def stats(runs):
    import numpy as np
    v, cpu = [a for a, _ in runs], [b for _, b in runs]
    return {"img_s": round(float(np.median(v)), 1), "img_s_runs": v, "img_s_spread": round(max(v) - min(v), 1),
            "host_cpu_ms": round(float(np.median(cpu)), 2), "host_cpu_ms_runs": cpu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["mix"], choices=("mix", "equal"))
    ap.add_argument("--images", type=int, default=256, help="images of the seeded mix")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20, help="batches per timed run of --what equal")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=4, help="timed runs per mode, interleaved A B B A ...")
    ap.add_argument("--match-on", default="host", choices=("host", "device"))
    ap.add_argument("--only", choices=("list", "tuple"), help="equal sizes in this form alone (for a profiler), no timing")
    ap.add_argument("--out", help="also write the JSON lines to this file")
    ap.add_argument("--summarize", metavar="DIR", help="DIR/list and DIR/tuple: rocprofv3 --kernel-trace --stats output")
    ap.add_argument("--csv", default=os.path.join(ROOT, "profiles", "mixed_size_kernel_stats.csv"))
    args = ap.parse_args()
    if args.summarize:
        return summarize(args)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mixed_size_bench: no GPU (the decode runs on the HIP path only)")
    import __graft_entry__ as entry
    entry.build()
    from oracle import synth
    from rtpe import _native as nat
    from rtpe import engine, inference
    from rtpe.helpers import build_hrnet_w48_teacher
    from rtpe.third_party import group, transforms
    torch.set_num_threads(nat.host_threads(8))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "tests", "golden", "w48_shapes.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
    sd = synth.make_state_dict(shapes, 0, "W0")
    model = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(dev)

    def parser():
        return group.HeatmapParser(num_joints=engine.NUM_HEATMAPS, **engine.HM_PARSER_PARAMS)
    lines = []
    common = {"weights": "W0", "device": torch.cuda.get_device_name(dev), "match_on": args.match_on,
              "host_threads": group._HOST_THREADS, "repeats": args.repeats}

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0, c0 = time.perf_counter(), time.process_time()
        res = fn()
        torch.cuda.synchronize(dev)
        return res, time.perf_counter() - t0, (time.process_time() - c0) * 1e3

    def interleave(modes, n_images):
        runs = {m: [] for m in modes}
        names = list(modes)
        for r in range(args.repeats):
            for m in (names if r % 2 == 0 else names[::-1]):
                _, dt, cpu = timed(modes[m])
                runs[m].append((round(n_images / dt, 1), round(cpu, 1)))
        return {m: stats(rr) for m, rr in runs.items()}

    if args.only or "equal" in args.what:
        B, S = args.batch, args.size
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        data = [torch.randn(B, 3, S, S, generator=g, device=dev) for _ in range(2)]
        pipe = engine.TeacherPipeline(model, parser(), device=dev, match_on=args.match_on)
        forms = {"list": [(S, S)] * B, "tuple": (S, S)}

        def stream(form, steps):
            people = 0
            for res in pipe.stream((data[k % 2] for k in range(steps)), forms[form]):
                people = sum(len(p) if p.ndim == 3 else 0 for p, _ in res)
            return people
        if args.only:
            stream(args.only, args.warmup + args.steps)
            print(json.dumps({"metric": "mixed_size_profile_run", "out_hw": args.only, "batches": args.warmup + args.steps}))
            return
        people = {f: stream(f, args.warmup) for f in forms}
        res = interleave({f: (lambda f=f: stream(f, args.steps)) for f in forms}, B * args.steps)
        for f in forms:
            res[f]["people_last_batch"] = people[f]
            res[f]["host_cpu_ms_per_step"] = round(res[f].pop("host_cpu_ms") / args.steps, 2)
            res[f]["host_cpu_ms_per_step_runs"] = [round(c / args.steps, 2) for c in res[f].pop("host_cpu_ms_runs")]
        res["list_over_tuple"] = round(res["list"]["img_s"] / res["tuple"]["img_s"], 4)
        lines.append(dict(common, metric="equal_sizes_list_against_tuple", batch=B, size=S, steps=args.steps, **res))

    if "mix" in args.what:
        sizes = mix_sizes(args.images)
        rng = np.random.default_rng(5)
        images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
        plan_a = inference.plain_plan(sizes, args.size, args.batch)
        plan_b = inference.plain_plan(sizes, args.size, args.batch, by_original_size=True)
        pa, pb = parser(), parser()

        def mode_a():
            return inference.plain_inference(model, pa, images, args.size, args.batch, device=dev, match_on=args.match_on)

        pipe_b = engine.TeacherPipeline(model, pb, device=dev, match_on=args.match_on)

        def mode_b():
            """the images grouped by (input size, original size); one stream per group, its (h, w) as a tuple"""
            out = [None] * len(images)
            groups = {}
            for c in plan_b:
                groups.setdefault(sizes[c[0]], []).append(c)
            with torch.no_grad():
                for hw, chunks in groups.items():
                    batches = (torch.cat([transforms.warp_normalize(images[i], args.size, 1, 1, device=dev)[0]
                                          for i in c]) for c in chunks)
                    for c, res in zip(chunks, pipe_b.stream(batches, hw)):
                        for i, r in zip(c, res):
                            out[i] = r
            return out
        ra, warm_a, _ = timed(mode_a)
        rb, warm_b, _ = timed(mode_b)
        same = all(np.array_equal(a[0], b[0]) and np.array_equal(np.array(a[1], np.float32), np.array(b[1], np.float32))
                   for a, b in zip(ra, rb))
        res = interleave({"per_image_sizes": mode_a, "one_size_per_batch": mode_b}, len(images))
        res["per_image_sizes"].update(batches_per_pass=len(plan_a), first_pass_s=round(warm_a, 2))
        res["one_size_per_batch"].update(batches_per_pass=len(plan_b), first_pass_s=round(warm_b, 2))
        res["speedup"] = round(res["per_image_sizes"]["img_s"] / res["one_size_per_batch"]["img_s"], 3)
        lines.append(dict(common, metric="mixed_sizes_plain_inference", images=len(images), batch=args.batch,
                          input_size=args.size, distinct_original_sizes=len(set(sizes)),
                          people=sum(len(p) if p.ndim == 3 else 0 for p, _ in ra), results_bit_identical=bool(same),
                          **res))
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
