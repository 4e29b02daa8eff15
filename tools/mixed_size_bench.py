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

--what warp   what making the input batches costs: the seeded mix through rtpe.inference.plain_inference with
    warp="image" (A: one upload, one allocation and one launch per image, then a concatenation) and warp="batch"
    (B: transforms.warp_normalize_batch, one upload and one launch per batch), and the first --ms-images images of the
    mix through multi_scale_batch_inference((2, 1, 0.5), flip_test=True) likewise (A: three uploads and launches per
    image).  The same order, repeats and statistics; besides images/s and the CPU time of the process, the wall time
    the host spends PRODUCING the batches (around the `next` of the generator the pipeline draws them from, no device
    synchronisation), per batch.  The results of A and B are compared bit for bit.

Prints one JSON line per --what (--out FILE also writes them).  Needs a GPU; there is no fallback.

    python tools/mixed_size_bench.py [--what mix equal warp] [--images 256] [--repeats 4] [--out profiles/mixed_size_bench.json]
    python tools/mixed_size_bench.py --what warp --out profiles/warp_batch_bench.json

GPU time of the decode kernels (a run of its own, the timing above is not taken under the profiler):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/list -o t -- python tools/mixed_size_bench.py --only list --steps 10
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/tuple -o t -- python tools/mixed_size_bench.py --only tuple --steps 10
    python tools/mixed_size_bench.py --summarize DIR --csv profiles/mixed_size_kernel_stats.csv

--only FORM runs `--warmup + --steps` batches of the equal-size stream in that form and nothing else; --summarize reads
the two *_kernel_stats.csv and writes the decode kernels of either form with calls and microseconds per call.

GPU time of the two warp kernels and the number of copies (again runs of their own):

    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR/image -o t -- python tools/mixed_size_bench.py --only-warp image --images 64 --ms-images 8
    rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d DIR/batch -o t -- python tools/mixed_size_bench.py --only-warp batch --images 64 --ms-images 8
    python tools/mixed_size_bench.py --summarize-warp DIR --csv profiles/warp_batch_kernel_stats.csv

--only-warp MODE runs one pass of either protocol with that warp and nothing else; --summarize-warp writes, per mode,
calls and microseconds per call of warp_normalize_kernel / warp_normalize_batch_kernel and of the concatenation kernel,
and the copies by direction.
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


WARP_KERNELS = ("warp_normalize_batch_kernel", "warp_normalize_kernel", "CatArrayBatchedCopy")


def summarize_warp(args):
    """DIR/image and DIR/batch -> one CSV: the warp kernels (and torch.cat's copy kernel) and the copies of either mode"""
    rows = []
    for mode in ("image", "batch"):
        def one(pattern):
            files = glob.glob(os.path.join(args.summarize_warp, mode, "**", pattern), recursive=True)
            if len(files) > 1:
                raise SystemExit("mixed_size_bench: more than one %s under %s/%s" % (pattern, args.summarize_warp, mode))
            return files[0] if files else None
        path = one("*kernel_stats.csv")
        if path is None:
            raise SystemExit("mixed_size_bench: no *kernel_stats.csv under %s/%s" % (args.summarize_warp, mode))
        with open(path) as f:
            for r in csv.DictReader(f):
                kernel = next((k for k in WARP_KERNELS if k in r["Name"]), None)
                if kernel is not None:
                    rows.append({"warp": mode, "kind": "kernel", "what": kernel, "calls": int(r["Calls"]),
                                 "total_ns": int(r["TotalDurationNs"]),
                                 "us_per_call": round(int(r["TotalDurationNs"]) / 1e3 / int(r["Calls"]), 2),
                                 "name": r["Name"]})
        path = one("*memory_copy_stats.csv")
        if path is not None:
            with open(path) as f:
                for r in csv.DictReader(f):
                    rows.append({"warp": mode, "kind": "copy", "what": r["Name"], "calls": int(r["Calls"]),
                                 "total_ns": int(r["TotalDurationNs"]),
                                 "us_per_call": round(int(r["TotalDurationNs"]) / 1e3 / int(r["Calls"]), 2), "name": ""})
    with open(args.csv, "w", newline="") as f:
        w = csv.DictWriter(f, ["warp", "kind", "what", "calls", "total_ns", "us_per_call", "name"])
        w.writeheader()
        w.writerows(rows)
    print(json.dumps({"metric": "warp_kernel_time", "rows": [{k: r[k] for k in ("warp", "kind", "what", "calls",
                                                                                 "us_per_call")} for r in rows]}))


def stats(runs):
    import numpy as np
    v, cpu = [a for a, _ in runs], [b for _, b in runs]
    return {"img_s": round(float(np.median(v)), 1), "img_s_runs": v, "img_s_spread": round(max(v) - min(v), 1),
            "host_cpu_ms": round(float(np.median(cpu)), 2), "host_cpu_ms_runs": cpu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["mix"], choices=("mix", "equal", "warp"))
    ap.add_argument("--ms-images", type=int, default=32, help="images of the multi-scale leg of --what warp")
    ap.add_argument("--only-warp", choices=("image", "batch"),
                    help="one pass of both protocols with this warp alone (for a profiler), no timing")
    ap.add_argument("--summarize-warp", metavar="DIR",
                    help="DIR/image and DIR/batch: rocprofv3 --kernel-trace --memory-copy-trace --stats output")
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
    if args.summarize_warp:
        return summarize_warp(args)
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

    if args.only_warp or "warp" in args.what:
        produce = []        # seconds the host spent in `next` of the batch generator, one entry per batch

        class TimedPipeline(engine.TeacherPipeline):
            """stream() draws its batches through a generator that times each `next` on the host (no device sync)"""

            def stream(self, batches, *a, **kw):
                def drawn():
                    it = iter(batches)
                    while True:
                        t0 = time.perf_counter()
                        try:
                            x = next(it)
                        except StopIteration:
                            return
                        produce.append(time.perf_counter() - t0)
                        yield x
                return super().stream(drawn(), *a, **kw)
        engine.TeacherPipeline = TimedPipeline          # the drivers import the name when they are called
        sizes = mix_sizes(args.images)
        rng = np.random.default_rng(5)
        images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
        ms_images = images[:args.ms_images]
        ms_scales = (2, 1, 0.5)
        legs = {
            "plain": (images, lambda warp: inference.plain_inference(
                model, parser(), images, args.size, args.batch, device=dev, match_on=args.match_on, warp=warp)),
            "multi_scale": (ms_images, lambda warp: inference.multi_scale_batch_inference(
                model, parser(), ms_images, args.size, ms_scales, True, batch_size=args.batch, device=dev,
                match_on=args.match_on, warp=warp)),
        }
        if args.only_warp:
            for name, (imgs, run) in legs.items():
                run(args.only_warp)
            torch.cuda.synchronize(dev)
            print(json.dumps({"metric": "warp_profile_run", "warp": args.only_warp, "images": len(images),
                              "ms_images": len(ms_images), "batches": len(produce)}))
            return

        def same_results(ra, rb):
            def rows(r):
                return [np.asarray(p, np.float32) for p in (r[0] if isinstance(r[0], list) else [r[0]])]
            return all(len(rows(a)) == len(rows(b)) and all(np.array_equal(x, y) for x, y in zip(rows(a), rows(b)))
                       and np.array_equal(np.array(a[1], np.float32), np.array(b[1], np.float32))
                       for a, b in zip(ra, rb))
        for name, (imgs, run) in legs.items():
            first = {}
            for warp in ("image", "batch"):
                first[warp], dt, _ = timed(lambda: run(warp))
                first[warp + "_s"] = round(dt, 2)
            host = {"image": [], "batch": []}

            def mode(warp):
                def fn():
                    del produce[:]
                    res = run(warp)
                    host[warp].append((round(sum(produce) * 1e3, 2), len(produce)))
                    return res
                return fn
            res = interleave({"warp_image": mode("image"), "warp_batch": mode("batch")}, len(imgs))
            for warp in ("image", "batch"):
                ms_total = [h[0] for h in host[warp]]
                n_batches = host[warp][0][1]
                scales_per_image = len(ms_scales) if name == "multi_scale" else 1
                res["warp_" + warp].update(
                    batches_per_pass=n_batches, first_pass_s=first[warp + "_s"],
                    produce_host_ms_per_pass=round(float(np.median(ms_total)), 2), produce_host_ms_per_pass_runs=ms_total,
                    produce_host_ms_per_batch=round(float(np.median(ms_total)) / n_batches, 3),
                    uploads_per_pass=len(imgs) * scales_per_image if warp == "image" else n_batches,
                    warp_launches_per_pass=(len(imgs) if warp == "image" else n_batches) * scales_per_image)
            res["speedup_img_s"] = round(res["warp_batch"]["img_s"] / res["warp_image"]["img_s"], 4)
            res["produce_host_ratio"] = round(res["warp_image"]["produce_host_ms_per_pass"]
                                              / max(res["warp_batch"]["produce_host_ms_per_pass"], 1e-9), 2)
            lines.append(dict(common, metric="warp_image_against_warp_batch", protocol=name, images=len(imgs),
                              batch=args.batch, input_size=args.size,
                              scales=list(ms_scales) if name == "multi_scale" else [1], flip=name == "multi_scale",
                              people=sum(len(r[0]) if isinstance(r[0], list) else (len(r[0]) if r[0].ndim == 3 else 0)
                                         for r in first["image"]),
                              results_bit_identical=bool(same_results(first["image"], first["batch"])), **res))
        engine.TeacherPipeline = TimedPipeline.__mro__[1]

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
