"""Throughput of the batched flip test against the plain pipeline and the per-image protocol, on one GPU.

In one process: seeded synthetic W0 weights, four different resident batches of synthetic images (bench.py's
headline configuration: batch 32, 640 x 640), then
  * the plain pipeline (TeacherPipeline.stream) and the flip-test pipeline (flip_test=True) in img/s;
  * the decode alone of each on the same network outputs, as GPU time between device events around the kernels of
    the two device phases (top-k; adjust + refine) - the host matching between them is not counted;
  * multi_scale_inference(scale_factors=(1,), flip_test=True) image by image on 64 uint8 images of 640 x 640.
Prints one JSON line.  Needs a GPU; there is no fallback.

``--no-project``: instead, the flip test without projection (``project2image=False``, the decode on the heat-map grid)
against the projected flip pipeline in the same process, A B B A, medians of ``--repeats`` runs of ``--steps`` batches,
with the decode's device phases and the maps buffers of both (tools/noproj_compare.py).

    python tools/flip_bench.py [--steps 20] [--warmup 3] [--images 64]
    python tools/flip_bench.py --no-project [--steps 12] [--warmup 3] [--repeats 4]
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
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=64, help="images of the per-image loop")
    ap.add_argument("--decode-reps", type=int, default=10)
    ap.add_argument("--no-project", action="store_true",
                    help="time the test without projection (project2image=False) against the projected protocol "
                         "instead: A B B A, medians of --repeats runs of --steps batches (tools/noproj_compare.py)")
    ap.add_argument("--repeats", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flip_bench: no GPU (the flip test runs on the HIP path only)")
    import __graft_entry__ as entry
    entry.build()
    from oracle import synth
    from rtpe import _native as nat
    from rtpe import engine, inference
    from rtpe.helpers import build_hrnet_w48_teacher
    torch.set_num_threads(nat.host_threads(8))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "tests", "golden", "w48_shapes.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
    sd = synth.make_state_dict(shapes, 0, "W0")
    model = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(dev)
    B, S = args.batch, args.size
    if args.no_project:
        from noproj_compare import compare
        print(json.dumps(compare(model, dev, B, S, (1,), args.steps, args.warmup, args.repeats, args.decode_reps,
                                 parse_flip=True)))
        return
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    xs = [torch.randn(B, 3, S, S, generator=g, device=dev) for _ in range(4)]
    plain = engine.TeacherPipeline(model, device=dev)
    flip = engine.TeacherPipeline(model, device=dev, flip_test=True)

    def rate(pipe, steps):
        people = 0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for res in pipe.stream((xs[k % len(xs)] for k in range(steps)), (S, S)):
            people = sum(len(p) if p.ndim == 3 else 0 for p, _ in res)
        torch.cuda.synchronize(dev)
        return B * steps / (time.perf_counter() - t0), people

    rate(plain, args.warmup)
    plain_rate, plain_people = rate(plain, args.steps)
    rate(flip, args.warmup)
    flip_rate, flip_people = rate(flip, args.steps)

    # decode alone: device events around the kernels of the two device phases, on fixed network outputs
    L = nat.lib()
    spans = []

    class Timed:
        """the library with its adjust / refine entries bracketed by events on the current stream"""
        def __getattr__(self, name):
            fn = getattr(L, name)
            if not name.startswith("rtpe_adjust_refine"):
                return fn

            def call(*a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*a)
                e1.record()
                spans.append((e0, e1))
                return rc
            return call
    with torch.no_grad():
        P, R = model(xs[0])
        Pf, Rf = model(flip.mirror(xs[0]))
    torch.cuda.synchronize(dev)

    def decode_ms(topk, reps):
        real_lib, nat._lib = nat._lib, Timed()
        try:
            total = []
            for r in range(reps + 2):
                spans.clear()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                st = topk()
                e1.record()
                plain.parser.lowres_match(st)
                plain.parser.lowres_finish(st)
                torch.cuda.synchronize(dev)
                if r >= 2:
                    total.append(e0.elapsed_time(e1) + sum(a.elapsed_time(b) for a, b in spans))
            return float(np.median(total))
        finally:
            nat._lib = real_lib
    p = plain.parser
    plain_dec = decode_ms(lambda: p.lowres_topk(R, P[:, engine.NUM_HEATMAPS:], (S, S)), args.decode_reps)
    flip_dec = decode_ms(lambda: p.flip_topk(P, R, Pf, Rf, (S, S)), args.decode_reps)

    # the per-image protocol
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8) for _ in range(args.images)]
    for img in images[:2]:
        inference.multi_scale_inference(model, p, img, S, (1,), True, True, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for img in images:
        inference.multi_scale_inference(model, p, img, S, (1,), True, True, device=dev)
    torch.cuda.synchronize(dev)
    per_image = len(images) / (time.perf_counter() - t0)
    print(json.dumps({
        "metric": "flip_test_throughput", "batch": B, "size": S, "steps": args.steps, "weights": "W0",
        "device": torch.cuda.get_device_name(dev),
        "plain_img_s": round(plain_rate, 1), "flip_img_s": round(flip_rate, 1),
        "flip_over_plain": round(flip_rate / plain_rate, 3),
        "plain_decode_gpu_ms": round(plain_dec, 3), "flip_decode_gpu_ms": round(flip_dec, 3),
        "flip_decode_over_plain": round(flip_dec / plain_dec, 3),
        "per_image_flip_img_s": round(per_image, 1), "batched_over_per_image": round(flip_rate / per_image, 1),
        "people_last_batch": {"plain": plain_people, "flip": flip_people}}))


if __name__ == "__main__":
    main()
