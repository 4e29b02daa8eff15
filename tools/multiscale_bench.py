"""Throughput of the batched multi-scale test against the plain and flip pipelines and the per-image protocol, on
one GPU.

In one process: seeded synthetic W0 weights, resident synthetic batches (batch 32, 640 x 640 at scale 1; the scale
inputs are 1280 x 1280, 640 x 640 and 320 x 320 for the default scales (2, 1, 0.5)), then
  * the plain, flip-test and multi-scale (+ flip) pipelines (TeacherPipeline.stream) in img/s;
  * per multi-scale batch: the GPU time of the forwards (device events around each sub-batch's forwards, run alone)
    and of the decode's device phases (prep, top-k, adjust + refine; the host matching is not counted);
  * multi_scale_inference with the same scales and flip image by image on --images uint8 images of 640 x 640;
  * the workspace bytes of every forward shape and whether the workspace cache evicted anything in the steady
    state of the multi-scale pipeline.
Prints one JSON line.  Needs a GPU; there is no fallback.

``--no-project``: instead, the multi-scale (+ flip) test without projection (``project2image=False``) against the
projected one in the same process, A B B A, medians of ``--repeats`` runs of ``--steps`` batches, with the decode's
device phases and the maps buffers of both (tools/noproj_compare.py).

    python tools/multiscale_bench.py [--steps 6] [--warmup 2] [--images 32]
    python tools/multiscale_bench.py --no-project [--steps 12] [--warmup 2] [--repeats 4]
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
    ap.add_argument("--scales", type=str, default="2,1,0.5")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=32, help="images of the per-image loop")
    ap.add_argument("--decode-reps", type=int, default=5)
    ap.add_argument("--no-project", action="store_true",
                    help="time the test without projection (project2image=False) against the projected protocol "
                         "instead: A B B A, medians of --repeats runs of --steps batches (tools/noproj_compare.py)")
    ap.add_argument("--repeats", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiscale_bench: no GPU (the multi-scale test runs on the HIP path only)")
    import __graft_entry__ as entry
    entry.build()
    from oracle import synth
    from rtpe import _native as nat
    from rtpe import engine, inference
    from rtpe.helpers import build_hrnet_w48_teacher
    from rtpe.third_party import pose_higher_hrnet as phh
    torch.set_num_threads(nat.host_threads(8))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "tests", "golden", "w48_shapes.json")) as f:
        shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
    sd = synth.make_state_dict(shapes, 0, "W0")
    model = build_hrnet_w48_teacher({"1." + k: v for k, v in sd.items()}).to(dev)
    B, S = args.batch, args.size
    scales = inference.check_scale_factors([float(v) if "." in v else int(v) for v in args.scales.split(",")])
    if args.no_project:
        from noproj_compare import compare
        print(json.dumps(compare(model, dev, B, S, scales, args.steps, args.warmup, args.repeats, args.decode_reps)))
        return
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    xs = [torch.randn(B, 3, S, S, generator=g, device=dev) for _ in range(2)]
    xms = [[torch.randn(B, 3, int(S * s), int(S * s), generator=g, device=dev) for s in scales] for _ in range(2)]
    plain = engine.TeacherPipeline(model, device=dev)
    flip = engine.TeacherPipeline(model, device=dev, flip_test=True)
    ms = engine.TeacherPipeline(model, device=dev, flip_test=True, scale_factors=scales)

    def rate(pipe, data, steps, hw):
        people = 0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for res in pipe.stream((data[k % len(data)] for k in range(steps)), hw):
            people = sum(len(p) if p.ndim == 3 else 0 for p, _ in res)
        torch.cuda.synchronize(dev)
        return B * steps / (time.perf_counter() - t0), people

    rate(plain, xs, args.warmup, (S, S))
    plain_rate, plain_people = rate(plain, xs, max(args.steps, 10), (S, S))
    rate(flip, xs, args.warmup, (S, S))
    flip_rate, flip_people = rate(flip, xs, max(args.steps, 10), (S, S))
    # the workspace cache: watch what Engine.workspace drops (the bench tool's own instrumentation)
    engines, dropped = [], []
    orig_ws = phh.Engine.workspace

    def workspace(self, N, H, W):
        before = set(self._ws)
        out = orig_ws(self, N, H, W)
        dropped.extend(before - set(self._ws))
        if self not in engines:
            engines.append(self)
        return out
    phh.Engine.workspace = workspace
    rate(ms, xms, args.warmup, (S, S))
    n_warm = len(dropped)
    ms_rate, ms_people = rate(ms, xms, args.steps, (S, S))
    steady_drops = dropped[n_warm:]
    phh.Engine.workspace = orig_ws
    ws = {"x".join(map(str, k)): int(t.numel()) for e in engines for k, t in e._ws.items()}

    # one multi-scale batch, every step alone: forwards (per sub-batch) and the decode's device phases
    P = ms.parser
    fwd_ms, fwd_shapes, prep_ms, topk_ms, refine_ms = [], {}, [], [], []
    L = nat.lib()

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a)
        e1.record()
        return out, (e0, e1)

    class Timed:
        def __getattr__(self, name):
            fn = getattr(L, name)
            if not name.startswith("rtpe_adjust_refine"):
                return fn

            def call(*a):
                rc, ev = timed(fn, *a)
                spans.append(ev)
                return rc
            return call
    spans = []
    kind = ms._kind(lambda k: (S, S))           # the pipeline's own steps, with a timing forward and a timing decode
    with torch.no_grad():
        for r in range(args.decode_reps + 1):
            fw, pr = [], []
            batch, hw = kind.begin(r, xms[r % 2])
            st = kind.open(batch, hw, lambda fn, *a: fn(*a))
            kind.forwards(r, batch, lambda k, t: _rec(timed(model, t), fw, tuple(t.shape[2:])), st,
                          lambda fn, *a, after=None, uses=(): pr.append(timed(fn, *a)[1]))
            _, tk = timed(kind.topk, (), hw, st)
            real, nat._lib = nat._lib, Timed()
            spans.clear()
            try:
                P.lowres_match(st)
                P.lowres_finish(st)
            finally:
                nat._lib = real
            torch.cuda.synchronize(dev)
            if r == 0:
                continue
            fwd_ms.append(sum(a.elapsed_time(b) for _, (a, b) in fw))
            for hw, (a, b) in fw:
                fwd_shapes.setdefault("x".join(map(str, hw)), []).append(a.elapsed_time(b))
            prep_ms.append(sum(a.elapsed_time(b) for a, b in pr))
            topk_ms.append(tk[0].elapsed_time(tk[1]))
            refine_ms.append(sum(a.elapsed_time(b) for a, b in spans))

    # the per-image protocol
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8) for _ in range(args.images)]
    for img in images[:2]:
        inference.multi_scale_inference(model, P, img, S, scales, True, True, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for img in images:
        inference.multi_scale_inference(model, P, img, S, scales, True, True, device=dev)
    torch.cuda.synchronize(dev)
    per_image = len(images) / (time.perf_counter() - t0)
    med = lambda v: round(float(np.median(v)), 3)      # noqa: E731
    print(json.dumps({
        "metric": "multi_scale_test_throughput", "batch": B, "size": S, "scales": list(scales), "flip": True,
        "steps": args.steps, "weights": "W0", "device": torch.cuda.get_device_name(dev),
        "max_forward_pixels": ms.max_forward_pixels,
        "plain_img_s": round(plain_rate, 1), "flip_img_s": round(flip_rate, 1), "ms_img_s": round(ms_rate, 1),
        "ms_over_plain": round(ms_rate / plain_rate, 4), "ms_over_flip": round(ms_rate / flip_rate, 4),
        "per_batch_gpu_ms": {"forwards": med(fwd_ms), "prep": med(prep_ms), "topk": med(topk_ms),
                             "adjust_refine": med(refine_ms)},
        "forward_gpu_ms_by_input_shape": {k: med(v) for k, v in fwd_shapes.items()},
        "per_image_ms_img_s": round(per_image, 2), "batched_over_per_image": round(ms_rate / per_image, 1),
        "workspace": {"bytes_by_N_H_W_slot": ws, "total_bytes": sum(ws.values()),
                      "budget_bytes": phh.Engine.WS_BUDGET_BYTES, "evicted_during_warmup": n_warm,
                      "evicted_in_steady_state": len(steady_drops)},
        "people_last_batch": {"plain": plain_people, "flip": flip_people, "ms": ms_people}}))


def _rec(res, acc, hw):
    out, ev = res
    acc.append((hw, ev))
    return out



if __name__ == "__main__":
    main()
