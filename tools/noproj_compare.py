"""The ``--no-project`` mode of tools/flip_bench.py and tools/multiscale_bench.py: the batched test without projection
to the image (``TeacherPipeline(..., project2image=False)``) against the projected protocol of the same scales, in one
process - both pipelines warmed up, then timed in the order A B B A ... (``repeats`` runs of ``steps`` batches each),
the median beside every run; per batch, every step alone, the GPU time of the decode's device phases (prep, top-k,
adjust + refine; the host matching is not counted) and the bytes of the maps buffer."""
import time

import numpy as np
import torch


def compare(model, dev, B, S, scales, steps, warmup, repeats, decode_reps, parse_flip=False):
    """``parse_flip``: the projected protocol is the single-scale flip pipeline (``flip_test=True`` without
    ``scale_factors``, ``HeatmapParser.parse_flip``), what ``flip_test_inference`` runs; ``scales`` is then (1,)"""
    from rtpe import _native as nat
    from rtpe import engine
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    data = [[torch.randn(B, 3, int(S * s), int(S * s), generator=g, device=dev) for s in scales] for _ in range(2)]
    pipes = {"projected": engine.TeacherPipeline(model, device=dev, flip_test=True,
                                                 scale_factors=None if parse_flip else scales),
             "no_project": engine.TeacherPipeline(model, device=dev, flip_test=True, scale_factors=scales,
                                                  project2image=False)}

    def rate(pipe, n):
        people = 0
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        one = pipe.scale_factors is None        # (the parse_flip pipeline takes a tensor, not one per scale)
        for res in pipe.stream((data[k % len(data)][0] if one else data[k % len(data)]) for k in range(n)):
            people = sum(len(p) if p.ndim == 3 else 0 for p, _ in res)
        torch.cuda.synchronize(dev)
        return B * n / (time.perf_counter() - t0), people

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
            if not name.startswith("rtpe_adjust_refine"):
                return fn

            def call(*a):
                rc, ev = timed(fn, *a)
                spans.append(ev)
                return rc
            return call

    def decode_times(pipe):
        P = pipe.parser
        prep_ms, topk_ms, refine_ms, maps_bytes = [], [], [], 0
        # the pipeline's own steps, with a timing decode (parse_flip: no prep, it is part of the top-k entry)
        kind = pipe._kind(lambda k: None)
        with torch.no_grad():
            for r in range(decode_reps + 1):
                pr = []
                batch, hw = kind.begin(r, data[r % 2][0] if pipe.scale_factors is None else data[r % 2])
                state = kind.open(batch, hw, lambda fn, *a: fn(*a))
                outs = kind.forwards(r, batch, None, state,
                                     lambda fn, *a, after=None, uses=(): pr.append(timed(fn, *a)[1]))
                st, tk = timed(kind.topk, outs, hw, state)
                maps_bytes = st["maps"].numel() * 4
                real, nat._lib = nat._lib, Timed()
                spans.clear()
                try:
                    P.lowres_match(st)
                    P.lowres_finish(st)
                finally:
                    nat._lib = real
                torch.cuda.synchronize(dev)
                if r:
                    prep_ms.append(sum(a.elapsed_time(b) for a, b in pr))
                    topk_ms.append(tk[0].elapsed_time(tk[1]))
                    refine_ms.append(sum(a.elapsed_time(b) for a, b in spans))
        med = lambda v: round(float(np.median(v)), 3)      # noqa: E731
        return {"prep": med(prep_ms), "topk": med(topk_ms), "adjust_refine": med(refine_ms),
                "total": med(np.array(prep_ms) + np.array(topk_ms) + np.array(refine_ms)),
                "decode_grid": list(st["hw"])}, maps_bytes

    for pipe in pipes.values():
        rate(pipe, warmup)
    runs, people = {k: [] for k in pipes}, {}
    for r in range(repeats):
        for key in (("projected", "no_project") if r % 2 == 0 else ("no_project", "projected")):
            v, people[key] = rate(pipes[key], steps)
            runs[key].append(round(v, 1))
    out = {"metric": "no_project_throughput", "batch": B, "size": S, "scales": list(scales), "flip": True,
           "steps": steps, "repeats": repeats, "weights": "W0", "device": torch.cuda.get_device_name(dev)}
    for key, pipe in pipes.items():
        times, nbytes = decode_times(pipe)
        out[key] = {"img_s": round(float(np.median(runs[key])), 1), "img_s_runs": runs[key],
                    "img_s_range": [min(runs[key]), max(runs[key])], "decode_gpu_ms_per_batch": times,
                    "maps_bytes": nbytes}
    out["no_project_over_projected"] = round(out["no_project"]["img_s"] / out["projected"]["img_s"], 4)
    lo, hi = out["projected"]["img_s_range"]
    out["no_project_within_the_range_of_projected"] = bool(lo <= out["no_project"]["img_s"] <= hi)
    out["people_last_batch"] = people
    return out
