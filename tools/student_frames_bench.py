"""What the students' frames front end (``students.pack_frames``: one upload and one launch per batch write both input
canvases) buys in front of ``forward_mixed``, on one GPU.

The seeded 256-size mix of ``tools/mixed_size_bench.py`` (``mix_sizes``) as uint8 HOST frames, batches of 32 cut by area
(``StudentPipeline.frame_batches``), one process, everything run once first, then timed A B B A ..., medians of
``--repeats`` passes.

Front end alone (host frames -> the image canvas and the LAB canvas on the GPU, per batch):
  A1  ``to_tensor`` / ``Normalize`` on the host, one fp32 upload per image (the image and, for LAB, ``to_tensor`` of it),
      ``dataloaders.rgb2lab`` per image, ``pack_mixed`` x 2 - the bit-identical old path (compared once, bit for bit);
  A2  one uint8 upload per image, ``/ 255`` and ``Normalize`` by torch on the GPU, ``rgb2lab`` per image, ``pack_mixed`` x 2 -
      the fastest thing to write without the new kernel.  Its BITS DIFFER: torch's GPU division by 255 multiplies by the
      reciprocal (126 of the 256 levels round otherwise), so its canvases are compared with a tolerance only;
  B   ``pack_frames(frames, "LAB")``.
Also B without the second canvas (``pack_frames(frames)``) against A1 / A2 without theirs.

End to end from host frames (``--what pipeline``): ``stream_mixed`` fed by A2 against ``stream_frames``, for
``AttentionStudent(inplanes=100, body_half=True)`` and ``AttentionStudentSteps(inplanes=48)`` with LAB (seeded W1 weights).

Reports images/s, ms per batch and CPU ms of the process per batch.  Prints one JSON line per measurement (--out FILE also
writes them).  Needs a GPU; there is no fallback.

    python tools/student_frames_bench.py [--what frontend pipeline] [--images 256] [--repeats 4] [--out profiles/student_frames_bench.json]

``--what kernel`` times the kernel alone on the first batch of the mix already on the device (hipEvents around
``--kernel-iters`` launches): the three modes, and LAB through the LDS table of the sRGB linearisation against the direct
form, A B B A in one process (profiles/frames_kernel_ab.txt).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["frontend", "pipeline"], choices=("frontend", "pipeline", "kernel"))
    ap.add_argument("--images", type=int, default=256, help="images of the seeded mix")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=4, help="timed passes per mode, interleaved A B B A ...")
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--out", help="also write the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("student_frames_bench: no GPU (the front end runs on the HIP path only)")
    import __graft_entry__ as entry
    entry.build()
    from mixed_size_bench import mix_sizes
    from oracle import synth
    from rtpe import _native as nat
    from rtpe import dataloaders, engine
    from rtpe.students import AttentionStudent, AttentionStudentSteps, pack_frames, pack_mixed
    from rtpe.third_party.transforms import IMAGENET_MEAN, IMAGENET_STD
    torch.set_num_threads(nat.host_threads(8))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sizes = mix_sizes(args.images)
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    batches, _ = engine.StudentPipeline.frame_batches(frames, args.batch)
    n_batches = len(batches)
    mean_h, std_h = torch.tensor(IMAGENET_MEAN)[:, None, None], torch.tensor(IMAGENET_STD)[:, None, None]
    mean_d, std_d = mean_h.to(dev), std_h.to(dev)
    common = {"device": torch.cuda.get_device_name(dev), "images": len(frames), "batch": args.batch, "batches": n_batches,
              "repeats": args.repeats, "frame_megabytes_uint8": round(sum(f.nbytes for f in frames) / 1e6, 1)}

    def a1(fs, lab=True):
        """host to_tensor / Normalize, fp32 uploads, rgb2lab, pack_mixed x 2"""
        xs, ts = [], []
        for f in fs:
            t = torch.from_numpy(f).permute(2, 0, 1).contiguous().float().div(255)
            xs.append(t.clone().sub_(mean_h).div_(std_h).to(dev, non_blocking=True))
            if lab:
                ts.append(t.to(dev, non_blocking=True))
        canvas, sz = pack_mixed(xs)
        alt = pack_mixed([dataloaders.rgb2lab(t) for t in ts], canvas_hw=canvas.shape[2:])[0] if lab else None
        return canvas, sz, alt

    def a2(fs, lab=True):
        """uint8 uploads, torch ops on the GPU, rgb2lab, pack_mixed x 2"""
        xs, labs = [], []
        for f in fs:
            t = torch.from_numpy(f).to(dev, non_blocking=True).permute(2, 0, 1).float().div(255)
            if lab:
                labs.append(dataloaders.rgb2lab(t))
            xs.append(t.sub(mean_d).div_(std_d))
        canvas, sz = pack_mixed(xs)
        alt = pack_mixed(labs, canvas_hw=canvas.shape[2:])[0] if lab else None
        return canvas, sz, alt

    def b(fs, lab=True):
        return pack_frames(fs, "LAB" if lab else None, device=dev)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0, c0 = time.perf_counter(), time.process_time()
        res = fn()
        torch.cuda.synchronize(dev)
        return res, time.perf_counter() - t0, (time.process_time() - c0) * 1e3

    def interleave(modes):
        runs = {m: [] for m in modes}
        names = list(modes)
        for r in range(args.repeats):
            for m in (names if r % 2 == 0 else names[::-1]):
                _, dt, cpu = timed(modes[m])
                runs[m].append((dt, cpu))
        out = {}
        for m, rr in runs.items():
            dts, cpus = [a for a, _ in rr], [c for _, c in rr]
            out[m] = {"img_s": round(len(frames) / float(np.median(dts)), 1),
                      "img_s_runs": [round(len(frames) / d, 1) for d in dts],
                      "ms_per_batch": round(float(np.median(dts)) * 1e3 / n_batches, 3),
                      "host_cpu_ms_per_batch": round(float(np.median(cpus)) / n_batches, 3),
                      "host_cpu_ms_per_batch_runs": [round(c / n_batches, 3) for c in cpus]}
        return out

    lines = []
    if "kernel" in args.what:
        devf = [torch.from_numpy(f).to(dev) for f in batches[-1]]             # the largest frames of the mix
        N = len(devf)
        Hc, Wc = max(f.shape[0] for f in devf), max(f.shape[1] for f in devf)
        out = (torch.empty((N, 3, Hc, Wc), device=dev), torch.empty((N, 3, Hc, Wc), device=dev))

        def kernel_ms(cs, lut=None):
            if lut is not None:
                os.environ["RTPE_FRAMES_LAB_LUT"] = str(lut)
            o = out if cs else (out[0], None)
            for _ in range(3):
                pack_frames(devf, cs, out=o)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(args.kernel_iters):
                pack_frames(devf, cs, out=o)
            e1.record()
            torch.cuda.synchronize(dev)
            os.environ.pop("RTPE_FRAMES_LAB_LUT", None)
            return round(e0.elapsed_time(e1) / args.kernel_iters, 4)
        want = [t.clone() for t in pack_frames(devf, "LAB", out=out)[::2]]
        os.environ["RTPE_FRAMES_LAB_LUT"] = "0"
        direct = pack_frames(devf, "LAB")
        os.environ["RTPE_FRAMES_LAB_LUT"] = "1"
        table = pack_frames(devf, "LAB")
        os.environ.pop("RTPE_FRAMES_LAB_LUT")
        same = all(torch.equal(a, c) and torch.equal(a, d) for a, c, d in zip(want, direct[::2], table[::2]))
        ab = {"direct": [], "table": []}
        for form in ("direct", "table", "table", "direct"):
            ab[form].append(kernel_ms("LAB", 0 if form == "direct" else 1))
        px = N * Hc * Wc
        lines.append(dict(common, metric="frames_kernel_ms", frames=N, canvas=[Hc, Wc],
                          note="device frames; the table upload (%d bytes) and the launch are in the interval" % (32 * N),
                          none_ms=kernel_ms(None), hsv_ms=kernel_ms("HSV"), lab_direct_ms_runs=ab["direct"],
                          lab_table_ms_runs=ab["table"], lab_forms_bit_identical=bool(same),
                          lab_store_gb_s_table=round(px * 24 / (min(ab["table"]) * 1e-3) / 1e9, 1)))

    if "frontend" in args.what:
        for lab in (True, False):
            modes = {"A1_host_fp32": a1, "A2_torch_gpu": a2, "B_pack_frames": b}
            first = {m: fn(batches[0], lab) for m, fn in modes.items()}
            exact_a1 = all((u is None and v is None) or torch.equal(u, v)
                           for u, v in zip(first["A1_host_fp32"][::2], first["B_pack_frames"][::2]))
            diff_a2 = [float((u - v).abs().max()) for u, v in zip(first["A2_torch_gpu"][::2], first["B_pack_frames"][::2])
                       if u is not None]
            res = interleave({m: (lambda fn=fn: [fn(fs, lab) for fs in batches]) for m, fn in modes.items()})
            lines.append(dict(common, metric="student_frames_front_end", alt="LAB" if lab else None,
                              B_equals_A1_bit_for_bit=bool(exact_a1), A2_max_abs_difference_from_B=diff_a2,
                              speedup_B_over_A1=round(res["B_pack_frames"]["img_s"] / res["A1_host_fp32"]["img_s"], 2),
                              speedup_B_over_A2=round(res["B_pack_frames"]["img_s"] / res["A2_torch_gpu"]["img_s"], 2), **res))
            del first

    if "pipeline" in args.what:
        for which in ("half", "steps"):
            steps = which == "steps"
            with open(os.path.join(ROOT, "tests", "golden", "student_steps_shapes.json" if steps else "student_shapes.json")) as f:
                shapes = {k: tuple(v) for k, v in json.load(f)["shapes"].items()}
            if steps:
                stu = AttentionStudentSteps(None, "cpu", 48, 17, 1, True, None, False).eval()
                stu.load_state_dict(synth.make_state_dict(shapes, 4, "W1"), strict=True)
            else:
                stu = AttentionStudent(None, "cpu", 100, 17, 1, True, None, False, body_half=True).eval()
                stu.load_state_dict(synth.make_state_dict(shapes, 3, "W1"), strict=True)
            stu = stu.to(dev)
            pipe = engine.StudentPipeline(stu, device=dev, match_on="host")
            cs = "LAB" if steps else None

            def old():
                def packed():
                    for fs in batches:
                        canvas, sz, alt = a2(fs, steps)
                        yield (canvas, sz, alt) if steps else (canvas, sz)
                return list(pipe.stream_mixed(packed()))

            def new():
                return list(pipe.stream_frames(iter(batches), alt_colorspace=cs))
            _, first_old, _ = timed(old)
            _, first_new, _ = timed(new)
            res = interleave({"A2_then_stream_mixed": old, "stream_frames": new})
            lines.append(dict(common, metric="student_frames_end_to_end",
                              model="AttentionStudentSteps(inplanes=48), LAB" if steps
                              else "AttentionStudent(inplanes=100, body_half=True)", weights="W1",
                              first_pass_s={"A2_then_stream_mixed": round(first_old, 2), "stream_frames": round(first_new, 2)},
                              speedup=round(res["stream_frames"]["img_s"] / res["A2_then_stream_mixed"]["img_s"], 3), **res))
            del stu, pipe
            torch.cuda.empty_cache()
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
