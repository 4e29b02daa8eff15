"""Keypoint scoring by two paths, in one process (5,000 synthetic images with 0-30 people and 0-20 annotations each):

  (a) device   ``rtpe.scoring.score_records``: the record tensor already on the GPU, one launch of the scoring kernel,
               one read-back of the result table, the accumulation in numpy;
  (b) host     the float64 restatement of the same rules (tests/scoring_restated.py: plain numpy with Python loops,
               written for reading, not for speed) on the unpacked records.

Everything is warmed up first (the annotation table is uploaded once, as ``CocoKeypointGT.to`` caches it), then the two
paths alternate A B B A (--repeats rounds).  Reports the median seconds per path, the kernel's own time (device events
around the launch) and whether the two paths give the same ten numbers.  No threshold: the figures are for comparing.
Prints one JSON line and writes it to --out.  Needs a GPU; there is no fallback.

    python tools/oks_bench.py [--images 5000] [--repeats 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "realtime-pose-estimation_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def workload(n_images, seed=0):
    """``(dt, gt, ids)``: per image 0-20 annotations (random poses of random size, some crowds, some joints not
    labelled) and 0-30 people - noisy copies of the annotations first, random poses after them"""
    rng = np.random.default_rng(seed)
    dt, gt = {}, {}
    for i in range(1, n_images + 1):
        anns, people = [], []
        for _ in range(int(rng.integers(0, 21))):
            size = rng.uniform(20, 300)
            p = rng.uniform(0, 640, 2)[None, :] + rng.uniform(-size / 2, size / 2, (17, 2))
            v = rng.integers(0, 3, 17)
            crowd = int(rng.random() < 0.05)
            kp = np.concatenate([p * (v[:, None] > 0), v[:, None]], 1)
            area = float(size * size * rng.uniform(0.3, 0.6))
            anns.append({"keypoints": kp.reshape(-1).tolist(), "area": area, "iscrowd": crowd,
                         "bbox": [float(p[:, 0].min()), float(p[:, 1].min()), float(np.ptp(p[:, 0])), float(np.ptp(p[:, 1]))],
                         "num_keypoints": 0 if crowd else int((v > 0).sum()), "category_id": 1})
            people.append(p + rng.normal(0, rng.uniform(0.02, 0.3) * np.sqrt(area) * 0.1, (17, 2)))
        n = int(rng.integers(0, 31))
        while len(people) < n:
            size = rng.uniform(20, 300)
            people.append(rng.uniform(0, 640, 2)[None, :] + rng.uniform(-size / 2, size / 2, (17, 2)))
        order = rng.permutation(len(people))[:n]
        kpts = np.zeros((n, 17, 4), np.float32)
        for k, o in enumerate(order):
            kpts[k, :, :2] = people[o]
        kpts[:, :, 2] = rng.random((n, 17))
        gt[i] = anns
        dt[i] = (kpts, rng.random(n).astype(np.float32))
    return dt, gt, list(gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=1, help="rounds of A B B A")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "oks_eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("oks_bench: no GPU (the scoring kernel runs on the HIP path only)")
    import __graft_entry__ as entry
    entry.build()
    import scoring_restated as SR
    from rtpe import engine, scoring
    dev = torch.device("cuda:0")
    dt, gt, ids = workload(args.images)
    images = [{"id": i} for i in ids]
    anns = [dict(a, image_id=i) for i in ids for a in gt[i]]
    g = scoring.CocoKeypointGT({"images": images, "annotations": anns})
    rec = engine.pack_records(ids, [dt[i] for i in ids], dev)
    print("oks_bench: %d images, %d people, %d annotations" % (len(ids), sum(len(s) for _, s in dt.values()), len(anns)),
          flush=True)

    def device_path():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = scoring.score_records(rec, g)
        return time.perf_counter() - t0, out

    def host_path():
        t0 = time.perf_counter()
        out = SR.score(engine.unpack_records(rec), gt, ids)
        return time.perf_counter() - t0, out

    device_path()                                       # warm-up: the table's upload, the kernel's first launch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kernel_ms = []
    for _ in range(5):
        ev[0].record()
        scoring._launch(rec, g)
        ev[1].record()
        torch.cuda.synchronize(dev)
        kernel_ms.append(ev[0].elapsed_time(ev[1]))
    runs = {"device": [], "host": []}
    stats = {}
    for r in range(args.repeats):
        for key in ("device", "host", "host", "device"):
            sec, stats[key] = (device_path if key == "device" else host_path)()
            runs[key].append(round(sec, 4))
            print("oks_bench: %s %.3f s" % (key, sec), flush=True)
    out = {"metric": "oks_eval_seconds", "images": len(ids), "people": int(sum(len(s) for _, s in dt.values())),
           "annotations": len(anns), "device": torch.cuda.get_device_name(dev), "order": "A B B A over device, host",
           "repeats": args.repeats,
           "device_s": round(float(np.median(runs["device"])), 4), "device_s_runs": runs["device"],
           "host_restatement_s": round(float(np.median(runs["host"])), 3), "host_restatement_s_runs": runs["host"],
           "kernel_ms": round(float(np.median(kernel_ms)), 3), "kernel_ms_runs": [round(v, 3) for v in kernel_ms],
           "same_statistics": stats["device"] == stats["host"],
           "max_abs_difference": max(abs(stats["device"][k] - stats["host"][k]) for k in stats["host"]),
           "statistics": stats["device"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
