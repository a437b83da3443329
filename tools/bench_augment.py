#!/usr/bin/env python3
"""Cost of the GPU augmentation per BATCH on KITTI-sized uint8 pairs resident in HBM, to compare with the step time of bench.py:
the per-sample path (data_transforms.StereoAugment in a loop + two torch.stack, as the training script runs it) against the batched
path (data_transforms.BatchAugment: one record-table upload, one launch), in the same process on the same device.

Every batch draws its own parameters (seeded), so the scale factors vary as they do in training and the per-sample path's coefficient
cache misses as it does there.  Both paths get the SAME parameter lists.  Per path and crop: host wall time per batch (perf_counter
around the issuing loop, device idle at its start, not synchronised at its end: what the step's host thread pays) and device time per
batch (HIP events around the same loop, which ends with the last kernel).  Warm-up batches first, then `--repeats` windows of
`--batches` batches, the two paths alternating window by window; the median and the range over the windows are reported.

usage: python tools/bench_augment.py [--batch 8] [--batches 40] [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fal_net_amd import data_transforms as DT  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--batches", type=int, default=40, help="batches per timed window")
ap.add_argument("--repeats", type=int, default=7, help="timed windows per path")
ap.add_argument("--warmup", type=int, default=10, help="untimed batches per path")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_augment.py measures on the GPU: none found (no fallback)")
dev = torch.device("cuda", 0)
H, W, B = 375, 1242, args.batch
g = torch.Generator().manual_seed(0)
frames = [[torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(2)] for _ in range(2 * B)]
lines = [f"augmentation per batch: B = {B}, source frames {H} x {W} uint8 in HBM, {args.repeats} windows of {args.batches} batches per path "
         f"after {args.warmup} warm-up batches, paths alternating; device: {torch.cuda.get_device_name(0)}"]
results = []


def window(fn, batches):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for pairs, params in batches:
        fn(pairs, params)
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return host / len(batches) * 1e3, e0.elapsed_time(e1) / len(batches)


for th, tw in ((256, 512), (192, 640)):
    single, batched = DT.StereoAugment(th, tw), DT.BatchAugment(th, tw)
    random.seed(th)
    np.random.seed(th)
    n = args.warmup + args.batches
    work = []
    for k in range(n):  # every batch its own seeded draws: varying scale factors
        pairs = [frames[(k * B + b) % len(frames)] for b in range(B)]
        work.append((pairs, [batched.draw(H, W) for _ in range(B)]))

    def per_sample(pairs, params):
        views = [single(p, params=q) for p, q in zip(pairs, params)]
        return torch.stack([v[0] for v in views]), torch.stack([v[1] for v in views])

    def one_call(pairs, params):
        return batched(pairs, params=params)

    a, b = per_sample(*work[0]), one_call(*work[0])
    same = all(float((x - y).abs().max()) <= 2e-6 for x, y in zip(a, b))
    paths = {"per-sample": per_sample, "batched": one_call}
    times = {k: [] for k in paths}
    for name, fn in paths.items():
        window(fn, work[:args.warmup])
    for _ in range(args.repeats):
        for name, fn in paths.items():
            DT._COEFF_CACHE.clear()  # a training run meets new sizes all the time: no window starts with the previous window's tables
            times[name].append(window(fn, work[args.warmup:]))
    rec = {"crop": [th, tw], "batch": B, "outputs_agree": same}
    for name in paths:
        host, devt = [t[0] for t in times[name]], [t[1] for t in times[name]]
        rec[name] = {"host_ms": statistics.median(host), "host_ms_range": [min(host), max(host)],
                     "device_ms": statistics.median(devt), "device_ms_range": [min(devt), max(devt)]}
        lines.append(f"crop {th} x {tw}  {name:10s}: host {statistics.median(host):7.3f} ms/batch [{min(host):.3f} .. {max(host):.3f}]   "
                     f"device {statistics.median(devt):7.3f} ms/batch [{min(devt):.3f} .. {max(devt):.3f}]   "
                     f"{B / statistics.median(devt) * 1e3:8.0f} pairs/s by the device clock")
    rec["host_ratio"] = rec["per-sample"]["host_ms"] / rec["batched"]["host_ms"]
    rec["device_ratio"] = rec["per-sample"]["device_ms"] / rec["batched"]["device_ms"]
    lines.append(f"crop {th} x {tw}  per-sample / batched: host x{rec['host_ratio']:.2f}, device x{rec['device_ratio']:.2f}; outputs agree within 2e-6: {same}")
    results.append(rec)

report = "\n".join(lines) + "\n" + json.dumps({"augment_batch": results}) + "\n"
print(report, end="")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(report)
