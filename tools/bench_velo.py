#!/usr/bin/env python3
"""Time of the original Eigen split's ground truth for one frame: a 120 000-point Velodyne scan into a 375 x 1242 depth map,
(a) on the device (fal_net_amd/velodyne.py: project -- fill, scatter and finish launches) by HIP events around single calls, REPS repetitions
    alternating between two scans and two output maps, and by events around the whole loop; the upload of the scan (pinned and pageable host
    memory) separately, the same way;
(b) on the host: Monodepth's original formulation (tests/_velo_ref.py: monodepth_host) and the element-wise numpy definition (spec), wall clock.
The device maps are checked against `spec` before anything is timed.  Nothing on the parent commit does this job, so there is no ratio to hold:
the figures are recorded.  usage: python tools/bench_velo.py [--out profiles/velo_project_timing.txt]  (on an MI355X)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _velo_ref as R  # noqa: E402
from fal_net_amd import velodyne  # noqa: E402

H, W, N_POINTS, REPS, WARM, HOST_REPS = 375, 1242, 120000, 200, 20, 5


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:9.4f}   min {ms[0]:9.4f}   max {ms[-1]:9.4f}"


def event_times(calls, reps, warm):
    """per-call milliseconds by HIP events, calls[i % len(calls)] in turn; and milliseconds per call of the whole loop"""
    for i in range(warm):
        calls[i % len(calls)]()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (e0, e1) in enumerate(pairs):
        e0.record()
        calls[i % len(calls)]()
        e1.record()
    torch.cuda.synchronize()
    each = [e0.elapsed_time(e1) for e0, e1 in pairs]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(reps):
        calls[i % len(calls)]()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    return each, e0.elapsed_time(e1) / reps, wall


def host_times(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "velo_project_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    P = R.kitti_like_P()
    scans = [R.seeded_scan(s, N_POINTS) for s in (0, 2)]
    dev = [torch.from_numpy(s).cuda() for s in scans]
    outs = [torch.empty((H, W), device="cuda") for _ in scans]
    lines = [f"{N_POINTS}-point seeded scans (tests/_velo_ref.py: seeded_scan, seeds 0 and 2) -> {H} x {W} f32 depth map; milliseconds",
             f"device: {torch.cuda.get_device_name(0)}; device figures over {REPS} calls alternating between the two scans after {WARM} warm-up calls; "
             f"host figures over {HOST_REPS} calls after one"]
    for s, d, o in zip(scans, dev, outs):
        want = R.spec(P, s, H, W)
        got = velodyne.project(d, P, H, W, out=o).cpu().numpy()
        assert np.array_equal(got, want), "the device map differs from the definition: nothing timed"
        lines.append(f"checked: device map == spec bit for bit, {int((want > 0).sum())} pixels set")
    calls = [lambda d=d, o=o: velodyne.project(d, P, H, W, out=o) for d, o in zip(dev, outs)]
    each, loop_ev, loop_wall = event_times(calls, REPS, WARM)
    lines.append(f"{'device projection, HIP events per call':58s} {stats(each)}")
    lines.append(f"{'device projection, HIP events around the loop, per call':58s} {loop_ev:16.4f}")
    lines.append(f"{'device projection, wall clock of the loop, per call':58s} {loop_wall:16.4f}")
    pinned = [torch.from_numpy(s).pin_memory() for s in scans]
    pageable = [torch.from_numpy(s) for s in scans]
    for name, src in (("pinned", pinned), ("pageable", pageable)):
        ups = [lambda h=h, d=d: d.copy_(h, non_blocking=True) for h, d in zip(src, dev)]
        each, loop_ev, _ = event_times(ups, REPS, WARM)
        lines.append(f"{'upload of the scan (1.92 MB), ' + name + ', HIP events per call':58s} {stats(each)}")
    lines.append(f"{'host: monodepth_host (np.dot + Counter loop)':58s} {stats(host_times(lambda: R.monodepth_host(P, scans[0], H, W), HOST_REPS))}")
    lines.append(f"{'host: spec (element-wise float64 numpy + np.minimum.at)':58s} {stats(host_times(lambda: R.spec(P, scans[0], H, W), HOST_REPS))}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
