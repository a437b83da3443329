#!/usr/bin/env python3
"""Time of one frame's pseudo-LiDAR scan: a 375 x 1242 disparity map back-projected into Velodyne-format records,
(a) on the device (fal_net_amd/pseudo_lidar.py: unproject) in dense mode and with 64 beams x 1024 azimuth bins: the launches of
    falnet_velo_unproject alone by HIP events around single calls into preallocated buffers, REPS repetitions alternating between two maps after
    WARM warm-up calls, and the whole wrapper (tables, workspace, the one count read) by wall clock;
(b) on the host: the element-wise numpy definition (tests/_lidar_ref.py: unproject_ref), wall clock, on the same box;
(c) the HBM floor of each mode at 8 TB/s: the bytes that must move at least once.
The device scans are checked against the definition before anything is timed.  Nothing on the parent commit does this job, so there is no ratio to
hold: the figures are recorded.  usage: python tools/bench_pseudo_lidar.py [--out profiles/pseudo_lidar_timing.txt]  (on an MI355X)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _lidar_ref as LR  # noqa: E402
import _velo_ref as R  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import pseudo_lidar, velodyne  # noqa: E402

H, W, REPS, WARM, HOST_REPS = 375, 1242, 200, 20, 5
HBM = 8e12  # bytes per second
MODES = (("dense", 0, 1024), ("64 beams x 1024 bins", 64, 1024))


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:9.4f}   min {ms[0]:9.4f}   max {ms[-1]:9.4f}"


def event_times(calls, reps, warm):
    for i in range(warm):
        calls[i % len(calls)]()
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (e0, e1) in enumerate(pairs):
        e0.record()
        calls[i % len(calls)]()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in pairs]


def wall_times(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudo_lidar_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = L.lib()
    P, fb = R.kitti_like_P(), 721.5377 * 0.54
    q12 = (C.c_double * 12)(*velodyne.backprojection_matrix(P).reshape(-1).tolist())
    disps = []
    for seed in (3, 4):
        depth = LR.road_depth(seed, H, W)
        with np.errstate(divide="ignore"):
            disps.append(np.where(depth > 0, fb / depth.astype(np.float64), 0.0).astype(np.float32))
    dev = [torch.from_numpy(d).cuda() for d in disps]
    lines = [f"{H} x {W} seeded road-like disparity maps (tests/_lidar_ref.py: road_depth, seeds 3 and 4, 5 % holes) -> Velodyne-format records; milliseconds",
             f"device: {torch.cuda.get_device_name(0)}; launch figures over {REPS} calls alternating between the two maps after {WARM} warm-up calls; "
             f"wrapper and host figures over {HOST_REPS} calls after one"]
    for name, beams, az in MODES:
        kw = dict(fb=fb, beams=beams, az_bins=az)
        kept = []
        for d_host, d in zip(disps, dev):
            want = LR.unproject_ref(d_host, P, **kw)
            got = pseudo_lidar.unproject(d, P, **kw).cpu().numpy()
            assert got.tobytes() == want.tobytes(), "the device scan differs from the definition: nothing timed"
            kept.append(len(want))
        in_range = len(LR.unproject_ref(disps[0], P, fb=fb))
        lines.append(f"--- {name}: checked, device scan == unproject_ref byte for byte, {kept[0]} and {kept[1]} points")
        cap = H * W if beams == 0 else beams * az
        outs = [torch.empty((cap, 4), device="cuda") for _ in dev]
        counts = [torch.empty(1, dtype=torch.int64, device="cuda") for _ in dev]
        ws = torch.empty(int(lib.falnet_lidar_workspace_bytes(H, W, beams, az)) // 8, dtype=torch.int64, device="cuda")
        te = ta = None
        if beams:
            te, ta = (torch.from_numpy(t).cuda() for t in pseudo_lidar.edge_tables(beams, az))
        st = L.stream_ptr()

        def launch(d, o, c):
            L.check(lib.falnet_velo_unproject(L.ptr(d), fb, None, 0.0, None, 1.0, q12, 0.0, 80.0, 1.0, H, W, beams, az, L.ptr(te), L.ptr(ta), L.ptr(o), cap, L.ptr(c),
                                              L.ptr(ws), st), "velo_unproject")

        each = event_times([lambda d=d, o=o, c=c: launch(d, o, c) for d, o, c in zip(dev, outs, counts)], REPS, WARM)
        # bytes that must move: the map read once per pass over the pixels, the records written once, the key table filled, updated and read
        n_pix = H * W
        if beams == 0:
            moved, floor = 2 * 4 * n_pix + 16 * kept[0], 4 * n_pix + 16 * kept[0]
            what = "map read by the count and the scatter pass, records written"
        else:
            bins = beams * az
            moved, floor = 4 * n_pix + 8 * bins + 8 * in_range + 2 * 8 * bins + 4 * kept[0] + 16 * kept[0], 4 * n_pix + 16 * kept[0]
            what = "map read, key table filled, one 8-byte atomic per in-range pixel, table read twice, winners' pixels re-read, records written"
        med = sorted(each)[len(each) // 2]
        lines.append(f"{'launches of falnet_velo_unproject, HIP events per call':58s} {stats(each)}")
        lines.append(f"{'bytes moved (' + what + ')':58s} {moved / 1e6:9.3f} MB -> {moved / HBM * 1e3:9.5f} ms at 8 TB/s; the call takes {med / (moved / HBM * 1e3):6.1f} x that")
        lines.append(f"{'HBM floor (map once, records once)':58s} {floor / 1e6:9.3f} MB -> {floor / HBM * 1e3:9.5f} ms at 8 TB/s; the call takes {med / (floor / HBM * 1e3):6.1f} x that")
        lines.append(f"{'pseudo_lidar.unproject (tables, workspace, count read), wall':58s} {stats(wall_times(lambda: pseudo_lidar.unproject(dev[0], P, **kw), HOST_REPS))}")
        lines.append(f"{'host: unproject_ref (element-wise float64 numpy)':58s} {stats(wall_times(lambda: LR.unproject_ref(disps[0], P, **kw), HOST_REPS))}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
