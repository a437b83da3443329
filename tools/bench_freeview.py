#!/usr/bin/env python3
"""Time of the free-viewpoint plane sweep (csrc/med_pose.hip, view + disparity + cover): one launch of 1 pose and one of 8 poses at PURE-BASELINE
poses against falnet_med_sweep_fwd (views + disparities) with the same fractions on the same buffers -- the parent's kernel is the yardstick --
and one launch of 8 poses on an orbit path with yaw.  375 x 1242, N = 49, B = 1 and 256 x 512, N = 49, B = 8.  HIP events around INNER
back-to-back launches, the candidates in alternating order within every round, median (min .. max) over ROUNDS; the buffers (tens of MB) are far
below the 256 MB Infinity Cache, so these are warm-cache figures, stated as such.  Also the achieved rate on the algorithmic bytes
(N + 3 + 5 V) H W 4 per sample.
usage: python tools/bench_freeview.py [out.txt]   (on an MI355X; profiles/freeview_timing.txt)"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import freeview as FV  # noqa: E402

ROUNDS, INNER, WARM = 15, 10, 3
T8 = (-1.0, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0)


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "freeview_timing.txt"), "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
    lib = L.lib()
    emit(f"{torch.cuda.get_device_name(0)}; microseconds per launch, HIP events around {INNER} back-to-back launches, median (min .. max) over {ROUNDS} rounds "
         f"after {WARM} warm-up rounds, candidates alternating within a round; warm caches (working set < Infinity Cache)")
    for B, N, H, W in ((1, 49, 375, 1242), (8, 49, 256, 512)):
        g = torch.Generator().manual_seed(3)
        d0 = (torch.randn(B, N, H, W, generator=g) * 2).cuda()
        left = (torch.rand(B, 3, H, W, generator=g) - 0.43).cuda()
        mx = torch.full((B,), 300.0).cuda()
        mn = mx * 2 / 300
        views, disps, cover = torch.empty(B, 8, 3, H, W, device="cuda"), torch.empty(B, 8, 1, H, W, device="cuda"), torch.empty(B, 8, 1, H, W, device="cuda")
        st = L.stream_ptr()
        K = FV.camera(H, W)

        def sweep(ts):
            t_host = (ctypes.c_float * len(ts))(*ts)
            tp = ctypes.cast(t_host, ctypes.c_void_p)

            def run():
                L.check(lib.falnet_med_sweep_fwd(L.ptr(d0), L.ptr(left), L.ptr(mn), L.ptr(mx), tp, len(ts), L.ptr(views), L.ptr(disps), B, N, H, W, st))
            run.keep = t_host
            return run

        def pose(recs):
            rec = np.ascontiguousarray(np.stack(recs).astype(np.float64))
            rp = rec.ctypes.data_as(ctypes.c_void_p)

            def run():
                L.check(lib.falnet_med_pose_fwd(L.ptr(d0), L.ptr(left), L.ptr(mn), L.ptr(mx), rp, len(rec), L.ptr(views), L.ptr(disps), L.ptr(cover), B, N, H, W, st))
            run.keep = rec
            return run
        base8 = [FV.pose(K, centre=(t, 0.0, 0.0)) for t in T8]
        orbit8 = [FV.pose(K, **kw) for kw in FV.paths.orbit(8, 0.5, 0.25, yaw=3.0)]
        cands = [("pose,  8 pure-baseline poses in [-1, 1]", pose(base8), 8), ("sweep, 8 views in [-1, 1]", sweep(T8), None),
                 ("pose,  1 pure-baseline pose (t = 1)", pose(base8[-1:]), 1), ("sweep, 1 view (t = 1)", sweep((1.0,)), None),
                 ("pose,  8 poses on an orbit (0.5, 0.25) with 3 deg yaw", pose(orbit8), 8)]
        times = {name: [] for name, _, _ in cands}
        for r in range(WARM + ROUNDS):
            order = cands if r % 2 == 0 else cands[::-1]
            for name, fn, _ in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(INNER):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r >= WARM:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / INNER)
        emit(f"B = {B}, N = {N}, {H} x {W}")
        med = {}
        for name, _, nv in cands:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            line = f"  {name:54s} {med[name]:9.1f} ({t[0]:8.1f} .. {t[-1]:8.1f}) us"
            if nv:
                nbytes = (N + 3 + 5 * nv) * H * W * 4 * B
                line += f"   algorithmic {nbytes / 1e6:7.1f} MB -> {nbytes / med[name] / 1e6:6.2f} TB/s"
            emit(line)
        emit(f"  pose / sweep at pure-baseline poses: {med[cands[0][0]] / med[cands[1][0]]:.2f} (8 views), {med[cands[2][0]] / med[cands[3][0]]:.2f} (1 view); "
             f"orbit / pure-baseline, 8 poses: {med[cands[4][0]] / med[cands[0][0]]:.2f}")


if __name__ == "__main__":
    main()
