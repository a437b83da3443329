#!/usr/bin/env python3
"""Time of the ground-plane kernels (fal_net_amd/ground.py, csrc/ground.hip) on seeded road clouds of n = 32 768 and n = 262 144 points -- the second
is a dense 375 x 1242 frame after the depth cut -- with H = 512 and H = 1 024 hypotheses.
(a) falnet_ground_consensus (fill, kernel, select), falnet_ground_moments (both launches), falnet_ground_heights and falnet_ground_split (count, scan,
    scatter): the launches alone by HIP events around single calls into preallocated buffers;
(b) the same definition of the consensus as torch operations on the same GPU -- a chunked (n, 3) @ (3, H), compare, sum -- in ALTERNATED pairs with
    (a): one call of each, REPS times, after WARM warm-up pairs; the file says which was the faster one in how many pairs, whichever it is;
(c) the numpy reference (tests/_ground_ref.py: consensus_ref) on the host, on the first HOST_HYPOTHESES hypotheses, scaled to all;
(d) the implied pair rate next to the chip's f32 vector rate (157.3 TFLOP/s with fused multiply-adds; a pair here is 5 roundings that may not fuse,
    an absolute value, a compare and an integer add).
The device counts are checked against the definition on a sample of hypotheses before anything is timed.  The kernel is untuned: its decomposition is
the first one written, and no counter run was made.
usage: python tools/bench_ground.py [--out profiles/ground_timing.txt]  (on an MI355X)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _ground_ref as GR  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import ground as G  # noqa: E402

REPS, WARM, HOST_HYPOTHESES, CHECKED, TORCH_CHUNK, TOL = 20, 3, 16, 32, 65536, 0.15
PEAK_F32 = 157.3e12  # FLOP/s, vector f32 with fused multiply-adds


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:9.4f}   min {ms[0]:9.4f}   max {ms[-1]:9.4f}"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def alternated(a, b, reps, warm):
    """reps pairs (a, then b) after warm pairs -> two lists of milliseconds, pair i at index i of both."""
    for _ in range(warm):
        a(), b()
    torch.cuda.synchronize()
    ev = [(timed(a), timed(b)) for _ in range(reps)]
    torch.cuda.synchronize()
    return [x[0].elapsed_time(x[1]) for x, _ in ev], [y[0].elapsed_time(y[1]) for _, y in ev]


def torch_consensus(pts, planes, tol, chunk=TORCH_CHUNK):
    """The other formulation: e = z - ((x, y, 1) @ (p, q, r)) for a chunk of points against every plane as one matrix product, compare, sum.  The
    product's order of operations is the library's, so a count may differ from the definition's where a residual sits within rounding of tol."""
    A = torch.stack([planes[:, 0], planes[:, 1], planes[:, 2]], 0)  # (3, H)
    valid = planes[:, 3] != 0
    counts = torch.zeros(planes.shape[0], dtype=torch.int64, device=pts.device)
    ones = torch.ones(pts.shape[0], 1, device=pts.device)
    xy1 = torch.cat([pts[:, :2], ones], 1)
    for a in range(0, pts.shape[0], chunk):
        e = pts[a:a + chunk, 2:3] - xy1[a:a + chunk] @ A
        counts += (e.abs() <= tol).sum(0)
    return counts * valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = L.lib()
    lines = ["seeded road clouds (tests/_ground_ref.py: road_cloud); milliseconds",
             f"device: {torch.cuda.get_device_name(0)}; HIP events around single calls, {REPS} alternated pairs (kernel, then torch) after {WARM} warm-up pairs; "
             f"hypothesis block {G.HYP_BLOCK}, point tile {G.POINT_TILE}, default splits for {G.TARGET_WORKGROUPS} workgroups; the kernel is untuned"]
    wins_all, pairs_all = 0, 0
    for n in (32768, 262144):
        pts_h = GR.road_cloud(n, seed=31)
        pts = torch.from_numpy(pts_h).cuda()
        for H in (512, 1024):
            tr = G.triples(0, H, n)
            planes = G.hypotheses(pts, tr)
            want_planes = GR.hypotheses_ref(pts_h, tr)
            assert np.array_equal(planes.cpu().numpy().view(np.uint32), want_planes.view(np.uint32)), "the planes differ from the definition: nothing timed"
            counts, best = G.consensus(pts, planes, TOL)
            want = GR.consensus_ref(pts_h, want_planes[:CHECKED], TOL)[0]
            assert np.array_equal(counts[:CHECKED].cpu().numpy(), want), "the counts differ from the definition: nothing timed"
            tc = torch_consensus(pts, planes, TOL)
            off = int((tc - counts.long()).abs().max())
            s = int(lib.falnet_ground_splits(n, H))
            ws = torch.empty(max(int(lib.falnet_ground_consensus_workspace_bytes(n, H, 0)) // 8, 1), dtype=torch.int64, device="cuda")
            st = L.stream_ptr()

            def ours():
                L.check(lib.falnet_ground_consensus(L.ptr(pts), n, L.ptr(planes), H, TOL, 0, L.ptr(counts), L.ptr(best), L.ptr(ws), st), "ground_consensus")

            t_ours, t_torch = alternated(ours, lambda: torch_consensus(pts, planes, TOL), REPS, WARM)
            wins = sum(x < y for x, y in zip(t_ours, t_torch))
            wins_all, pairs_all = wins_all + wins, pairs_all + REPS
            med = sorted(t_ours)[REPS // 2]
            pairs = n * H
            lines.append(f"--- consensus: n = {n} points x H = {H} hypotheses = {pairs / 1e9:.3f} G pairs, {s} splits, {int((want_planes[:, 3] != 0).sum())} valid; "
                         f"first {CHECKED} counts == consensus_ref; the torch form's counts differ from the kernel's by at most {off}")
            lines.append(f"  {'falnet_ground_consensus (fill, kernel, select)':60s} {stats(t_ours)}")
            lines.append(f"  {'chunked (n, 3) @ (3, H), compare, sum; ' + str(TORCH_CHUNK) + ' points a chunk':60s} {stats(t_torch)}")
            lines.append(f"  the kernel is the faster one in {wins} of {REPS} alternated pairs; median ratio torch / kernel {sorted(t_torch)[REPS // 2] / med:.2f}")
            lines.append(f"  pair rate {pairs / (med * 1e-3) / 1e12:.3f} T pairs/s = {5 * pairs / (med * 1e-3) / 1e12:.2f} T f32 roundings/s "
                         f"({5 * pairs / (med * 1e-3) / (PEAK_F32 / 2):.1%} of the {PEAK_F32 / 2e12:.1f} T/s of unfused f32 vector operations, "
                         f"{5 * pairs / (med * 1e-3) / PEAK_F32:.1%} of the {PEAK_F32 / 1e12:.1f} TFLOP/s fused peak)")
            t0 = time.perf_counter()
            GR.consensus_ref(pts_h, want_planes[:HOST_HYPOTHESES], TOL)
            dt = (time.perf_counter() - t0) * 1e3
            lines.append(f"  host: numpy definition on the first {HOST_HYPOTHESES} hypotheses, wall: {dt:.1f}; scaled to {H}: {dt * H / HOST_HYPOTHESES:.0f}")
        # the rest of a fit at this n: moments of the winner's inliers, heights, split
        row = torch.empty(G.ROW, dtype=torch.float64, device="cuda")
        mws = torch.empty(int(lib.falnet_ground_moments_workspace_bytes()) // 8, dtype=torch.int64, device="cuda")
        t_mom, _ = alternated(lambda: G.moments(pts, TOL, best=best, out=row, workspace=mws), lambda: None, REPS, WARM)
        plane = G.solve(row.cpu().numpy())
        hts = torch.empty(n, dtype=torch.float32, device="cuda")
        t_h, _ = alternated(lambda: G.heights(pts, plane, out=hts), lambda: None, REPS, WARM)
        p, q, r, cz = G.plane_f32(plane)
        out, cnt = torch.empty(n, 4, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
        sws = torch.empty(int(lib.falnet_ground_split_workspace_bytes(n)) // 8, dtype=torch.int64, device="cuda")

        def split():
            L.check(lib.falnet_ground_split(L.ptr(pts), n, p, q, r, cz, float("-inf"), 0.2, 0, L.ptr(out), n, L.ptr(cnt), L.ptr(sws), st), "ground_split")

        t_s, _ = alternated(split, lambda: None, REPS, WARM)
        lines.append(f"--- n = {n}: the refit's plane p {plane.p:+.5f} q {plane.q:+.5f} r {plane.r:+.4f}, sensor height {plane.sensor_height:.4f} m, "
                     f"{plane.inliers} inliers, {int(cnt.item())} points above 0.2 m")
        lines.append(f"  {'ground.moments (two launches), through Python':60s} {stats(t_mom)}")
        lines.append(f"  {'ground.heights, through Python':60s} {stats(t_h)}")
        lines.append(f"  {'falnet_ground_split (count, scan, scatter)':60s} {stats(t_s)}")
        t0 = time.perf_counter()
        fit = G.fit(pts, tol=TOL)
        torch.cuda.synchronize()
        lines.append(f"  ground.fit, H = 512, 2 refits, wall with its two reads: {(time.perf_counter() - t0) * 1e3:.3f}; sensor height {fit.sensor_height:.4f} m")
    lines.append(f"the kernel was the faster one in {wins_all} of {pairs_all} alternated pairs against the torch form over all four shapes")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
