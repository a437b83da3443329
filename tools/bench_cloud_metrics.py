#!/usr/bin/env python3
"""Time of one frame's cloud metrics at 375 x 1242 with about 4 % and about 20 % of the pixels carrying ground truth (the densities of the original
and the improved Eigen split): the back-projected prediction against the back-projected ground truth, both on the device.
(a) falnet_nearest per direction, the launches alone by HIP events around single calls into preallocated buffers, and the whole
    cloud_metrics.cloud_errors call (both directions and the sums) the same way;
(b) a chunked torch.cdist(...).min(...) of the same direction on the same GPU, in ALTERNATED pairs with (a): one call of each, REPS times, after
    WARM warm-up pairs; the kernel has to be the faster one in every pair -- the one gate -- and the file says whether it was;
(c) on the host: scipy.spatial.cKDTree where scipy is importable, else the chunked numpy definition (tests/_cloud_ref.py: nearest_ref) on the first
    HOST_QUERIES queries, scaled to the whole set;
(d) the achieved pair rate next to the chip's f32 vector rate (157.3 TFLOP/s with fused multiply-adds; a pair here is 8 roundings that may not fuse,
    a compare and two selects).
The device result is checked against the definition on a sample of queries before anything is timed.
usage: python tools/bench_cloud_metrics.py [--out profiles/cloud_metrics_timing.txt]  (on an MI355X)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cloud_ref as CR  # noqa: E402
import _lidar_ref as LR  # noqa: E402
import _velo_ref as VR  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import cloud_metrics as CM  # noqa: E402
from fal_net_amd import pseudo_lidar  # noqa: E402

H, W, REPS, WARM, HOST_QUERIES, CHECKED, CDIST_CHUNK = 375, 1242, 20, 3, 2048, 512, 8192
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


def cdist_min(q, r, chunk=CDIST_CHUNK):
    """The other formulation: torch.cdist of a chunk of queries against every reference, its row minimum and arg-minimum."""
    d, i = [], []
    for a in range(0, q.shape[0], chunk):
        m = torch.cdist(q[a:a + chunk, :3], r[:, :3]).min(1)
        d.append(m.values), i.append(m.indices)
    return torch.cat(d), torch.cat(i)


def clouds(density, seed):
    """(prediction, ground truth) on the device: a road-like depth with `density` of its pixels kept as the scan, the prediction 3 % off it at those
    pixels (CloudMetrics with on='gt')."""
    rng = np.random.default_rng(seed)
    depth = LR.road_depth(seed, H, W, holes=0.0)
    P, fb = VR.kitti_like_P(), 721.5377 * 0.54
    target = depth.copy()
    target[rng.random((H, W)) >= density] = 0
    disp = (fb / (depth.astype(np.float64) * rng.uniform(0.97, 1.03, (H, W)))).astype(np.float32)
    t, d = torch.from_numpy(target).cuda(), torch.from_numpy(disp).cuda()
    gt = pseudo_lidar.unproject(t, P, max_height=float("inf"))
    pred = pseudo_lidar.unproject(d, P, fb=fb, score=(t > 0).float(), threshold=0.5, max_height=float("inf"))
    return pred, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_metrics_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = L.lib()
    lines = [f"{H} x {W} seeded road-like frames (tests/_lidar_ref.py: road_depth): prediction and ground truth back-projected on the device; milliseconds",
             f"device: {torch.cuda.get_device_name(0)}; HIP events around single calls, {REPS} alternated pairs (kernel, then torch) after {WARM} warm-up pairs; "
             f"query block {CM.QUERY_BLOCK}, reference tile {CM.REF_TILE}, default splits for {CM.TARGET_WORKGROUPS} workgroups"]
    gate = True
    for density in (0.04, 0.20):
        pred, gt = clouds(density, 3)
        lines.append(f"--- {density:.0%} of the pixels carry ground truth: {pred.shape[0]} predicted points, {gt.shape[0]} ground-truth points")
        for name, q, r in (("prediction -> ground truth", pred, gt), ("ground truth -> prediction", gt, pred)):
            nq, nr = int(q.shape[0]), int(r.shape[0])
            d2, idx = CM.nearest(q, r)
            want = CR.nearest_ref(q[:CHECKED].cpu().numpy(), r.cpu().numpy())
            assert np.array_equal(d2[:CHECKED].cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(idx[:CHECKED].cpu().numpy(), want[1]), \
                "the device result differs from the definition: nothing timed"
            td, ti = cdist_min(q, r)
            far = float((td.double() - d2.double().sqrt()).abs().max())
            s = int(lib.falnet_nearest_splits(nq, nr))
            ws = torch.empty(max(int(lib.falnet_nearest_workspace_bytes(nq, nr, 0)) // 8, 1), dtype=torch.int64, device="cuda")
            st = L.stream_ptr()

            def ours():
                L.check(lib.falnet_nearest(L.ptr(q), nq, L.ptr(r), nr, 0, L.ptr(d2), L.ptr(idx), L.ptr(ws), st), "nearest")

            t_ours, t_torch = alternated(ours, lambda: cdist_min(q, r), REPS, WARM)
            wins = sum(x < y for x, y in zip(t_ours, t_torch))
            gate = gate and wins == REPS
            med = sorted(t_ours)[REPS // 2]
            pairs = nq * nr
            lines.append(f"{name}: {nq} x {nr} = {pairs / 1e9:.3f} G pairs, {s} splits; first {CHECKED} queries == nearest_ref bit for bit; "
                         f"torch.cdist's distances within {far:.2e} m of sqrt(d2)")
            lines.append(f"  {'falnet_nearest (fill, kernel, finish)':52s} {stats(t_ours)}")
            lines.append(f"  {'chunked torch.cdist(...).min(1), ' + str(CDIST_CHUNK) + ' queries a chunk':52s} {stats(t_torch)}")
            lines.append(f"  the kernel is the faster one in {wins} of {REPS} alternated pairs; median ratio torch / kernel {sorted(t_torch)[REPS // 2] / med:.2f}")
            lines.append(f"  pair rate {pairs / (med * 1e-3) / 1e12:.3f} T pairs/s = {8 * pairs / (med * 1e-3) / 1e12:.2f} T f32 roundings/s "
                         f"({8 * pairs / (med * 1e-3) / (PEAK_F32 / 2):.1%} of the {PEAK_F32 / 2e12:.1f} T/s of unfused f32 vector operations, "
                         f"{8 * pairs / (med * 1e-3) / PEAK_F32:.1%} of the {PEAK_F32 / 1e12:.1f} TFLOP/s fused peak)")
            qh, rh = q.cpu().numpy(), r.cpu().numpy()
            try:
                from scipy.spatial import cKDTree
                t0 = time.perf_counter()
                cKDTree(rh[:, :3]).query(qh[:, :3])
                lines.append(f"  host: scipy.spatial.cKDTree build + query, wall: {(time.perf_counter() - t0) * 1e3:.1f}")
            except ImportError:
                t0 = time.perf_counter()
                CR.nearest_ref(qh[:HOST_QUERIES], rh)
                dt = (time.perf_counter() - t0) * 1e3
                lines.append(f"  host: chunked numpy definition on the first {min(HOST_QUERIES, nq)} queries, wall: {dt:.1f}; scaled to {nq} queries: {dt * nq / min(HOST_QUERIES, nq):.0f}")
        table = CM.CloudTable(1, CM.THRESHOLDS, "cuda")
        whole, _ = alternated(lambda: CM.cloud_errors(pred, gt, out=table.row(0)), lambda: None, REPS, WARM)
        res = table.result()
        lines.append(f"{'cloud_errors: both directions and the sums, HIP events':54s} {stats(whole)}")
        lines.append(f"  chamfer {res['chamfer'][0]:.4f} m (accuracy {res['accuracy'][0]:.4f}, completeness {res['completeness'][0]:.4f}); F at {list(CM.THRESHOLDS)} m: "
                     + ", ".join(f"{v:.4f}" for v in res["f"][0]))
    lines.append("GATE: the kernel is faster than the chunked torch formulation in every alternated pair at both densities: " + ("yes" if gate else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
