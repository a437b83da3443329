#!/usr/bin/env python3
"""Time per 375 x 1242 frame of the evaluation metrics: (a) the HOST chain as inference.evaluate / train.validate run it per frame (two full-size
copies, myUtils.disps_to_depths_* + compute_kitti_errors in float64 numpy, realEPE, get_rmse with a float()) and (b) the DEVICE path
(fal_net_amd/metrics.py into a MetricTable row, no host read per frame; the table is read once at the end, inside the timed region), on the same
box and the same seeded frames.  Wall clock per frame of a loop over FRAMES frames ending in a synchronise, and -- device path -- HIP events around
the same loop.  usage: python tools/bench_metrics.py  (on an MI355X; profiles/metrics_timing.txt)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from fal_net_amd import metrics as M  # noqa: E402
from fal_net_amd import myUtils as utils  # noqa: E402
from fal_net_amd.loss_functions import realEPE  # noqa: E402

H, W, FRAMES, REPS, WARM = 375, 1242, 20, 5, 2


def frames(mode):
    out = []
    for k in range(FRAMES):
        rng = np.random.default_rng(100 + k)
        pred = (rng.random((H, W)) ** 2 * 90 + 0.5).astype(np.float32)
        noisy = np.maximum(pred.astype(np.float64) * (1 + 0.15 * rng.standard_normal((H, W))), 0.05)
        gt = (noisy if mode == "kitti2015" else M.focal_baseline(mode, W) / noisy).astype(np.float32)
        gt[rng.random((H, W)) >= 0.3] = 0
        out.append((torch.from_numpy(pred).cuda().view(1, 1, H, W), torch.from_numpy(gt).cuda().view(1, 1, H, W)))
    return out


def timed(loop):
    """median / min / max over REPS of (wall ms per frame, event ms per frame) of one pass over the frames"""
    for _ in range(WARM):
        loop()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        loop()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / FRAMES)
        dev.append(e0.elapsed_time(e1) / FRAMES)
    wall.sort(), dev.sort()
    return (wall[len(wall) // 2], wall[0], wall[-1]), (dev[len(dev) // 2], dev[0], dev[-1])


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    print(f"{H} x {W} frames, {FRAMES} per pass; median (min .. max) over {REPS} passes after {WARM} warm-up passes; milliseconds PER FRAME")
    print(f"{'what':46s} {'host chain, wall':>26s} {'device path, wall':>26s} {'device path, HIP events':>26s}")
    fmt = lambda t: f"{t[0]:8.3f} ({t[1]:7.3f} ..{t[2]:8.3f})"
    slower = []
    for mode, median, with_epe in (("kitti2015", False, True), ("kitti2015", True, True), ("eigen", False, False), ("eigen", True, False)):
        fr = frames(mode)

        def host():
            for disp, target in fr:
                t_np, p_np = target.squeeze(1).cpu().numpy(), disp.float().squeeze(1).cpu().numpy()
                if with_epe:
                    float(realEPE(disp, target, sparse=True))
                gd, pd = (utils.disps_to_depths_kitti2015 if mode == "kitti2015" else utils.disps_to_depths_kitti)(t_np, p_np)
                utils.compute_kitti_errors(gd[0], pd[0], use_median=median)

        def device():
            table = M.MetricTable(FRAMES)
            for i, (disp, target) in enumerate(fr):
                row = table.row(i)
                if with_epe:
                    M.epe(disp, target, True, out=row)
                M.depth_errors(disp, target, mode, use_median=median, out=row)
            table.result()

        h, d = timed(host), timed(device)
        name = f"{mode}{' -median' if median else ''}: depth errors{' + EPE' if with_epe else ''}"
        print(f"{name:46s} {fmt(h[0])} {fmt(d[0])} {fmt(d[1])}")
        if d[0][0] > h[0][0]:
            slower.append(name)
    rng = np.random.default_rng(9)
    views = [(torch.from_numpy((rng.random((1, 3, H, W)) - 0.4).astype(np.float32)).cuda(), torch.from_numpy((rng.random((1, 3, H, W)) - 0.4).astype(np.float32)).cuda())
             for _ in range(FRAMES)]

    def host_view():
        for a, b in views:
            float(utils.get_rmse(a, b))

    def device_view():
        table = M.MetricTable(FRAMES)
        for i, (a, b) in enumerate(views):
            M.view_errors(a, b, out=table.row(i))
        table.result()

    h, d = timed(host_view), timed(device_view)
    name = "validate: view RMSE (get_rmse + float())"
    print(f"{name:46s} {fmt(h[0])} {fmt(d[0])} {fmt(d[1])}")
    if d[0][0] > h[0][0]:
        slower.append(name)
    print("device path slower than the host chain per frame: " + (", ".join(slower) if slower else "none"))


if __name__ == "__main__":
    main()
