#!/usr/bin/env python3
"""Wall time per 375 x 1242 frame of the test-time outputs (fal_net_amd/dumps.py): (a) the device path up to a finished HOST buffer (kernel +
copy of the result, synchronised) and (b) the host restatement the tests compare against (copy of the f32 maps + numpy / torch-CPU), then
Test_KITTI.py --synthetic with and without --device-percentile.  usage: python tools/bench_dumps.py  (on an MI355X; profiles/dumps_timing.txt)"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from fal_net_amd import dumps  # noqa: E402

H, W, REPS, WARM = 375, 1242, 30, 5
MEAN = np.array(dumps.MEAN, np.float32)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    rng = np.random.default_rng(0)
    disp = torch.from_numpy((rng.random((1, 1, H, W)) ** 3 * 120).astype(np.float32)).cuda()
    img = torch.from_numpy((rng.random((1, 3, H, W)) - 0.43).astype(np.float32)).cuda()
    lut = dumps.plasma_lut()
    focal, baseline = dumps.camera_for_width(W)

    def host_plasma():
        d = disp.squeeze().cpu().numpy()
        v = 256 * np.clip(d / (np.percentile(d, 95) + 1e-6), 0, 1)
        return lut[np.minimum(np.rint(v), 255).astype(np.int64)]

    def host_image():
        return np.rint(255 * (img.squeeze().cpu().numpy() + MEAN[:, None, None]).transpose(1, 2, 0)).clip(0, 255).astype(np.uint8)

    def host_feature():
        return np.rint(np.clip(255 * np.abs(img.cpu().numpy()), 0, 255)).astype(np.uint8)

    def host_local_norm():
        x = img.cpu() + torch.tensor(MEAN).view(1, 3, 1, 1)
        m = F.avg_pool2d(x, 3, 1, 1)
        return (x - m) / (F.avg_pool2d((x - m) ** 2, 3, 1, 1) ** 0.5 + 1e-7)

    def host_point_cloud():
        d, im = disp.cpu().numpy(), img.cpu().numpy()
        z = np.float32(focal * baseline) / (d + np.float32(1e-4))
        u = (np.arange(W, dtype=np.float32) + 0.5).reshape(1, 1, 1, W)
        v = (np.arange(H, dtype=np.float32) + 0.5).reshape(1, 1, H, 1)
        x, y = (u - W / 2) / np.float32(focal) * z, (v - H / 2) / np.float32(focal) * z
        return np.concatenate([x, np.clip(z, 0, 200), -y, (im + MEAN.reshape(1, 3, 1, 1)) * 255], 1).reshape(1, 6, H * W)

    rows = [
        ("percentile q=95 (value on the host)", lambda: dumps.percentile(disp, 95).cpu(), lambda: np.percentile(disp.cpu().numpy(), 95)),
        ("disparity RGBA (percentile + plasma)", lambda: dumps.disparity_png(disp).cpu(), host_plasma),
        ("image u8 (3 ch)", lambda: dumps.image_u8(img).cpu(), host_image),
        ("feature u8 (3 ch)", lambda: dumps.feature_u8(img).cpu(), host_feature),
        ("local normalisation (3 ch, f32)", lambda: dumps.local_normalization(img).cpu(), host_local_norm),
        ("point cloud planar (6 x HW f32)", lambda: dumps.point_cloud(img, disp).cpu(), host_point_cloud),
        ("point cloud packed (HW x 15 B)", lambda: dumps.point_cloud(img, disp, packed=True).cpu(), lambda: dumps.pack_vertices(host_point_cloud()[0])),
    ]
    print(f"{H} x {W} frame, median (min .. max) of {REPS} synchronised calls after {WARM} warm-up calls, milliseconds of wall time")
    print(f"{'output':40s} {'device -> host buffer':>28s} {'host restatement':>28s}")
    for name, dev_fn, host_fn in rows:
        d, h = timed(dev_fn), timed(host_fn)
        print(f"{name:40s} {d[0]:9.3f} ({d[1]:7.3f} .. {d[2]:7.3f}) {h[0]:9.3f} ({h[1]:7.3f} .. {h[2]:7.3f})")
    for extra in ([], ["--device-percentile"]):
        secs = []
        for _ in range(2):  # alternating would need one process; two runs each show the spread
            r = subprocess.run([sys.executable, os.path.join(ROOT, "Test_KITTI.py"), "--synthetic", "--iters", "30"] + extra, capture_output=True, text=True,
                               timeout=600, cwd=ROOT)
            assert r.returncode == 0, r.stderr[-2000:]
            secs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["sec_per_image_median"])
        print(f"Test_KITTI.py --synthetic --iters 30 {' '.join(extra) or '(host percentile)':22s} sec_per_image_median {secs}")


if __name__ == "__main__":
    main()
