"""Host references of the Velodyne projection (fal_net_amd/velodyne.py, csrc/velo.hip).  numpy only, no GPU.

  spec(P, points, H, W, vel_depth)            the chain the kernel is defined by (include/falnet_hip.h), element-wise float64 numpy with the matrix
                                              product written out in its fixed order (numpy does not fuse a multiply and an add), the minimum per
                                              pixel with np.minimum.at on an inf-filled buffer;
  monodepth_host(P, points, H, W, vel_depth)  the original formulation, Monodepth's generate_depth_map after the calibration files are read: np.dot,
                                              last write wins, a Counter loop that takes the minimum over the pixels hit more than once, negatives to zero.

                                              (Pixels are numbered row * W + column for the Counter; Monodepth's own `sub2ind` numbers them
                                              row * (W - 1) + column - 1, which gives the last pixel of a row the number of the first pixel of
                                              the next: that slip is not part of the definition and is not restated.)

Both return the (H, W) float32 map.  tests/test_velo_host.py shows that they agree on seeded scans; tests/test_gpu_velo.py holds the kernel to `spec`
bit for bit.  `seeded_scan` and `kitti_like_P` are the inputs both test files share."""
import os
from collections import Counter

import numpy as np

# KITTI-like calibration values (the magnitudes of a 2011_09_26 calibration, rounded; not a copy of one)
P_RECT_02 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
P_RECT_03 = np.array([[721.5377, 0.0, 609.5593, -339.5242], [0.0, 721.5377, 172.854, 2.199936], [0.0, 0.0, 1.0, 0.002729905]])
R_RECT_00 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]])
VELO_R = np.array([[0.007533745, -0.9999714, -0.000616602], [0.01480249, 0.0007280733, -0.9998902], [0.9998621, 0.00752379, 0.01480755]])
VELO_T = np.array([-0.004069766, -0.07631618, -0.2717806])


def compose_P(p_rect=P_RECT_02, r_rect=R_RECT_00, velo_r=VELO_R, velo_t=VELO_T):
    """P_rect . [R_rect | 0; 0 1] . [R T; 0 0 0 1], composed by hand (float64)."""
    v2c = np.eye(4)
    v2c[:3, :3], v2c[:3, 3] = velo_r, velo_t
    r4 = np.eye(4)
    r4[:3, :3] = r_rect
    return np.dot(np.dot(p_rect, r4), v2c)


def write_calib(d, cam3=True):
    """calib_cam_to_cam.txt and calib_velo_to_cam.txt of the values above in KITTI's format, with the non-numeric and unused lines such files carry."""
    os.makedirs(d, exist_ok=True)
    row = lambda a: " ".join(repr(float(v)) for v in np.asarray(a).reshape(-1))
    with open(os.path.join(d, "calib_cam_to_cam.txt"), "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n")
        f.write("S_00: 1.392000e+03 5.120000e+02\n")
        f.write("R_rect_00: " + row(R_RECT_00) + "\n")
        f.write("P_rect_02: " + row(P_RECT_02) + "\n")
        if cam3:
            f.write("P_rect_03: " + row(P_RECT_03) + "\n")
    with open(os.path.join(d, "calib_velo_to_cam.txt"), "w") as f:
        f.write("calib_time: 15-Mar-2012 11:37:16\nR: " + row(VELO_R) + "\nT: " + row(VELO_T) + "\ndelta_f: 0.000000e+00 0.000000e+00\n")


def kitti_like_P(image_scale=1.0):
    """The composed matrix; image_scale multiplies its first two rows (a smaller image of the same scene)."""
    P = compose_P()
    P[:2] *= image_scale
    return P


def seeded_scan(seed, n):
    """(n, 4) float32: x uniform in [-5, 80] with a quarter of the points in [-1, 6] (close points spread over few pixels, so pixels collide),
    y in [-40, 40], z in [-3, 3], reflectance in [0, 1)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5.0, 80.0, n)
    near = rng.random(n) < 0.25
    x[near] = rng.uniform(-1.0, 6.0, int(near.sum()))
    pts = np.stack([x, rng.uniform(-40.0, 40.0, n), rng.uniform(-3.0, 3.0, n), rng.random(n)], axis=1)
    return pts.astype(np.float32)


def spec(P, points, H, W, vel_depth=False):
    P = np.asarray(P, np.float64)
    pts = np.asarray(points, np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        pts = pts[pts[:, 0] >= np.float32(0)]  # a NaN x compares false
        x, y, z = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64), pts[:, 2].astype(np.float64)
        s = [((P[i, 0] * x + P[i, 1] * y) + P[i, 2] * z) + P[i, 3] for i in range(3)]
        u, v = np.rint(s[0] / s[2]) - 1.0, np.rint(s[1] / s[2]) - 1.0
        d = (pts[:, 0] if vel_depth else s[2]).astype(np.float32)
        ok = (u >= 0) & (v >= 0) & (u < W) & (v < H)  # as doubles: NaN and infinity fail
        ui, vi, d = u[ok].astype(np.int64), v[ok].astype(np.int64), d[ok]
    buf = np.full(H * W, np.inf, np.float32)
    hit = np.zeros(H * W, bool)
    np.minimum.at(buf, vi * W + ui, d)
    hit[vi * W + ui] = True
    buf[~hit] = 0  # a pixel no point reaches
    buf[buf < 0] = 0  # after the minimum: a negative minimum hides a positive point on the same pixel
    return buf.reshape(H, W)


def monodepth_host(P, points, H, W, vel_depth=False):
    velo = np.array(points, np.float32).reshape(-1, 4)
    velo[:, 3] = 1.0
    with np.errstate(all="ignore"):
        velo = velo[velo[:, 0] >= 0, :]
        pts_im = np.dot(np.asarray(P, np.float64), velo.T).T
        pts_im[:, :2] = pts_im[:, :2] / pts_im[:, 2][..., np.newaxis]
        if vel_depth:
            pts_im[:, 2] = velo[:, 0]
        pts_im[:, 0] = np.round(pts_im[:, 0]) - 1  # (minus 1: the pixel numbering of KITTI's matlab code)
        pts_im[:, 1] = np.round(pts_im[:, 1]) - 1
        val = (pts_im[:, 0] >= 0) & (pts_im[:, 1] >= 0) & (pts_im[:, 0] < W) & (pts_im[:, 1] < H)
    pts_im = pts_im[val, :]
    depth = np.zeros((H, W))
    rows, cols = pts_im[:, 1].astype(np.int64), pts_im[:, 0].astype(np.int64)
    depth[rows, cols] = pts_im[:, 2]  # last write wins
    inds = rows * W + cols
    for dd in [item for item, count in Counter(inds.tolist()).items() if count > 1]:  # the closest point where several landed
        sel = np.where(inds == dd)[0]
        depth[rows[sel[0]], cols[sel[0]]] = pts_im[sel, 2].min()
    depth[depth < 0] = 0
    with np.errstate(over="ignore"):  # a depth beyond float32 becomes infinite, as on the device
        return depth.astype(np.float32)
