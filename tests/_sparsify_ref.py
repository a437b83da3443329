"""The numpy definition of the sparsification curves (include/falnet_hip.h: falnet_sparsify), for tests/test_sparsify_host.py and
tests/test_gpu_sparsify.py: the key image by integer bit operations, np.argsort(~key, kind="stable"), the depth chain of myUtils as
tests/test_gpu_metrics.py forms it, math.fsum for the two sums (exactly rounded: the yardstick of the derived bound), integer counts."""
import math

import numpy as np

from fal_net_amd import myUtils as utils

METRICS = ("abs_rel", "rms", "d1")


def key_image(x):
    """f32 -> u32, monotone: NaN above everything, -0 below +0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    k = np.where((u >> np.uint32(31)) != 0, u ^ np.uint32(0xFFFFFFFF), u | np.uint32(0x80000000))
    k[(u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return k.astype(np.uint32)


def order(x):
    """The removal order of the f32 values x: the largest first, NaN before everything, ties in index order."""
    return np.argsort(~key_image(x), kind="stable")


def cut_ranks(n, steps):
    return [(j * n) // steps for j in range(steps)]


def pairs(mode, pred, gt, use_median=False, min_d=1.0, max_d=None):
    """-> (g, p, idx): the clamped f64 depths of the counted pixels in region row-major order and their flat positions in the H x W frame."""
    H, W = gt.shape
    with np.errstate(all="ignore"):
        if mode == "make3d":
            max_d = 70.0 if max_d is None else max_d
            mask = (gt > 0) * (gt < max_d)
            g, p = gt[mask], (721 * 0.22 / (pred + (1.0 - (pred > 0))))[mask]
            idx = np.flatnonzero(mask)
            use_median = True
        else:
            max_d = 80.0 if max_d is None else max_d
            gd, pd = (utils.disps_to_depths_kitti2015 if mode == "kitti2015" else utils.disps_to_depths_kitti)([gt], [pred])
            mask = gd[0] > 0
            g, p = gd[0][mask].copy(), pd[0][mask].copy()
            if mode == "kitti2015":
                idx = np.flatnonzero(mask)
            else:
                r, c = np.nonzero(mask)
                idx = (H - 219 + r) * W + 44 + c
        if use_median and len(g):
            p = np.median(g) / np.median(p) * p
        p, g = np.clip(p, min_d, max_d).astype(np.float64), np.clip(g, min_d, max_d).astype(np.float64)
    return g, p, idx


def errors(g, p):
    with np.errstate(all="ignore"):
        return np.abs(g - p) / g, (g - p) * (g - p), np.maximum(g / p, p / g)


def kept_curve(values, perm, steps, kind):
    """The curve of one metric over the cuts of one ordering: 'abs_rel' (fsum / n_j), 'rms' (sqrt(fsum / n_j)), 'd1' (values: the flags t < 1.25)."""
    n = len(perm)
    if n == 0:
        return [float("nan")] * steps
    v = values[perm].tolist()
    out = []
    for r in cut_ranks(n, steps):
        nj = n - r
        if kind == "d1":
            out.append((nj - int(sum(v[r:]))) / nj)
        else:
            s = math.fsum(v[r:]) / nj
            out.append(s if kind == "abs_rel" else math.sqrt(s))
    return out


def curves_from_pairs(g, p, xs, steps):
    """g, p: the f64 depths of the n counted pixels; xs: per score the f32 values x (sign applied) of those pixels -> the row of
    1 + (3 len(xs) + 3) steps doubles."""
    e_abs, e_sq, t = errors(g, p)
    lt = (t < 1.25).astype(np.int64)
    vals = {"abs_rel": e_abs, "rms": e_sq, "d1": lt}
    row = [float(len(g))]
    for x in xs:
        perm = order(np.asarray(x, np.float32))
        for m in METRICS:
            row += kept_curve(vals[m], perm, steps, m)
    for m, x in zip(METRICS, (e_abs, e_sq, t)):
        row += kept_curve(vals[m], order(x.astype(np.float32)), steps, m)
    return np.array(row, np.float64)


def score_values(scores, idx):
    """scores: [(H x W f32 map, sign)] -> per score the signed f32 values at the counted pixels."""
    out = []
    for m, sign in scores:
        v = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)[idx]
        out.append(v if sign > 0 else -v)
    return out


def sparsify_ref(mode, pred, gt, scores, use_median=False, min_d=1.0, max_d=None, steps=50):
    g, p, idx = pairs(mode, pred, gt, use_median, min_d, max_d)
    return curves_from_pairs(g, p, score_values(scores, idx), steps)


def split(row, n_scores, steps):
    """row -> (n, score curves (n_scores, 3, S), oracle curves (3, S))."""
    body = np.asarray(row[1:], np.float64).reshape(n_scores + 1, 3, steps)
    return row[0], body[:n_scores], body[n_scores]


def trapezoid(curve):
    curve = np.asarray(curve, np.float64)
    return (1.0 / len(curve)) * (math.fsum(curve.tolist()) - (curve[0] + curve[-1]) / 2)


def areas(row, n_scores, steps):
    """-> (ause, aurg), each (n_scores, 3)."""
    _, sc, orc = split(row, n_scores, steps)
    ause = np.array([[trapezoid(sc[s, m] - orc[m]) for m in range(3)] for s in range(n_scores)]).reshape(n_scores, 3)
    aurg = np.array([[trapezoid(sc[s, m, 0] - sc[s, m]) for m in range(3)] for s in range(n_scores)]).reshape(n_scores, 3)
    return ause, aurg


def curve_bound(n, steps, ref):
    """|got - ref| <= (n_j + 2) 2^-53 |ref| per cut: any-order summation of n_j non-negative terms against the exactly rounded fsum, plus the
    division and the square root.  ref: (..., S) -> the bound of the same shape."""
    nj = np.array([n - r for r in cut_ranks(int(n), steps)], np.float64)
    return (nj + 2) * 2.0 ** -53 * np.abs(ref)
