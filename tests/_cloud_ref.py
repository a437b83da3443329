"""Host restatement of the cloud metrics (fal_net_amd/cloud_metrics.py, csrc/nearest.hip).  numpy only, no GPU.

  nearest_ref(query, ref)            the f32 chain of include/falnet_hip.h per pair, element-wise numpy in the stated order (numpy does not fuse a
                                     multiply and an add), chunked over the queries: dx = qx - rx, dy, dz; d2 = (dx dx + dy dy) + dz dz; NaN pairs
                                     masked; np.argmin for the first minimum -> (d2 float32, idx int32), +inf / -1 where no pair takes part
  nearest_f64(query, ref)            a float64 brute force of the same quantity -> (d2, idx, second-best d2)
  cloud_errors_ref(d2_pred, d2_gt, thresholds)
                                     the row of falnet_cloud_errors: counts as integers, sums by math.fsum over the finite entries
  sum_bounds(row)                    how far an ordered f64 sum of the device may sit from those sums
  product_ref(disp, target, ...)     the composed reference of cloud_metrics.CloudMetrics.frame on top of tests/_lidar_ref.py -> (row, pred, gt)
  derived(row, thresholds)           accuracy, completeness, chamfer, ... of one row in plain Python"""
import math

import numpy as np

import _lidar_ref as LR

ROW, MAX_K = 22, 8
N_PRED, SUM_PRED, SUMSQ_PRED, N_GT, SUM_GT, SUMSQ_GT, HIT_PRED, HIT_GT = 0, 1, 2, 3, 4, 5, 6, 14


def nearest_ref(query, ref, chunk=256):
    q, r = np.asarray(query, np.float32), np.asarray(ref, np.float32)
    nq, nr = len(q), len(r)
    d2, idx = np.full(nq, np.inf, np.float32), np.full(nq, -1, np.int32)
    if nr == 0:
        return d2, idx
    with np.errstate(all="ignore"):
        for a in range(0, nq, chunk):
            b = min(a + chunk, nq)
            dx = q[a:b, None, 0] - r[None, :, 0]
            dy = q[a:b, None, 1] - r[None, :, 1]
            dz = q[a:b, None, 2] - r[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            nan = np.isnan(d)
            d[nan] = np.inf  # a masked pair never beats one that takes part: +inf ties go to the first index, sorted out below
            j = np.argmin(d, axis=1)  # the first minimum
            best = d[np.arange(b - a), j]
            # a minimum of +inf is attained by the first pair that takes part and IS +inf, if any; else nothing takes part
            for i in np.flatnonzero(np.isinf(best)):
                part = np.flatnonzero(~nan[i])
                j[i] = part[0] if len(part) else -1
            d2[a:b], idx[a:b] = best, j
    return d2, idx


def attained(query, ref, d2):
    """Per query, how many references attain d2[q] in the f32 chain (bit equality; a NaN pair attains nothing)."""
    q, r = np.asarray(query, np.float32), np.asarray(ref, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = (q[:, None, i] - r[None, :, i] for i in range(3))
        d = (dx * dx + dy * dy) + dz * dz
    return (d == np.asarray(d2, np.float32)[:, None]).sum(1)


def nearest_f64(query, ref, chunk=256):
    """Finite clouds with at least two references: the exact (to f64 rounding) squared distances -> (best, its first index, second best)."""
    q, r = np.asarray(query, np.float64)[:, :3], np.asarray(ref, np.float64)[:, :3]
    best, idx, second = np.empty(len(q)), np.empty(len(q), np.int64), np.empty(len(q))
    for a in range(0, len(q), chunk):
        d = ((q[a:a + chunk, None, :] - r[None, :, :]) ** 2).sum(-1)
        j = np.argmin(d, axis=1)
        rows = np.arange(len(j))
        best[a:a + chunk], idx[a:a + chunk] = d[rows, j], j
        d[rows, j] = np.inf
        second[a:a + chunk] = d.min(1)
    return best, idx, second


def cloud_errors_ref(d2_pred, d2_gt, thresholds):
    """-> ROW float64: exact integer counts; the two sums per direction correctly rounded (math.fsum) over float64 terms -- math.sqrt of an f32 widened
    to f64 is correctly rounded, and the widened value itself is exact."""
    row = np.zeros(ROW, np.float64)
    for d2, n_at, hit_at in ((d2_pred, N_PRED, HIT_PRED), (d2_gt, N_GT, HIT_GT)):
        v = np.asarray(d2, np.float32)
        v = v[np.isfinite(v)].astype(np.float64)
        row[n_at] = len(v)
        row[n_at + 1] = math.fsum(math.sqrt(x) for x in v.tolist())
        row[n_at + 2] = math.fsum(v.tolist())
        for k, t in enumerate(thresholds):
            row[hit_at + k] = int(np.count_nonzero(v <= np.float64(t) * np.float64(t)))
    return row


def sum_bounds(row):
    """{column: absolute bound} for the four sums of a reference row.  An ordered f64 sum of n non-negative terms, in any order and grouping, is
    within (n - 1) u (1 + O(n u)) relative of the exact sum with u = 2^-53, and math.fsum within u: (n + 2) 2^-53 relative covers both (the
    bound tests/_sparsify_ref.py uses).  The terms of the squared sum are exact (an f32 widened).  A term of the root sum is the device's f64 sqrt,
    which is held to 1 ulp = 2 u here and not to correct rounding, against a correctly rounded reference term (u): 3 more units."""
    out = {}
    for n_at in (N_PRED, N_GT):
        n = row[n_at]
        out[n_at + 1] = (n + 5) * 2.0 ** -53 * row[n_at + 1]
        out[n_at + 2] = (n + 2) * 2.0 ** -53 * row[n_at + 2]
    return out


def derived(row, thresholds):
    """The host arithmetic of cloud_metrics.summarize for one row, in plain Python; None where a direction is empty."""
    n_p, n_g = row[N_PRED], row[N_GT]
    if not (n_p >= 1 and n_g >= 1):
        return None
    acc, comp = row[SUM_PRED] / n_p, row[SUM_GT] / n_g
    out = {"accuracy": acc, "completeness": comp, "chamfer": acc + comp, "chamfer_l2": row[SUMSQ_PRED] / n_p + row[SUMSQ_GT] / n_g,
           "precision": [], "recall": [], "f": []}
    for k in range(len(thresholds)):
        P, R = row[HIT_PRED + k] / n_p, row[HIT_GT + k] / n_g
        out["precision"].append(P), out["recall"].append(R), out["f"].append(2 * P * R / (P + R) if P + R > 0 else 0.0)
    return out


def product_ref(disp, target, P, fb, target_fb, thresholds, on="gt", beams=0, az_bins=1024, max_depth=80.0):
    """CloudMetrics.frame restated: the ground truth (a depth when target_fb is None, else a disparity) and the prediction (a disparity with `fb`,
    which carries the median factor already) through tests/_lidar_ref.py's unproject_ref with no height ceiling; on="gt": the prediction keeps the
    pixels with target > 0; both directions of nearest_ref; cloud_errors_ref."""
    target = np.asarray(target, np.float32)
    gt = LR.unproject_ref(target, P, fb=target_fb, max_depth=max_depth, max_height=np.inf)
    score, threshold = ((target > 0).astype(np.float32), 0.5) if on == "gt" else (None, None)
    pred = LR.unproject_ref(np.asarray(disp, np.float32), P, fb=fb, score=score, threshold=threshold, max_depth=max_depth, max_height=np.inf,
                            beams=beams, az_bins=az_bins)
    d_p, _ = nearest_ref(pred, gt)
    d_g, _ = nearest_ref(gt, pred)
    return cloud_errors_ref(d_p, d_g, thresholds), pred, gt
