"""Host restatement of the pseudo-LiDAR back-projection (fal_net_amd/pseudo_lidar.py, csrc/lidar.hip).  numpy only, no GPU.

  kept_records(map, P, ...)     steps 1-5 of include/falnet_hip.h per pixel, element-wise numpy in the stated order (numpy does not fuse a multiply
                                and an add): (flat indices of the kept pixels in row-major order, their (n, 4) float32 records, their float32 depths)
  unproject_ref(map, P, ...)    the (n, 4) float32 scan: the records in pixel order (beams = 0), or the winner of every (beam, azimuth) bin in bin
                                order -- searchsorted(side='right') - 1 on the two edge tables, the smallest (bits(d) << 32) | index per bin
  edge_tables(...)              the float64 tangents of the bin edges, restated
  backprojection(P)             [M^-1 | M^-1 P[:, 3]], composed by hand
  road_depth(seed, H, W)        a seeded road-like depth map in 3 .. 80 m with 5 % holes
  roundtrip_bound(P, pts, d)    how far (float)s_2 of a back-projected point may sit from the depth it was made of

tests/test_lidar_host.py closes the loop with tests/_velo_ref.py: spec(P, unproject_ref(depth)) gives `depth` back; tests/test_gpu_pseudo_lidar.py
holds the kernels to unproject_ref bit for bit."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def backprojection(P):
    P = np.asarray(P, np.float64)
    m_inv = np.linalg.inv(P[:, :3])
    return np.hstack((m_inv, np.dot(m_inv, P[:, 3:4])))


def edge_tables(beams, az_bins, elevation=(-24.8, 2.0), azimuth=(-45.0, 45.0)):
    out = []
    for (lo, hi), n in ((elevation, beams), (azimuth, az_bins)):
        lo, hi = np.deg2rad(np.float64(lo)), np.deg2rad(np.float64(hi))
        out.append(np.tan(lo + np.arange(n + 1, dtype=np.float64) * (hi - lo) / n))
    return out[0], out[1]


def kept_records(map, P, fb=None, score=None, threshold=None, intensity=1.0, min_depth=0.0, max_depth=80.0, max_height=1.0):
    m = np.asarray(map, np.float32)
    H, W = m.shape
    Q = backprojection(P)
    m = m.reshape(-1)
    with np.errstate(all="ignore"):
        if fb is not None and fb > 0:
            ok = m > np.float32(0)  # a NaN disparity compares false
            d = np.zeros(H * W, np.float32)
            d[ok] = (np.float64(fb) / m[ok].astype(np.float64)).astype(np.float32)
        else:
            ok = np.ones(H * W, bool)
            d = m
        ok &= (d > np.float32(min_depth)) & (d <= np.float32(max_depth))  # f32 compares: NaN and infinity fail
        if score is not None:
            ok &= np.asarray(score, np.float32).reshape(-1) >= np.float32(threshold)
        idx = np.flatnonzero(ok)
        d = d[idx]
        v, u = idx // W, idx % W
        u1, v1, dd = (u + 1).astype(np.float64), (v + 1).astype(np.float64), d.astype(np.float64)
        X = []
        for i in range(3):
            r = (Q[i, 0] * u1 + Q[i, 1] * v1) + Q[i, 2]
            X.append((dd * r - Q[i, 3]).astype(np.float32))
        front = (X[0] > np.float32(0)) & (X[2] <= np.float32(max_height))
    idx, d = idx[front], d[front]
    inten = np.asarray(intensity, np.float32).reshape(-1)[idx] if np.ndim(intensity) else np.full(len(idx), intensity, np.float32)
    return idx, np.stack([X[0][front], X[1][front], X[2][front], inten], axis=1).astype(np.float32), d


def _bin(table, val):
    """#{k : val >= table[k]} - 1 for an increasing table; a NaN counts nothing."""
    b = np.searchsorted(table, val, side="right") - 1
    b[np.isnan(val)] = -1
    return b


def unproject_ref(map, P, fb=None, score=None, threshold=None, intensity=1.0, min_depth=0.0, max_depth=80.0, max_height=1.0, beams=0, az_bins=1024,
                  elevation=(-24.8, 2.0), azimuth=(-45.0, 45.0)):
    idx, rec, d = kept_records(map, P, fb, score, threshold, intensity, min_depth, max_depth, max_height)
    if beams == 0:
        return rec
    te, ta = edge_tables(beams, az_bins, elevation, azimuth)
    with np.errstate(all="ignore"):
        x, y, z = rec[:, 0].astype(np.float64), rec[:, 1].astype(np.float64), rec[:, 2].astype(np.float64)
        rho = np.sqrt(x * x + y * y)
        beam, col = _bin(te, z / rho), _bin(ta, y / x)
    inside = (beam >= 0) & (beam < beams) & (col >= 0) & (col < az_bins)
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    table = np.full(beams * az_bins, EMPTY, np.uint64)
    np.minimum.at(table, (beam[inside] * az_bins + col[inside]).astype(np.int64), keys[inside])
    winners = (table[table != EMPTY] & np.uint64(0xFFFFFFFF)).astype(np.int64)  # bin order, beam major
    return rec[np.searchsorted(idx, winners)]  # idx is increasing: the record of each winning pixel


def road_depth(seed, H, W, holes=0.05):
    """float32 (H, W): a ground plane 1.65 m below a camera whose horizon lies at 0.46 H, walls of piecewise-constant depth per column above it,
    2 % multiplicative noise, all clipped to 3 .. 80 m; then `holes` of the pixels set to 0."""
    rng = np.random.default_rng(seed)
    rows = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore"):
        ground = 1.65 * 1.92 * H / np.maximum(rows - 0.46 * H, 1e-9)
    walls = np.repeat(rng.uniform(6.0, 80.0, (W + 15) // 16), 16)[:W][None, :]
    depth = np.minimum(ground, walls) * rng.uniform(0.98, 1.02, (H, W))
    depth = np.clip(depth, 3.0, 80.0).astype(np.float32)
    depth[rng.random((H, W)) < holes] = 0
    return depth


def roundtrip_bound(P, pts, d):
    """2^-23 (sum_i |P[2][i]| |X_i| + |P[2][3]|) + 2^-24 d per point: each f32 coordinate of the record is within half an ulp (2^-24 relative) of
    the exact back-projection, the float64 arithmetic on either side adds nothing at this scale, and (float)s_2 rounds once more."""
    P = np.asarray(P, np.float64)
    X = np.abs(np.asarray(pts, np.float64)[:, :3])
    return 2.0 ** -23 * (X @ np.abs(P[2, :3]) + abs(P[2, 3])) + 2.0 ** -24 * np.asarray(d, np.float64)
