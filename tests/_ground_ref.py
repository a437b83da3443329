"""Host restatement of the ground plane (fal_net_amd/ground.py, csrc/ground.hip).  numpy only, no GPU.

  road_cloud(n, seed), lattice_cloud(n, seed), line_cloud(n)
                                     the seeded clouds of the tests
  hypotheses_ref(points, triples, max_tilt)
                                     the f64 chain of include/falnet_hip.h per triple, element-wise numpy in the stated order (numpy does not fuse a
                                     multiply and an add): u = P1 - P0, v = P2 - P0; nx = uy vz - uz vy, ny = uz vx - ux vz, nz = ux vy - uy vx;
                                     p = -(nx / nz), q = -(ny / nz), r = z0 - (p x0 + q y0); valid iff finite and (p p + q q) <= tan2_max
                                     -> (H, 4) float32, four +0 where invalid
  residual_ref(points, p, q, r)      e = z - ((p x + q y) + r) in float32 in this order
  consensus_ref(points, planes, tol) -> (counts int64, best dict): |e| <= tol counted per valid plane; the maximum of (count << 32) | (0xffffffff - h)
  moments_ref(points, plane, tol, ...)
                                     -> (row, bounds): the row of falnet_ground_moments with math.fsum sums, and per sum (n + 2) 2^-53 sum |term|
  fit_ref(points, ...)               ground.fit restated on these; the refit is ground.solve itself: it is host code, pinned by the host tests
  heights_ref(points, plane), split_ref(points, plane, lo, hi, inside)"""
import math

import numpy as np

from fal_net_amd import ground as G

ROW = 16
N, SX, SY, SZ, SXX, SXY, SYY, SXZ, SYZ, SZZ, INDEX, COUNT, P, Q, R, STATUS = range(16)
ROAD = (0.02, -0.01, -1.65)  # the planted plane z = -1.65 + 0.02 x - 0.01 y


def road_cloud(n, seed=21):
    """(n, 4) float32: x in [2, 60) metres ahead, y in [-15, 15); 40 % of the points lie on ROAD with 4 cm Gaussian noise, the rest is uniform in the
    3 m column above the plane's offset."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(2.0, 60.0, n), rng.uniform(-15.0, 15.0, n)
    on = rng.random(n) < 0.4
    z = np.where(on, ROAD[2] + ROAD[0] * x + ROAD[1] * y + rng.normal(0.0, 0.04, n), rng.uniform(ROAD[2], ROAD[2] + 3.0, n))
    return np.stack([x, y, z, rng.random(n)], 1).astype(np.float32)


def lattice_cloud(n, seed=22):
    """(n, 4) float32 of integer coordinates in [0, 12)^3: collinear and repeated triples, exact arithmetic and ties in abundance."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(0, 12, (n, 3)), rng.integers(0, 100, (n, 1))], 1).astype(np.float32)


def line_cloud(n):
    """(n, 4) float32 on one straight line: every triple is collinear."""
    t = np.arange(n, dtype=np.float32)
    return np.stack([1.0 + t, 2.0 * t, 0.5 * t - 1.0, np.zeros(n, np.float32)], 1).astype(np.float32)


def hypotheses_ref(points, triples, max_tilt=15.0):
    pts = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    tr = np.asarray(triples, np.int64)
    tan2 = G.tan2_of(max_tilt)
    p0, p1, p2 = pts[tr[:, 0]], pts[tr[:, 1]], pts[tr[:, 2]]
    with np.errstate(all="ignore"):
        x0, y0, z0 = p0[:, 0], p0[:, 1], p0[:, 2]
        ux, uy, uz = p1[:, 0] - x0, p1[:, 1] - y0, p1[:, 2] - z0
        vx, vy, vz = p2[:, 0] - x0, p2[:, 1] - y0, p2[:, 2] - z0
        nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        p, q = -(nx / nz), -(ny / nz)
        r = z0 - (p * x0 + q * y0)
        valid = np.isfinite(p) & np.isfinite(q) & np.isfinite(r) & ((p * p + q * q) <= tan2)
        out = np.stack([p, q, r, np.ones_like(p)], 1).astype(np.float32)
    out[~valid] = 0.0
    return out


def residual_ref(points, p, q, r):
    pts = np.asarray(points, np.float32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    p, q, r = np.float32(p), np.float32(q), np.float32(r)
    with np.errstate(all="ignore"):
        e = z - ((p * x + q * y) + r)
    assert e.dtype == np.float32
    return e


def inliers_ref(points, p, q, r, tol):
    with np.errstate(invalid="ignore"):
        return np.abs(residual_ref(points, p, q, r)) <= np.float32(tol)  # a NaN compares false


def key_of(count, h):
    return (int(count) << 32) | (0xFFFFFFFF - int(h))


def consensus_ref(points, planes, tol):
    planes = np.asarray(planes, np.float32)
    counts = np.zeros(len(planes), np.int64)
    for h, (p, q, r, w) in enumerate(planes):
        if w != 0:
            counts[h] = int(inliers_ref(points, p, q, r, tol).sum())
    key = max(key_of(c, h) for h, c in enumerate(counts))
    count, h = key >> 32, 0xFFFFFFFF - (key & 0xFFFFFFFF)
    found = count >= 3
    best = {"key": key, "status": int(found), "index": int(h) if found else -1, "count": int(count),
            "plane": planes[h, :3].copy() if found else np.zeros(3, np.float32)}
    return counts, best


def best_words(best):
    """The reference's best record as the BEST_WORDS uint32 words of the device."""
    p = np.asarray(best["plane"], np.float32).view(np.uint32)
    return np.array([best["key"] & 0xFFFFFFFF, best["key"] >> 32, best["status"], best["index"] & 0xFFFFFFFF, p[0], p[1], p[2], best["count"]], np.uint32)


def moments_ref(points, plane, tol, index=-1, count=0, status=1):
    """plane: (p, q, r), rounded to f32 as the device takes them.  -> (row of ROW doubles, {column: bound}).  The terms are f64 products of f32
    coordinates widened -- one rounding each, the same on both sides -- and the sums math.fsum, correctly rounded.  An ordered f64 sum of n terms, in any
    order and grouping, is within (n - 1) u (1 + O(n u)) sum |term| of the exact sum with u = 2^-53, and math.fsum within u |sum|: (n + 2) 2^-53
    sum |term| covers both (the bound of tests/_cloud_ref.py: sum_bounds, restated for signed terms)."""
    pts = np.asarray(points, np.float32)
    row, bounds = np.zeros(ROW, np.float64), {}
    row[INDEX], row[COUNT], row[STATUS] = index, count, status
    row[P], row[Q], row[R] = (float(np.float32(v)) for v in plane)
    if not status:
        row[P] = row[Q] = row[R] = 0.0
        return row, {c: 0.0 for c in range(SX, SZZ + 1)}
    m = inliers_ref(pts, *plane, tol)
    x, y, z = (pts[m, k].astype(np.float64) for k in range(3))
    n = int(m.sum())
    row[N] = n
    for col, term in ((SX, x), (SY, y), (SZ, z), (SXX, x * x), (SXY, x * y), (SYY, y * y), (SXZ, x * z), (SYZ, y * z), (SZZ, z * z)):
        row[col] = math.fsum(term.tolist())
        bounds[col] = (n + 2) * 2.0 ** -53 * math.fsum(np.abs(term).tolist())
    return row, bounds


def fit_ref(points, tol=0.15, hypotheses=512, seed=0, max_tilt=15.0, refits=2):
    """-> (GroundPlane or None, the rows read): ground.fit on the restatements above."""
    pts = np.asarray(points, np.float32)
    n = len(pts)
    if n < 3:
        return None, []
    planes = hypotheses_ref(pts, G.triples(seed, hypotheses, n), max_tilt)
    _, best = consensus_ref(pts, planes, tol)
    row, _ = moments_ref(pts, best["plane"], tol, best["index"], best["count"], best["status"])
    rows, plane = [row], G.solve(row)
    for _ in range(1, refits):
        if plane is None:
            return None, rows
        row, _ = moments_ref(pts, (plane.p, plane.q, plane.r), tol, best["index"], best["count"])
        rows.append(row)
        plane = G.solve(row)
    return (None if plane is None else plane._replace(n=n)), rows


def heights_ref(points, plane):
    p, q, r, cz = G.plane_f32(plane)
    with np.errstate(all="ignore"):
        h = residual_ref(points, p, q, r) * np.float32(cz)
    assert h.dtype == np.float32
    return h


def split_ref(points, plane, lo, hi, inside=True):
    pts = np.asarray(points, np.float32)
    h = heights_ref(pts, plane)
    with np.errstate(invalid="ignore"):
        m = (np.float32(lo) < h) & (h <= np.float32(hi))
    return pts[m if inside else ~m]


def centred_condition(row):
    """The 2-norm condition number of the centred normal matrix [cxx cxy; cxy cyy] of a row, and the matrix."""
    n = row[N]
    mx, my = row[SX] / n, row[SY] / n
    A = np.array([[row[SXX] - row[SX] * mx, row[SXY] - row[SX] * my], [row[SXY] - row[SX] * my, row[SYY] - row[SY] * my]])
    return float(np.linalg.cond(A)), A
