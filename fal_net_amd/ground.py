"""The ground plane of a scan on the device (csrc/ground.hip): a consensus fit over plane hypotheses, the refit from the moments of the inliers,
heights above the plane and the removal of the ground from a scan -- the road plane that the pseudo-LiDAR pipelines and the KITTI-object detectors
read beside every scan (planes/<frame>.txt), and the only check of metric scale that needs no ground truth: the camera height it implies.

  triples(seed, H, n)                  the H index triples of the hypotheses: a stated 64-bit integer mix on the host, no device RNG
  hypotheses(points, triples, ...)     the (H, 4) f32 planes (falnet_ground_hypotheses)
  consensus(points, planes, tol, ...)  the inlier count of every plane and the winner's record (falnet_ground_consensus): the all-pairs hot loop
  moments(points, tol, ...)            the f64 moments of a plane's inliers into one row of doubles (falnet_ground_moments)
  solve(row)                           the refit: the regression of z on (x, y) from a row, pure numpy f64 on the host
  fit(points, ...)                     triples, hypotheses, consensus, `refits` times moments + solve -> GroundPlane or None
  heights(points, plane), split(points, plane, lo, hi, inside)
  to_camera(plane, P), write_plane(path, plane_cam), read_plane(path)
  GroundPlanes                         the product behind Test_KITTI.py --ground
  HYP_BLOCK, POINT_TILE, TARGET_WORKGROUPS, default_splits, SPLIT_TILE
                                       the kernels' decomposition: the tests take their shapes from these

A point is the 16-byte record of pseudo_lidar.unproject (x forward, y left, z up, .).  A plane is held in height form z = p x + q y + r and every
residual is the vertical one, e = z - ((p x + q y) + r), every operation rounded to f32 in this order; a point is an inlier iff |e| <= tol
(include/falnet_hip.h; the numpy restatement is tests/_ground_ref.py).  Nothing here needs a GPU to import; like the rest of the
package there is no CPU fallback: every device function raises on a CPU tensor."""
import collections
import math
import os

import numpy as np
import torch

HYP_BLOCK = 512           # GR_BLOCK of csrc/ground.hip: the hypotheses of one workgroup
POINT_TILE = 1024         # GR_TILE: the point records of one LDS tile
TARGET_WORKGROUPS = 512   # GR_TARGET_WGS: what the default split rule fills
MAX_SPLITS = 1024
SPLIT_TILE = 2048         # ORD_TILE of csrc/ordered.h: the records of one workgroup of split()'s ordered compaction
MAX_HYPOTHESES = 4096     # FALNET_GROUND_MAX_HYPOTHESES
ROW = 16                  # FALNET_GROUND_ROW; the columns (FALNET_GROUND_*):
COL = {"n": 0, "sx": 1, "sy": 2, "sz": 3, "sxx": 4, "sxy": 5, "syy": 6, "sxz": 7, "syz": 8, "szz": 9, "index": 10, "count": 11, "p": 12, "q": 13, "r": 14,
       "status": 15}
BEST_WORDS = 8            # FALNET_GROUND_BEST_WORDS; the words (FALNET_GROUND_BEST_*):
BEST = {"key_lo": 0, "key_hi": 1, "status": 2, "index": 3, "p": 4, "q": 5, "r": 6, "count": 7}

_MASK = (1 << 64) - 1
_GOLDEN, _MIX1, _MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

GroundPlane = collections.namedtuple("GroundPlane", "p q r normal d sensor_height tilt_deg inliers n rms hypothesis hypothesis_count")
GroundPlane.__doc__ = """A refined plane z = p x + q y + r in the scan's axes (float64): normal = (-p, -q, 1) / sqrt(1 + p p + q q), the unit normal with
positive z; d the offset of normal . X + d = 0, which is the height of the sensor (the origin) above the plane, sensor_height = d; tilt_deg the angle
between the normal and the z axis; inliers of n points summed by the last refit; rms their vertical residual; hypothesis and hypothesis_count the
winning index of the consensus and its count (-1 and 0 for a plane that did not come from a consensus)."""


def default_splits(n, H):
    """falnet_ground_splits restated: enough ranges of whole point tiles that the grid reaches TARGET_WORKGROUPS workgroups, at most one per tile."""
    blocks, tiles = -(-int(H) // HYP_BLOCK), -(-int(n) // POINT_TILE)
    return max(1, min(-(-TARGET_WORKGROUPS // blocks), tiles, MAX_SPLITS))


def triples(seed, H, n):
    """(H, 3) int32: entry (h, k) is mix64(seed, 3 h + k) mod n with, in arithmetic modulo 2^64,
        x = seed + 0x9E3779B97F4A7C15 (i + 1);  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
    (the finaliser of splitmix64 on a counter): numpy integers on the host, a pure function of its arguments.  1 <= n < 2^31."""
    H, n = int(H), int(n)
    if not 1 <= H <= MAX_HYPOTHESES or not 1 <= n < 1 << 31:
        raise ValueError("ground.triples: H must lie in [1, {}] and n in [1, 2^31), got {} and {}".format(MAX_HYPOTHESES, H, n))
    i = np.arange(1, 3 * H + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(int(seed) & _MASK) + np.uint64(_GOLDEN) * i
        x ^= x >> np.uint64(30)
        x *= np.uint64(_MIX1)
        x ^= x >> np.uint64(27)
        x *= np.uint64(_MIX2)
        x ^= x >> np.uint64(31)
    return (x % np.uint64(n)).astype(np.int32).reshape(H, 3)


def tan2_of(max_tilt):
    """tan^2 of a tilt in degrees as the double the library compares with: 0 <= max_tilt < 90."""
    max_tilt = float(max_tilt)
    if not 0.0 <= max_tilt < 90.0:
        raise ValueError("ground: max_tilt must lie in [0, 90) degrees, got {}".format(max_tilt))
    t = math.tan(math.radians(max_tilt))
    return t * t


def _points(x, what):
    """(n, 4) or (n, 3) f32 CUDA tensor -> contiguous (n, 4); three columns are padded once, with zeros."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("fal_net_amd.ground runs on an MI355X only (no CPU fallback); {} is {}".format(
            what, "on " + str(x.device) if torch.is_tensor(x) else type(x).__name__))
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] not in (3, 4):
        raise ValueError("{}: expected (n, 4) or (n, 3) float32 points, got {} {}".format(what, tuple(x.shape), x.dtype))
    x = x.detach()
    if x.shape[1] == 3:
        x = torch.nn.functional.pad(x, (0, 1))
    return x.contiguous()


def _out(t, shape, dtype, device, name):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not torch.is_tensor(t) or t.device != device or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("out: {} must be a contiguous {} tensor of shape {} on {}".format(name, dtype, tuple(shape), device))
    return t


def _check_n(n, what):
    if not 3 <= n < 1 << 31:
        raise ValueError("ground.{}: a plane needs 3 <= n < 2^31 points, got {}".format(what, n))


def hypotheses(points, triples, max_tilt=15.0, out=None):
    """-> (H, 4) f32 planes on the device: row h is (p, q, r, 1) of the plane through the three points triples[h] names, formed in f64 in the stated
    order, or four +0 where the hypothesis is invalid: p, q or r not finite (a repeated index, a collinear triple) or p p + q q > tan^2(max_tilt).
    triples: (H, 3) int32, a host array (ground.triples) or a tensor on the device.  Bit for bit the numpy restatement."""
    from . import _lib as L
    pts = _points(points, "points")
    n = int(pts.shape[0])
    _check_n(n, "hypotheses")
    tr = triples if torch.is_tensor(triples) else torch.from_numpy(np.ascontiguousarray(np.asarray(triples, dtype=np.int32)))
    if tr.dim() != 2 or tr.shape[1] != 3 or tr.dtype != torch.int32 or not 1 <= tr.shape[0] <= MAX_HYPOTHESES:
        raise ValueError("triples: expected (H, 3) int32 with 1 <= H <= {}, got {} {}".format(MAX_HYPOTHESES, tuple(tr.shape), tr.dtype))
    tr = tr.to(pts.device).contiguous()
    H = int(tr.shape[0])
    planes = _out(out, (H, 4), torch.float32, pts.device, "planes")
    with torch.cuda.device(pts.device):
        L.check(L.lib().falnet_ground_hypotheses(L.ptr(pts), n, L.ptr(tr), H, tan2_of(max_tilt), L.ptr(planes), L.stream_ptr()), "ground_hypotheses")
    return planes


_hypotheses = hypotheses  # fit() has a parameter of this name


def consensus(points, planes, tol, splits=0, out=None, workspace=None):
    """-> (counts, best): counts[h] (int32, H entries) the number of points within `tol` of plane h vertically, 0 for an invalid plane; best: BEST_WORDS
    int32 words on the device (BEST): the maximum of the 64-bit key (count << 32) | (0xffffffff - h) -- the largest count, ties to the smallest index
    -- as two words, the status (0: no hypothesis has 3 inliers), the winning index (-1 then), the bits of its p, q, r, the largest count.  planes: (H, 4)
    f32 as hypotheses() writes them.  splits: into how many ranges the points are divided over the grid (0: the library's choice, default_splits) -- the
    result is the same for every value.  out: a (counts, best) pair to write into.  workspace: an int64 tensor of at least
    falnet_ground_consensus_workspace_bytes / 8 words (S > 1), or None.  No value is read from the device; bit-identical from run to run."""
    from . import _lib as L
    pts = _points(points, "points")
    n, splits, tol = int(pts.shape[0]), int(splits), float(tol)
    _check_n(n, "consensus")
    if (not torch.is_tensor(planes) or planes.device != pts.device or planes.dtype != torch.float32 or planes.dim() != 2 or planes.shape[1] != 4
            or not 1 <= planes.shape[0] <= MAX_HYPOTHESES):
        raise ValueError("planes: expected an (H, 4) float32 tensor on {} with 1 <= H <= {}".format(pts.device, MAX_HYPOTHESES))
    planes = planes.detach().contiguous()
    H = int(planes.shape[0])
    if not 0 <= splits <= MAX_SPLITS:
        raise ValueError("consensus: splits must lie in [0, {}] (0: the library's choice), got {}".format(MAX_SPLITS, splits))
    if not 0.0 <= tol < float("inf"):
        raise ValueError("consensus: tol must be finite and >= 0, got {}".format(tol))
    counts, best = (None, None) if out is None else out
    counts = _out(counts, (H,), torch.int32, pts.device, "counts")
    best = _out(best, (BEST_WORDS,), torch.int32, pts.device, "best")
    lib = L.lib()
    need = int(lib.falnet_ground_consensus_workspace_bytes(n, H, splits)) // 8
    if need and (workspace is None or workspace.numel() < need):
        workspace = torch.empty(need, dtype=torch.int64, device=pts.device)
    elif workspace is not None and (workspace.dtype != torch.int64 or workspace.device != pts.device):
        raise ValueError("workspace: expected an int64 tensor on {}".format(pts.device))
    with torch.cuda.device(pts.device):
        L.check(lib.falnet_ground_consensus(L.ptr(pts), n, L.ptr(planes), H, tol, splits, L.ptr(counts), L.ptr(best), L.ptr(workspace) if need else None,
                                            L.stream_ptr()), "ground_consensus")
    return counts, best


def best_key(best):
    """The 64-bit key of a `best` record read to the host (an array of BEST_WORDS int32)."""
    b = np.asarray(best, np.int32).view(np.uint32)
    return (int(b[BEST["key_hi"]]) << 32) | int(b[BEST["key_lo"]])


def moments(points, tol, best=None, plane=None, index=-1, count=0, out=None, workspace=None):
    """-> ROW doubles on the device (COL): over the points within `tol` of one plane vertically n, sum x, y, z, xx, xy, yy, xz, yz, zz, then the plane:
    index, count, p, q, r, status.  The plane is `best`, the record consensus() left on the device (no host round trip; status 0 sums nothing), or
    `plane` = (p, q, r), rounded to f32 here, with the `index` and `count` the row is to carry.  out: a contiguous tensor of ROW doubles (a row of a
    table).  Ordered f64 sums over a fixed grid: two calls give the same bits."""
    from . import _lib as L
    pts = _points(points, "points")
    n, tol = int(pts.shape[0]), float(tol)
    _check_n(n, "moments")
    if (best is None) == (plane is None):
        raise ValueError("moments: give either best (the device record of consensus) or plane = (p, q, r)")
    if best is not None and (not torch.is_tensor(best) or best.device != pts.device or best.dtype != torch.int32 or tuple(best.shape) != (BEST_WORDS,)
                             or not best.is_contiguous()):
        raise ValueError("best: expected the {} int32 words of consensus() on {}".format(BEST_WORDS, pts.device))
    p, q, r = (0.0, 0.0, 0.0) if plane is None else (float(np.float32(v)) for v in plane)
    if not 0.0 <= tol < float("inf"):
        raise ValueError("moments: tol must be finite and >= 0, got {}".format(tol))
    row = _out(out, (ROW,), torch.float64, pts.device, "row")
    lib = L.lib()
    need = int(lib.falnet_ground_moments_workspace_bytes()) // 8
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.int64, device=pts.device)
    elif workspace.dtype != torch.int64 or workspace.device != pts.device:
        raise ValueError("workspace: expected an int64 tensor on {}".format(pts.device))
    with torch.cuda.device(pts.device):
        L.check(lib.falnet_ground_moments(L.ptr(pts), n, L.ptr(best) if best is not None else None, p, q, r, int(index), int(count), tol, L.ptr(row),
                                          L.ptr(workspace), L.stream_ptr()), "ground_moments")
    return row


def solve(row):
    """The refit, on the host in float64: the 3 x 3 normal equations of the regression of z on (x, y) with an intercept, centred on the inliers' means
    -- which leaves the 2 x 2 system [cxx cxy; cxy cyy] (p, q) = (cxz, cyz) with cab = sum ab - sum a . mean b -- solved by Cramer's rule, and
    r = mean z - p mean x - q mean y.  row: ROW doubles (COL).  -> GroundPlane, or None where the row has no plane: status 0, fewer than 3 inliers, or
    inliers on one vertical plane (the determinant is not positive).  rms: sqrt(max(0, czz - p cxz - q cyz) / n), the inliers' vertical residual."""
    row = np.asarray(row, np.float64).reshape(-1)
    if row.shape[0] != ROW:
        raise ValueError("solve: expected {} doubles, got {}".format(ROW, row.shape[0]))
    n = row[COL["n"]]
    if not row[COL["status"]] == 1.0 or not n >= 3:
        return None
    sx, sy, sz = row[COL["sx"]], row[COL["sy"]], row[COL["sz"]]
    mx, my, mz = sx / n, sy / n, sz / n
    cxx, cxy, cyy = row[COL["sxx"]] - sx * mx, row[COL["sxy"]] - sx * my, row[COL["syy"]] - sy * my
    cxz, cyz, czz = row[COL["sxz"]] - sx * mz, row[COL["syz"]] - sy * mz, row[COL["szz"]] - sz * mz
    det = cxx * cyy - cxy * cxy
    if not (det > 0.0 and np.isfinite(det)):
        return None
    p, q = (cxz * cyy - cyz * cxy) / det, (cyz * cxx - cxz * cxy) / det
    r = mz - p * mx - q * my
    if not (np.isfinite(p) and np.isfinite(q) and np.isfinite(r)):
        return None
    s = math.sqrt(1.0 + p * p + q * q)
    rms = math.sqrt(max(0.0, czz - p * cxz - q * cyz) / n)
    return GroundPlane(p=float(p), q=float(q), r=float(r), normal=(float(-p / s), float(-q / s), float(1.0 / s)), d=float(-r / s), sensor_height=float(-r / s),
                       tilt_deg=float(math.degrees(math.atan(math.sqrt(p * p + q * q)))), inliers=int(n), n=0, rms=float(rms),
                       hypothesis=int(row[COL["index"]]), hypothesis_count=int(row[COL["count"]]))


def fit(points, tol=0.15, hypotheses=512, seed=0, max_tilt=15.0, refits=2):
    """The ground plane of a scan -> GroundPlane, or None when there is none (fewer than 3 points, no hypothesis with 3 inliers, a degenerate refit).
    `hypotheses` planes through seeded point triples (ground.triples), the consensus winner within `tol` metres vertically among those tilted at most
    max_tilt degrees, then `refits` >= 1 times: the moments of the current plane's inliers, read as ONE table row, and solve().  The first row sums
    the winner's inliers and carries the consensus result; each later refit sums the inliers of the previous refined plane (its f32 parameters).
    Values read from the device: `refits` rows of ROW doubles, nothing else."""
    pts = _points(points, "points")
    n, refits = int(pts.shape[0]), int(refits)
    if refits < 1:
        raise ValueError("ground.fit: refits must be >= 1, got {}".format(refits))
    if n < 3:
        return None
    planes = _hypotheses(pts, triples(seed, hypotheses, n), max_tilt)
    _, best = consensus(pts, planes, tol)
    table = torch.full((refits, ROW), float("nan"), dtype=torch.float64, device=pts.device)
    row = moments(pts, tol, best=best, out=table[0]).cpu().numpy()  # the read of the first row: status, winner and moments together
    plane = solve(row)
    index, count = int(row[COL["index"]]), int(row[COL["count"]])
    for k in range(1, refits):
        if plane is None:
            return None
        plane = solve(moments(pts, tol, plane=(plane.p, plane.q, plane.r), index=index, count=count, out=table[k]).cpu().numpy())
    return None if plane is None else plane._replace(n=n)


def plane_f32(plane):
    """What the device takes of a refined plane: (f32 p, f32 q, f32 r, cz = f32(1 / sqrt(1 + p p + q q))) as Python floats."""
    p, q, r = float(plane.p), float(plane.q), float(plane.r)
    return float(np.float32(p)), float(np.float32(q)), float(np.float32(r)), float(np.float32(1.0 / math.sqrt(1.0 + p * p + q * q)))


def heights(points, plane, out=None):
    """-> (n,) f32 on the device: h[i] = (z - ((p x + q y) + r)) cz in f32 in this order with plane_f32(plane): the height of every point above the
    plane along its normal.  plane: a GroundPlane (anything with p, q, r).  Bit for bit the numpy line."""
    from . import _lib as L
    pts = _points(points, "points")
    n = int(pts.shape[0])
    h = _out(out, (n,), torch.float32, pts.device, "heights")
    p, q, r, cz = plane_f32(plane)
    if n:
        with torch.cuda.device(pts.device):
            L.check(L.lib().falnet_ground_heights(L.ptr(pts), n, p, q, r, cz, L.ptr(h), L.stream_ptr()), "ground_heights")
    return h


def split(points, plane, lo, hi, inside=True, out=None):
    """-> the records with lo < heights <= hi (inside=True) or every other record (inside=False; a NaN height is outside every range), in point
    order: byte for byte points[(lo < h) & (h <= hi)] or its complement.  out: a contiguous (capacity, 4) f32 tensor to write into; more kept points
    than it holds raise.  One int64 is read from the device."""
    from . import _lib as L
    pts = _points(points, "points")
    n, lo, hi = int(pts.shape[0]), float(lo), float(hi)
    if lo != lo or hi != hi:
        raise ValueError("ground.split: lo or hi is NaN")
    if out is None:
        out = torch.empty((n, 4), dtype=torch.float32, device=pts.device)
    elif (not torch.is_tensor(out) or out.device != pts.device or out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != 4
          or not out.is_contiguous()):
        raise ValueError("out: expected a contiguous (capacity, 4) float32 tensor on {}".format(pts.device))
    if n == 0:
        return out[:0]
    p, q, r, cz = plane_f32(plane)
    lib = L.lib()
    count = torch.empty(1, dtype=torch.int64, device=pts.device)
    ws = torch.empty(int(lib.falnet_ground_split_workspace_bytes(n)) // 8, dtype=torch.int64, device=pts.device)
    with torch.cuda.device(pts.device):
        L.check(lib.falnet_ground_split(L.ptr(pts), n, p, q, r, cz, lo, hi, int(bool(inside)), L.ptr(out) if out.shape[0] else None, int(out.shape[0]),
                                        L.ptr(count), L.ptr(ws), L.stream_ptr()), "ground_split")
    kept = int(count.item())  # the one read
    if kept > out.shape[0]:
        raise RuntimeError("ground.split: {} points are kept but `out` holds {}: its first {} records are written, the rest is lost".format(
            kept, out.shape[0], out.shape[0]))
    return out[:kept]


def to_camera(plane, P):
    """The plane in the frame of the camera that the 3 x 4 matrix `P` projects into -> (a, b, c, d) float64 with a x + b y + c z + d = 0 in camera
    axes (x right, y down, z forward) and (a, b, c) the unit normal pointing up, so b < 0 on a road and d is the camera's height above it.
    With (K, R, t) = velodyne.decompose(P) a scan point X is the camera point R X + t: the normal turns with R and d' = d - (R normal) . t."""
    from . import velodyne
    _, R, t = velodyne.decompose(P)
    nrm = np.dot(R, np.asarray(plane.normal, np.float64))
    return np.array([nrm[0], nrm[1], nrm[2], float(plane.d) - float(np.dot(nrm, t))], np.float64)


def write_plane(path, plane_cam):
    """planes/<frame>.txt of the KITTI-object tools: the lines '# Plane', 'Width 4', 'Height 1', then 'a b c d' in %e."""
    v = np.asarray(plane_cam, np.float64).reshape(-1)
    if v.shape[0] != 4 or not np.isfinite(v).all():
        raise ValueError("write_plane: expected 4 finite numbers a b c d, got {}".format(v.tolist()))
    with open(path, "w") as f:
        f.write("# Plane\nWidth 4\nHeight 1\n" + " ".join("%e" % x for x in v) + "\n")


def read_plane(path):
    """The four numbers of a write_plane file as float64."""
    lines = [ln.strip() for ln in open(path).read().splitlines() if ln.strip()]
    if lines[:3] != ["# Plane", "Width 4", "Height 1"] or len(lines) != 4 or len(lines[3].split()) != 4:
        raise ValueError("{} is not a plane file ('# Plane', 'Width 4', 'Height 1', 'a b c d')".format(path))
    return np.array([float(x) for x in lines[3].split()], np.float64)


def check_fit_args(tol=0.15, hypotheses=512, seed=0, max_tilt=15.0, refits=2):
    """The parameters of fit() as a dict; ValueError names the one out of range."""
    tol, hypotheses, refits = float(tol), int(hypotheses), int(refits)
    if not 0.0 < tol < float("inf"):
        raise ValueError("ground: tol must be a finite positive distance in metres, got {}".format(tol))
    if not 1 <= hypotheses <= MAX_HYPOTHESES:
        raise ValueError("ground: hypotheses must lie in [1, {}], got {}".format(MAX_HYPOTHESES, hypotheses))
    if refits < 1:
        raise ValueError("ground: refits must be >= 1, got {}".format(refits))
    tan2_of(max_tilt)
    return dict(tol=tol, hypotheses=hypotheses, seed=int(seed), max_tilt=float(max_tilt), refits=refits)


def dense_cloud(disp, P, fb, max_depth=80.0):
    """The cloud a frame's plane is fitted on: pseudo_lidar.unproject of every pixel with depth in (0, max_depth], no height ceiling, no score."""
    from . import pseudo_lidar
    return pseudo_lidar.unproject(disp, P, fb=fb, max_depth=max_depth, max_height=float("inf"))


class GroundPlanes:
    """The product behind Test_KITTI.py --ground: every frame's disparity is unprojected densely with the calibration given here (a callable
    (frame index, H, W) -> (P, fb), as pseudo_lidar.PseudoLidarWriter takes it; dense_cloud), fitted, and the plane written in the camera's frame as
    Ground/<frame:010d>.txt under `save_path` (write_plane of to_camera).  A frame without a plane writes no file and counts as failed.
    Values read from the device per frame: the point count of unproject and the `refits` rows of fit().  extra: what summary() says besides."""
    key = "ground"

    def __init__(self, save_path, calibration, tol=0.15, hypotheses=512, seed=0, max_tilt=15.0, refits=2, max_depth=80.0, extra=None):
        if calibration is None or not callable(calibration):
            raise ValueError("GroundPlanes: calibration must be a callable (frame index, H, W) -> (P, fb)")
        if not np.isfinite(max_depth) or not max_depth > 0.0:
            raise ValueError("GroundPlanes: max_depth must be finite and positive, got {}".format(max_depth))
        self.kw = check_fit_args(tol, hypotheses, seed, max_tilt, refits)
        self.save_path, self.calibration, self.max_depth, self.extra = save_path, calibration, float(max_depth), dict(extra or {})
        self.folder = os.path.join(save_path, "Ground")
        os.makedirs(self.folder, exist_ok=True)
        self.frames = self.failed = 0
        self.planes = {}  # frame index -> GroundPlane, the fitted frames

    def file(self, i):
        return os.path.join(self.folder, "{:010d}.txt".format(i))

    def frame(self, f):
        """An inference.Frame: `f.disp` unprojected, fitted, written."""
        P, fb = self.calibration(f.index, int(f.disp.shape[-2]), int(f.disp.shape[-1]))
        plane = fit(dense_cloud(f.disp, P, fb, self.max_depth), **self.kw)
        self.frames += 1
        if plane is None:
            self.failed += 1
            return None
        self.planes[f.index] = plane
        write_plane(self.file(f.index), to_camera(plane, P))
        return plane

    def summary(self):
        """The run's extra JSON line: frames, fitted, failed, and over the fitted frames the mean sensor height, tilt, inlier fraction and rms (None
        where no frame has a plane)."""
        ps = list(self.planes.values())
        mean = lambda v: float(np.mean(v)) if len(v) else None  # noqa: E731
        out = {"frames": self.frames, "fitted": len(ps), "failed": self.failed, "sensor_height": mean([p.sensor_height for p in ps]),
               "tilt_deg": mean([p.tilt_deg for p in ps]), "inlier_fraction": mean([p.inliers / p.n for p in ps]), "rms": mean([p.rms for p in ps])}
        return dict(out, **dict(self.kw, max_depth=self.max_depth), **self.extra)
