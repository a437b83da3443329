"""Pseudo-LiDAR: a predicted depth or disparity map back-projected into a Velodyne-format scan on the device (csrc/lidar.hip:
falnet_velo_unproject) -- the inverse of velodyne.project, and the form in which a KITTI depth network's output reaches a 3-D detector: (n, 4)
float32 records x forward, y left, z up, intensity, 16 bytes each, exactly the points of a raw scan's .bin file.

  unproject(map, P, fb, ...)      the kept points of an (H, W) map: every pixel in row-major order (dense), or one point per (elevation, azimuth)
                                  bin of a simulated scanner, the nearest one (beams > 0)
  edge_tables(...)                the float64 tangents of the bin edges the device searches
  write_bin(path, points)         the .bin file; velodyne.load_scan reads it back
  PseudoLidarWriter               Pseudo_lidar/<frame>.bin of Test_KITTI.py --pseudo-lidar

The result is defined operation by operation (include/falnet_hip.h); the host restatement it is tested against is
tests/_lidar_ref.py.  Nothing here needs a GPU to import; `unproject` does: like the rest of the package it has no CPU fallback and raises on a
CPU tensor."""
import ctypes as C
import os

import numpy as np
import torch

from . import velodyne
from .confidence import check_min_conf

MAX_BEAMS, MAX_AZ_BINS = 128, 4096


def edge_tables(beams, az_bins, elevation=(-24.8, 2.0), azimuth=(-45.0, 45.0)):
    """(te, ta): te[k] = tan(elev_lo + k (elev_hi - elev_lo) / beams), k = 0 .. beams, and ta[j] = tan(az_lo + j (az_hi - az_lo) / az_bins),
    j = 0 .. az_bins, angles in degrees, float64.  Both ranges must be increasing and inside (-90, 90): the tables are then increasing."""
    beams, az_bins = int(beams), int(az_bins)
    if not 1 <= beams <= MAX_BEAMS or not 1 <= az_bins <= MAX_AZ_BINS:
        raise ValueError("pseudo_lidar: beams must lie in [1, {}] and az_bins in [1, {}], got {} and {}".format(MAX_BEAMS, MAX_AZ_BINS, beams, az_bins))
    out = []
    for name, rng, n in (("elevation", elevation, beams), ("azimuth", azimuth, az_bins)):
        lo, hi = np.deg2rad(np.float64(rng[0])), np.deg2rad(np.float64(rng[1]))
        if not -np.pi / 2 < lo < hi < np.pi / 2:
            raise ValueError("pseudo_lidar: the {} range must be increasing and inside (-90, 90) degrees, got {}".format(name, tuple(rng)))
        out.append(np.tan(lo + np.arange(n + 1, dtype=np.float64) * (hi - lo) / n))
    return out[0], out[1]


def _map(x, what, H=None, W=None, device=None):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("fal_net_amd.pseudo_lidar.unproject runs on an MI355X only (no CPU fallback); {} is {}".format(
            what, "on " + str(x.device) if torch.is_tensor(x) else type(x).__name__))
    x = x.detach()
    if x.dim() < 2 or x.numel() != x.shape[-2] * x.shape[-1]:
        raise ValueError("{}: expected one (H, W) map, got {}".format(what, tuple(x.shape)))
    if H is not None and (tuple(x.shape[-2:]) != (H, W) or x.device != device):
        raise ValueError("{}: expected a ({}, {}) map on {}, got {} on {}".format(what, H, W, device, tuple(x.shape), x.device))
    return x.to(torch.float32).contiguous()


def unproject(map, P, fb=None, score=None, threshold=None, intensity=1.0, min_depth=0.0, max_depth=80.0, max_height=1.0, beams=0, az_bins=1024,
              elevation=(-24.8, 2.0), azimuth=(-45.0, 45.0), out=None):
    """The map (CUDA f32 (H, W); leading dimensions of size 1 are allowed) back through the 3 x 4 float64 matrix `P` of velodyne.project into an
    (n, 4) f32 tensor of points x, y, z, intensity on the same device.  fb: None -- the map is a depth, the projection's third homogeneous
    coordinate, what velodyne.project writes -- or focal length times baseline > 0 -- the map is a disparity and depth = fb / disparity.  Kept
    are the pixels with min_depth < depth <= max_depth, score >= threshold (with a score map; both or neither), x > 0 and z <= max_height
    (float('inf'): no ceiling).  intensity: a number, or an (H, W) map.  beams = 0: every kept pixel in row-major order; beams > 0: the
    nearest point of each of beams x az_bins bins over the elevation and azimuth ranges (degrees), in bin order.  out: a contiguous (capacity, 4) f32
    tensor to write into; more kept points than it holds raise.  One int64 is read from the device.  Bit-identical from run to run."""
    from . import _lib as L
    m = _map(map, "map")
    H, W = int(m.shape[-2]), int(m.shape[-1])
    dev = m.device
    if (score is None) != (threshold is None):
        raise ValueError("pseudo_lidar.unproject: score and threshold go together")
    sc = None if score is None else _map(score, "score", H, W, dev)
    imap = None
    if torch.is_tensor(intensity):
        imap, intensity = _map(intensity, "intensity", H, W, dev), 0.0
    Q = velodyne.backprojection_matrix(P)
    beams, az_bins = int(beams), int(az_bins)
    if beams < 0:
        raise ValueError("pseudo_lidar.unproject: beams must be >= 0, got {}".format(beams))
    te = ta = None
    if beams > 0:
        te_h, ta_h = edge_tables(beams, az_bins, elevation, azimuth)
        te, ta = torch.from_numpy(te_h).to(dev), torch.from_numpy(ta_h).to(dev)
    fb = 0.0 if fb is None else float(fb)  # 0 tells the kernel that the map is a depth
    if not 0.0 <= fb < float("inf"):
        raise ValueError("pseudo_lidar.unproject: fb must be positive (or None for a depth map), got {}".format(fb))
    lib = L.lib()
    ws_bytes = int(lib.falnet_lidar_workspace_bytes(H, W, beams, az_bins))
    if ws_bytes <= 0:
        raise ValueError("pseudo_lidar.unproject: a {} x {} map with beams = {}, az_bins = {} is outside what falnet_velo_unproject takes "
                         "(1 <= H W < 2^31, beams <= {}, 1 <= az_bins <= {})".format(H, W, beams, az_bins, MAX_BEAMS, MAX_AZ_BINS))
    if out is None:
        out = torch.empty((H * W if beams == 0 else min(H * W, beams * az_bins), 4), dtype=torch.float32, device=dev)
    elif (not torch.is_tensor(out) or out.device != dev or out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != 4
          or not out.is_contiguous()):
        raise ValueError("out: expected a contiguous (capacity, 4) float32 tensor on {}".format(dev))
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    q12 = (C.c_double * 12)(*Q.reshape(-1).tolist())
    with torch.cuda.device(dev):
        L.check(lib.falnet_velo_unproject(L.ptr(m), fb, L.ptr(sc), 0.0 if threshold is None else float(threshold), L.ptr(imap), float(intensity), q12,
                                          float(min_depth), float(max_depth), float(max_height), H, W, beams, az_bins, L.ptr(te), L.ptr(ta),
                                          L.ptr(out), int(out.shape[0]), L.ptr(count), L.ptr(ws), L.stream_ptr()), "velo_unproject")
    n = int(count.item())  # the one read
    if n > out.shape[0]:
        raise RuntimeError("pseudo_lidar.unproject: {} points are kept but `out` holds {}: its first {} records are written, the rest is lost".format(
            n, out.shape[0], out.shape[0]))
    return out[:n]


def write_bin(path, points):
    """`points` ((n, 4) float32, a tensor on any device or an array) as a KITTI scan: n 16-byte little-endian records, nothing else."""
    pts = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    if pts.ndim != 2 or pts.shape[1] != 4 or pts.dtype != np.float32:
        raise ValueError("write_bin: expected (n, 4) float32 points, got {} {}".format(pts.shape, pts.dtype))
    np.ascontiguousarray(pts).astype("<f4", copy=False).tofile(path)
    return int(pts.shape[0])


class PseudoLidarWriter:
    """Test_KITTI.py --pseudo-lidar: writes Pseudo_lidar/{frame:010d}.bin under `save_path`, the frame's disparity back-projected with the
    parameters given here.  calibration: a callable (frame index, H, W) -> (P, fb) -- frame() asks it per frame -- or None when
    write() is always given both.  min_conf: with it, write() needs the frame's confidence map and keeps only the pixels of conf >= min_conf.
    extra: what summary() says besides the counts.
    min_component = K: a speckle filter.  The frame's component sizes (components.size_score of the disparity, joined at component_jump, the depth
    bounds as disparity bounds lo = fb / max_depth and hi = fb / min_depth or infinity, and with min_conf the confidence map as the components' score,
    so that a low-confidence pixel has size 0) become unproject's score with threshold K: only the pixels in components of at least K pixels are kept,
    and unproject sees only the size map.  An approximation: the components judge the bound on the disparity, unproject on its own f64 depth
    fb / disparity, so a pixel within rounding of a bound can count towards a size and still be dropped by unproject, or the reverse; and the scan's
    x > 0 and max_height tests do not enter the graph -- a component is counted with the pixels those tests drop afterwards.
    remove_ground = h: the ground is taken out of the scan.  The frame's plane is fitted (ground.fit with the parameters `ground`, a dict) on the
    dense, ceiling-free unprojection of the frame (ground.dense_cloud: every pixel within max_depth, whatever the scan's own filters are), and the scan
    that is written loses every point whose height above that plane (ground.heights) is <= h metres.  A frame without a plane is written unfiltered
    and counted (summary: ground_failed).  None: the writer does exactly what it does without the parameter."""
    key = "pseudo_lidar"

    def __init__(self, save_path, calibration=None, beams=0, az_bins=1024, max_depth=80.0, max_height=1.0, min_conf=None, min_depth=0.0,
                 elevation=(-24.8, 2.0), azimuth=(-45.0, 45.0), extra=None, min_component=None, component_jump=0.05, remove_ground=None, ground=None):
        from .components import check_jump, check_min_component
        self.remove_ground, self.ground_kw = None, None
        if remove_ground is not None:
            from .ground import check_fit_args
            self.remove_ground, self.ground_kw = float(remove_ground), check_fit_args(**dict(ground or {}))
            if not np.isfinite(self.remove_ground):
                raise ValueError("remove_ground must be a finite height in metres (or None), got {}".format(remove_ground))
        self.ground_failed = self.ground_removed = 0
        if beams != 0:
            edge_tables(beams, az_bins, elevation, azimuth)  # the range checks, before the first frame
        check_min_conf(min_conf)
        self.min_component, self.component_jump = check_min_component(min_component), check_jump(component_jump, "component_jump")
        if not np.isfinite(max_depth) or not max_depth > min_depth:
            raise ValueError("max_depth must be finite and above min_depth, got {}".format(max_depth))
        self.save_path, self.calibration, self.min_conf, self.extra = save_path, calibration, min_conf, dict(extra or {})
        self.kw = dict(beams=int(beams), az_bins=int(az_bins), max_depth=float(max_depth), max_height=float(max_height), min_depth=float(min_depth),
                       elevation=tuple(elevation), azimuth=tuple(azimuth))
        self.folder = os.path.join(save_path, "Pseudo_lidar")
        os.makedirs(self.folder, exist_ok=True)
        self.frames = self.points = self.pixels = 0

    def file(self, i):
        return os.path.join(self.folder, "{:010d}.bin".format(i))

    def frame(self, f):
        """An inference.Frame: `f.disp`, the disparity the run evaluates, back-projected with the calibration the writer has for the frame; the
        confidence map (f.conf(): one more disparity-only forward) only when the writer filters by it."""
        conf = f.conf() if self.min_conf is not None else None
        P, fb = self.calibration(f.index, f.disp.shape[-2], f.disp.shape[-1])
        self.write(f.index, f.disp, P, fb, conf=conf)

    def write(self, i, disp, P, fb, conf=None):
        """Frame `i`: disp (1, 1, H, W) or (H, W) disparity on the device, P and fb its calibration, conf the confidence map (needed with min_conf)."""
        if self.min_conf is not None and conf is None:
            raise ValueError("PseudoLidarWriter: min_conf = {} needs the frame's confidence map".format(self.min_conf))
        use = self.min_conf is not None
        score, threshold = (conf, self.min_conf) if use else (None, None)
        if self.min_component is not None:
            from . import components
            lo_z, hi_z = self.kw["min_depth"], self.kw["max_depth"]
            # a disparity's bounds are the depth bounds through fb; a depth map (fb None) takes them as they are
            lo, hi = (lo_z, hi_z) if fb is None else (fb / hi_z, fb / lo_z if lo_z > 0.0 else float("inf"))
            if score is not None:
                score = score.reshape(disp.shape)
            score, threshold = components.size_score(disp, self.component_jump, lo=lo, hi=hi, score=score, threshold=threshold), float(self.min_component)
        pts = unproject(disp, P, fb=fb, score=score, threshold=threshold, **self.kw)
        if self.remove_ground is not None:
            from . import ground
            plane = ground.fit(ground.dense_cloud(disp, P, fb, self.kw["max_depth"]), **self.ground_kw)
            if plane is None:
                self.ground_failed += 1
            else:  # what is NOT in (-inf, h]: heights > h, and a NaN height
                before = int(pts.shape[0])
                pts = ground.split(pts, plane, float("-inf"), self.remove_ground, inside=False)
                self.ground_removed += before - int(pts.shape[0])
        n = write_bin(self.file(i), pts)
        self.frames += 1
        self.points += n
        self.pixels += int(disp.shape[-2] * disp.shape[-1])
        return n

    def summary(self):
        """The run's extra JSON line: frames, mean points per scan, the kept fraction of all pixels."""
        out = {"frames": self.frames, "points": self.points, "mean_points": self.points / self.frames if self.frames else float("nan"),
               "kept_fraction": self.points / self.pixels if self.pixels else float("nan"), "beams": self.kw["beams"]}
        if self.kw["beams"]:
            out["az_bins"] = self.kw["az_bins"]
        if self.min_conf is not None:
            out["min_conf"] = self.min_conf
        if self.min_component is not None:
            out["min_component"] = self.min_component
        if self.remove_ground is not None:
            out.update(remove_ground=self.remove_ground, ground_failed=self.ground_failed, ground_removed=self.ground_removed)
        return dict(out, **self.extra)
