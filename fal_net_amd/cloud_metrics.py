"""Cloud metrics on the device (csrc/nearest.hip): how far is the predicted point cloud from the measured one, in metres, in space -- the Chamfer
distance and the precision / recall / F-score at distance thresholds, between the pseudo-LiDAR scan of a prediction and the back-projected
ground truth.

  nearest(query, ref, ...)            per query point the squared distance to its nearest reference point and that point's index (falnet_nearest):
                                      an LDS-tiled all-pairs kernel whose result is held exactly
  cloud_errors(pred, gt, ...)         both directions and the frame's sums, one row of doubles on the device (falnet_cloud_errors)
  CloudTable                          (frames, ROW) doubles on the device, NaN until written, read once; result() forms the means on the host
  CloudMetrics                        the product behind Test_KITTI.py --cloud-metrics
  QUERY_BLOCK, REF_TILE, TARGET_WORKGROUPS, default_splits
                                      the kernel's decomposition: the tests take their shapes from these

A pair's squared distance is d2 = (dx dx + dy dy) + dz dz with dx = qx - rx, ..., every operation rounded to f32 in that order; a NaN pair does not
take part; ties go to the smallest index (include/falnet_hip.h; the numpy restatement is tests/_cloud_ref.py).  Nothing here needs a
GPU to import; like the rest of the package there is no CPU fallback: every function raises on a CPU tensor."""
import numpy as np
import torch

QUERY_BLOCK = 1024        # NN_BLOCK of csrc/nearest.hip: the queries of one workgroup
REF_TILE = 1024           # NN_TILE: the reference records of one LDS tile
TARGET_WORKGROUPS = 512   # NN_TARGET_WGS: what the default split rule fills
MAX_SPLITS = 1024
MAX_THRESHOLDS = 8        # FALNET_CLOUD_MAX_THRESHOLDS
THRESHOLDS = (0.1, 0.25, 0.5, 1.0)
"""The default distance thresholds of the F-score in metres.  Nobody has tuned them: they span the range between a Velodyne's range noise and a
detector's box tolerance, and a run that reports an F-score should name its own."""
ROW = 22  # FALNET_CLOUD_ROW; the columns (FALNET_CLOUD_*):
COL = {"n_pred": 0, "sum_pred": 1, "sumsq_pred": 2, "n_gt": 3, "sum_gt": 4, "sumsq_gt": 5, "hit_pred": 6, "hit_gt": 14}


def default_splits(nq, nr):
    """falnet_nearest_splits restated: enough ranges of whole reference tiles that the grid reaches TARGET_WORKGROUPS workgroups, at most one per
    tile; 1 for an empty set."""
    if nq <= 0 or nr <= 0:
        return 1
    blocks, tiles = -(-nq // QUERY_BLOCK), -(-nr // REF_TILE)
    return max(1, min(-(-TARGET_WORKGROUPS // blocks), tiles, MAX_SPLITS))


def check_thresholds(thresholds):
    """The thresholds of a run as a tuple of floats: 0 to 8 finite numbers >= 0, increasing; ValueError otherwise."""
    t = tuple(float(x) for x in thresholds)
    if len(t) > MAX_THRESHOLDS or any(not 0.0 <= x < float("inf") for x in t) or any(b <= a for a, b in zip(t, t[1:])):
        raise ValueError("cloud_metrics: thresholds are at most {} increasing finite distances >= 0 in metres, got {}".format(MAX_THRESHOLDS, list(thresholds)))
    return t


def _points(x, what):
    """(n, 4) or (n, 3) f32 CUDA tensor -> contiguous (n, 4); three columns are padded once, with zeros."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("fal_net_amd.cloud_metrics runs on an MI355X only (no CPU fallback); {} is {}".format(
            what, "on " + str(x.device) if torch.is_tensor(x) else type(x).__name__))
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] not in (3, 4):
        raise ValueError("{}: expected (n, 4) or (n, 3) float32 points, got {} {}".format(what, tuple(x.shape), x.dtype))
    x = x.detach()
    if x.shape[1] == 3:
        x = torch.nn.functional.pad(x, (0, 1))
    return x.contiguous()


def nearest(query, ref, splits=0, out=None, workspace=None):
    """-> (d2, idx): for each of the nq query points the f32 squared distance to its nearest reference point and that point's int32 index in `ref`
    (the smallest index on a tie); +inf and -1 where no pair takes part (an empty `ref`, NaN coordinates).  query, ref: (n, 4) or (n, 3) float32
    CUDA tensors on one device; the fourth column is ignored.  splits: into how many ranges the references are divided over the grid (0: the
    library's choice, default_splits) -- the result is the same for every value.  out: a (d2, idx) pair of contiguous tensors of nq entries to
    write into.  workspace: an int64 tensor of at least falnet_nearest_workspace_bytes / 8 words (S > 1), or None.  No value is read from the
    device; bit-identical from run to run."""
    from . import _lib as L
    q, r = _points(query, "query"), _points(ref, "ref")
    if r.device != q.device:
        raise ValueError("nearest: query is on {} but ref on {}".format(q.device, r.device))
    nq, nr, splits = int(q.shape[0]), int(r.shape[0]), int(splits)
    if not 0 <= splits <= MAX_SPLITS:
        raise ValueError("nearest: splits must lie in [0, {}] (0: the library's choice), got {}".format(MAX_SPLITS, splits))
    if out is None:
        d2, idx = torch.empty(nq, dtype=torch.float32, device=q.device), torch.empty(nq, dtype=torch.int32, device=q.device)
    else:
        d2, idx = out
        for t, dt, name in ((d2, torch.float32, "d2"), (idx, torch.int32, "idx")):
            if not torch.is_tensor(t) or t.device != q.device or t.dtype != dt or tuple(t.shape) != (nq,) or not t.is_contiguous():
                raise ValueError("out: {} must be a contiguous {} tensor of {} entries on {}".format(name, dt, nq, q.device))
    if nq == 0:
        return d2, idx
    lib = L.lib()
    need = int(lib.falnet_nearest_workspace_bytes(nq, nr, splits)) // 8
    if need and (workspace is None or workspace.numel() < need):
        workspace = torch.empty(need, dtype=torch.int64, device=q.device)
    elif workspace is not None and (workspace.dtype != torch.int64 or workspace.device != q.device):
        raise ValueError("workspace: expected an int64 tensor on {}".format(q.device))
    with torch.cuda.device(q.device):
        L.check(lib.falnet_nearest(L.ptr(q), nq, L.ptr(r) if nr else None, nr, splits, L.ptr(d2), L.ptr(idx), L.ptr(workspace) if need else None,
                                   L.stream_ptr()), "nearest")
    return d2, idx


class CloudRow:
    """Row `index` of a CloudTable: what cloud_errors() takes as `out`."""

    def __init__(self, table, index):
        self.table, self.index = table, index

    @property
    def tensor(self):
        return self.table.table[self.index]


class CloudTable:
    """Owns the results table -- (n_frames, ROW) doubles on the device, NaN where nothing was written -- and the workspace of the sums.  row(i) hands
    out row i (the table grows on the device when i is beyond it), n is the number of rows handed out, result() reads everything back ONCE."""

    def __init__(self, n_frames=1, thresholds=THRESHOLDS, device="cuda"):
        from . import _lib as L
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("fal_net_amd.cloud_metrics runs on an MI355X only (no CPU fallback); asked for " + str(device))
        self.thresholds = check_thresholds(thresholds)
        if self.device.index is None:  # "cuda" names the current device: the tensors of a call carry its index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = torch.full((max(int(n_frames), 1), ROW), float("nan"), dtype=torch.float64, device=self.device)
        self.workspace = torch.empty(int(L.lib().falnet_cloud_errors_workspace_bytes()) // 8, dtype=torch.int64, device=self.device)
        self.nn_workspace = None  # falnet_nearest's keys, grown to the largest query set seen
        self.n = 0

    def row(self, i):
        if i >= self.table.shape[0]:  # a loader of unknown length: double, on the device (no host read)
            grown = torch.full((max(2 * self.table.shape[0], i + 1), ROW), float("nan"), dtype=torch.float64, device=self.device)
            grown[:self.table.shape[0]] = self.table
            self.table = grown
        self.n = max(self.n, i + 1)
        return CloudRow(self, i)

    def nn_workspace_for(self, nq):
        if self.nn_workspace is None or self.nn_workspace.numel() < nq:
            self.nn_workspace = torch.empty(max(int(nq), 1), dtype=torch.int64, device=self.device)
        return self.nn_workspace

    def rows(self):
        """The rows handed out so far as a host array -- one copy, one synchronisation."""
        return self.table[:self.n].cpu().numpy()

    def result(self):
        """One read of the table -> summarize(rows, thresholds)."""
        return summarize(self.rows(), self.thresholds)


def summarize(rows, thresholds):
    """(frames, ROW) doubles -> {'rows', 'thresholds', 'counted': which frames have a point in both clouds, 'frames': how many, per frame (arrays over
    ALL rows, NaN where a direction is empty or the row was never written) 'n_pred', 'n_gt', 'accuracy' = sum sqrt / n over the prediction, 'completeness'
    the same over the ground truth, 'chamfer' = accuracy + completeness, 'chamfer_l2' = the sum of the two mean squared distances, 'precision',
    'recall', 'f' ((frames, K): f = 2 P R / (P + R), 0 where P + R = 0), and '<name>_mean' of each over the counted frames (NaN when there is none)}."""
    rows = np.asarray(rows, np.float64).reshape(-1, ROW)
    K = len(thresholds)
    with np.errstate(invalid="ignore", divide="ignore"):
        n_p, n_g = rows[:, COL["n_pred"]], rows[:, COL["n_gt"]]
        n_p, n_g = np.where(n_p >= 1, n_p, np.nan), np.where(n_g >= 1, n_g, np.nan)  # NaN (never written) compares false
        acc, comp = rows[:, COL["sum_pred"]] / n_p, rows[:, COL["sum_gt"]] / n_g
        acc2, comp2 = rows[:, COL["sumsq_pred"]] / n_p, rows[:, COL["sumsq_gt"]] / n_g
        P = rows[:, COL["hit_pred"]:COL["hit_pred"] + K] / n_p[:, None]
        R = rows[:, COL["hit_gt"]:COL["hit_gt"] + K] / n_g[:, None]
        F = np.where(P + R > 0, 2 * P * R / (P + R), np.where(np.isnan(P + R), np.nan, 0.0))
    counted = ~np.isnan(n_p) & ~np.isnan(n_g)
    out = {"rows": rows, "thresholds": list(thresholds), "counted": counted, "frames": int(counted.sum()), "n_pred": n_p, "n_gt": n_g,
           "accuracy": acc, "completeness": comp, "chamfer": acc + comp, "chamfer_l2": acc2 + comp2, "precision": P, "recall": R, "f": F}
    for k in ("n_pred", "n_gt", "accuracy", "completeness", "chamfer", "chamfer_l2", "precision", "recall", "f"):
        v = out[k][counted]
        out[k + "_mean"] = (v.mean(0) if len(v) else np.full(v.shape[1:], np.nan)).tolist()
    return out


def cloud_errors(pred, gt, thresholds=None, out=None, splits=0):
    """Both nearest() calls -- prediction -> ground truth and ground truth -> prediction -- and the frame's row: per direction the number of finite
    distances, the sum of the distances and of their squares, and per threshold the count of distances within it (tau is compared squared, in f64:
    (double)d2 <= tau tau).  pred, gt: point tensors as nearest() takes them.  out: a CloudRow (CloudTable.row(i)), whose table's thresholds are then
    used (`thresholds` must be None or equal to them), or None: a table of one row with `thresholds` (default THRESHOLDS).  -> the row's tensor of
    ROW doubles on the device.  An empty cloud leaves both n's directions without a finite distance: summarize() does not count the frame."""
    from . import _lib as L
    import ctypes as C
    p, g = _points(pred, "pred"), _points(gt, "gt")
    if out is None:
        out = CloudTable(1, THRESHOLDS if thresholds is None else thresholds, p.device).row(0)
    elif not isinstance(out, CloudRow):
        raise TypeError("out must be a CloudRow (CloudTable.row(i)) or None, got " + type(out).__name__)
    t = out.table
    if thresholds is not None and check_thresholds(thresholds) != t.thresholds:
        raise ValueError("cloud_errors: the table holds the thresholds {}, the call names {}".format(list(t.thresholds), list(thresholds)))
    if p.device != t.device or g.device != t.device:
        raise ValueError("cloud_errors: the clouds are on {} and {}, the table on {}".format(p.device, g.device, t.device))
    d_p, _ = nearest(p, g, splits=splits, workspace=t.nn_workspace_for(p.shape[0]))
    d_g, _ = nearest(g, p, splits=splits, workspace=t.nn_workspace_for(g.shape[0]))
    K = len(t.thresholds)
    tau2 = (C.c_double * max(K, 1))(*[x * x for x in t.thresholds])
    with torch.cuda.device(t.device):
        L.check(L.lib().falnet_cloud_errors(L.ptr(d_p) if d_p.numel() else None, int(d_p.numel()), L.ptr(d_g) if d_g.numel() else None, int(d_g.numel()),
                                            tau2, K, L.ptr(out.tensor), L.ptr(t.workspace), L.stream_ptr()), "cloud_errors")
    return out.tensor


def target_fb(mode, width):
    """How metrics.depth_errors reads a frame's ground truth for `mode`: None -- it is a depth (eigen) -- or the focal length times baseline that turns
    its disparity into one (kitti2015)."""
    from .metrics import focal_baseline
    if mode == "eigen":
        return None
    if mode == "kitti2015":
        return focal_baseline(mode, width)
    raise ValueError("cloud metrics: mode must be 'kitti2015' or 'eigen', got {!r}".format(mode))


class CloudMetrics:
    """The product behind Test_KITTI.py --cloud-metrics: every frame with ground truth gets the next row of a CloudTable.
    calibration: a callable (frame index, H, W) -> (P, fb), as pseudo_lidar.PseudoLidarWriter takes it.
    The ground-truth cloud is pseudo_lidar.unproject of f.target through P, read as metrics.depth_errors reads it for f.mode (target_fb), with
    depths in (0, max_depth] and no height ceiling.  The predicted cloud is unproject of f.disp with the calibration's fb, the same depth range and no
    ceiling; on="gt" (the default) keeps only the pixels that carry ground truth (target > 0) -- otherwise the accuracy of a dense prediction against
    a sparse scan measures the scan's sparsity -- on="all" keeps every pixel; beams > 0 first reduces the prediction to the nearest point of each of
    beams x az_bins scanner bins.  With f.use_median the prediction's fb is multiplied by the frame's factor of metrics.median_scale.
    Values read from the device per frame: the two point counts that the two unproject calls read, nothing else -- plus the one double of the median
    factor with f.use_median.  The table is read once, by result().  beside: what the JSON line carries next to `key`."""
    key = "cloud"

    def __init__(self, n_frames=1, calibration=None, thresholds=THRESHOLDS, on="gt", beams=0, az_bins=1024, max_depth=80.0, device="cuda", beside=None):
        from . import pseudo_lidar
        if on not in ("gt", "all"):
            raise ValueError("CloudMetrics: on must be 'gt' or 'all', got {!r}".format(on))
        if calibration is None or not callable(calibration):
            raise ValueError("CloudMetrics: calibration must be a callable (frame index, H, W) -> (P, fb)")
        beams, az_bins = int(beams), int(az_bins)
        if beams < 0:
            raise ValueError("CloudMetrics: beams must be >= 0, got {}".format(beams))
        if beams:
            pseudo_lidar.edge_tables(beams, az_bins)  # the range checks, before the first frame
        if not np.isfinite(max_depth) or not max_depth > 0.0:
            raise ValueError("CloudMetrics: max_depth must be finite and positive, got {}".format(max_depth))
        thresholds = check_thresholds(thresholds)
        self.table = CloudTable(n_frames, thresholds, device)
        self.calibration, self.on, self.beams, self.az_bins, self.max_depth = calibration, on, beams, az_bins, float(max_depth)
        self.beside = dict(beside or {})

    def frame(self, f):
        """An inference.Frame with ground truth into the next row; one without is passed over."""
        if f.target is None:
            return
        from . import metrics, pseudo_lidar
        H, W = int(f.disp.shape[-2]), int(f.disp.shape[-1])
        P, fb = self.calibration(f.index, H, W)
        target = f.target.reshape(H, W).to(torch.float32)
        if f.use_median:
            fb = float(fb) * float(metrics.median_scale(f.disp, target, f.mode)[0].item())  # the one extra read
        inf = float("inf")
        gt = pseudo_lidar.unproject(target, P, fb=target_fb(f.mode, W), max_depth=self.max_depth, max_height=inf)
        score, threshold = ((target > 0).to(torch.float32), 0.5) if self.on == "gt" else (None, None)
        pred = pseudo_lidar.unproject(f.disp, P, fb=fb, score=score, threshold=threshold, max_depth=self.max_depth, max_height=inf, beams=self.beams,
                                      az_bins=self.az_bins)
        cloud_errors(pred, gt, out=self.table.row(self.table.n))

    def result(self):
        """CloudTable.result(): the per-frame values and the means over the counted frames -- one read of the table."""
        return self.table.result()

    def summary(self):
        """The run's extra JSON line: the means over the counted frames (one more read of the table)."""
        res = self.result()
        out = {"frames": res["frames"], "thresholds": res["thresholds"], "on": self.on, "beams": self.beams, "max_depth": self.max_depth}
        if self.beams:
            out["az_bins"] = self.az_bins
        for k in ("accuracy", "completeness", "chamfer", "chamfer_l2", "precision", "recall", "f", "n_pred", "n_gt"):
            out[k] = res[k + "_mean"]
        return out
