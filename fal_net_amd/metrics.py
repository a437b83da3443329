"""Evaluation metrics computed on the device (csrc/metrics.hip): the KITTI / Make3D depth errors with optional median scaling, the end-point
error and the view errors (RMSE / MAE / PSNR) -- what `inference.evaluate` and `train.validate` otherwise compute per frame on the host
(myUtils.disps_to_depths_* + compute_kitti_errors in float64 numpy after two full-size copies, loss_functions.realEPE, myUtils.get_rmse).

A frame's numbers land in one row of a device-resident table of doubles (`MetricTable`); nothing is copied to the host per frame and the table is
read once, with `.result()`.  The per-pixel arithmetic of the depth chain is f64 in the host's order (its threshold counts equal numpy's as
integers) and every reduction is deterministic: two calls on the same inputs give bit-identical rows.

There is no host fallback: every function here takes CUDA tensors and raises on anything else.  The camera constants come from
myUtils.width_to_focal / width_to_baseline (KeyError on a width that is not a KITTI width, as in the host chain)."""
import numpy as np
import torch

from . import _lib as L
from .myUtils import kitti_error_names, make_error_names, width_to_baseline, width_to_focal

MEAN = (0.411, 0.432, 0.45)  # Train_Stage1_K.py:127 -- what the loader subtracted
MODES = {"kitti2015": 0, "eigen": 1, "make3d": 2}  # FALNET_DEPTH_* of include/falnet_hip.h
ROW = 24  # FALNET_MET_ROW; the columns (FALNET_MET_*):
COLUMNS = ("abs_rel", "sq_rel", "rms", "log_rms", "a1", "a2", "a3", "n", "n_a1", "n_a2", "n_a3", "scale", "median_gt", "median_pred",
           "epe", "epe_n", "rmse", "mea", "psnr", "view_sum_sq", "view_sum_abs", "view_sum_rsq", "view_n", "ssim")
COL = {name: i for i, name in enumerate(COLUMNS)}
_GROUP_COLUMN = {"depth": COL["n"], "epe": COL["epe_n"], "view": COL["view_n"]}  # a group's count column: NaN until the group is written
# ('ssim' is a group of one column, written by csrc/ssim.hip: MetricTable.result() filters it on the column itself)


def focal_baseline(mode, width):
    """focal * baseline exactly as the host chain forms it: width_to_focal[w] * 0.54 (disps_to_depths_kitti2015), width_to_focal[w] *
    width_to_baseline[w] (disps_to_depths_kitti), 721 * 0.22 (disps_to_depths_make: no table)."""
    if mode == "kitti2015":
        return width_to_focal[width] * 0.54
    if mode == "eigen":
        return width_to_focal[width] * width_to_baseline[width]
    if mode == "make3d":
        return 721 * 0.22
    raise ValueError("mode must be one of {}, got {!r}".format(", ".join(MODES), mode))


def _map(x, what):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("fal_net_amd.metrics runs on an MI355X only (no CPU fallback); {} is {}".format(
            what, "on " + str(x.device) if torch.is_tensor(x) else type(x).__name__))
    return x.detach().to(torch.float32).contiguous()


def _frame(x, what):
    """(H, W), (1, H, W) or (1, 1, H, W) -> contiguous f32 map and its size (the evaluation loops run at batch size 1: KITTI mixes sizes)."""
    x = _map(x, what)
    if x.dim() < 2 or x.numel() != x.shape[-2] * x.shape[-1]:
        raise ValueError("{}: expected one H x W map, got {}".format(what, tuple(x.shape)))
    return x, int(x.shape[-2]), int(x.shape[-1])


class MetricRow:
    """Row `index` of a MetricTable: what the metric functions take as `out`."""

    def __init__(self, table, index):
        self.table, self.index = table, index

    @property
    def tensor(self):
        """The row's ROW doubles on the device (a view of the table)."""
        return self.table.table[self.index]


class MetricTable:
    """Owns the results table -- (n_frames, ROW) doubles on the device, NaN where nothing was written -- and the workspace of the kernels.
    `row(i)` hands out row i (the table grows on the device when i is beyond it), `result()` reads everything back ONCE."""

    def __init__(self, n_frames, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("fal_net_amd.metrics runs on an MI355X only (no CPU fallback); asked for " + str(device))
        self.table = torch.full((max(int(n_frames), 1), ROW), float("nan"), dtype=torch.float64, device=self.device)
        self.workspace = torch.empty(int(L.lib().falnet_metrics_workspace_bytes()) // 8, dtype=torch.int64, device=self.device)
        self.scale = torch.empty(4, dtype=torch.float64, device=self.device)  # {factor, median gt, median pred, n}: select -> error kernel
        self.n = 0  # rows handed out
        self._ssim_ws = None  # partial sums of csrc/ssim.hip: one word per tile of the largest frame so far

    def ssim_workspace(self, nbytes):
        if self._ssim_ws is None or self._ssim_ws.numel() * 8 < nbytes:
            self._ssim_ws = torch.empty(max((int(nbytes) + 7) // 8, 1), dtype=torch.int64, device=self.device)
        return self._ssim_ws

    def row(self, i):
        if i >= self.table.shape[0]:  # a loader of unknown length: double, on the device (no host read)
            grown = torch.full((max(2 * self.table.shape[0], i + 1), ROW), float("nan"), dtype=torch.float64, device=self.device)
            grown[:self.table.shape[0]] = self.table
            self.table = grown
        self.n = max(self.n, i + 1)
        return MetricRow(self, i)

    def rows(self):
        """The rows handed out so far as a host array -- one copy, one synchronisation."""
        return self.table[:self.n].cpu().numpy()

    def running_mean(self, column):
        """Mean of `column` over the rows of its group written so far (a read of the table: for the iterations of a loop that print)."""
        rows = self.rows()
        col = COL[column] if isinstance(column, str) else column
        group = "depth" if col < COL["epe"] else ("epe" if col < COL["rmse"] else "view")
        vals = rows[~np.isnan(rows[:, col if col == COL["ssim"] else _GROUP_COLUMN[group]]), col]
        return float(np.mean(vals)) if len(vals) else 0.0

    def result(self, make3d=False):
        """{'rows': (n, ROW) array, 'names': the seven depth names, 'depth' / 'epe' / 'view': per-frame rows of each group that was written
        (frames in order), 'depth_mean', 'epe_mean', 'rmse_mean', 'mea_mean', 'psnr_mean': their means over those frames, 'ssim': the SSIM of
        the frames it was written for (in order), 'ssim_mean'}.  A group never written has no rows and a mean of 0, like an AverageMeter that
        was never updated."""
        rows = self.rows()
        written = {g: ~np.isnan(rows[:, c]) for g, c in _GROUP_COLUMN.items()}  # the count column is a finite number once a group is written
        depth, epe, view = rows[written["depth"]][:, :7], rows[written["epe"]][:, COL["epe"]], rows[written["view"]][:, COL["rmse"]:COL["psnr"] + 1]
        mean = lambda a: a.mean(0) if len(a) else np.zeros(a.shape[1:])
        vm = mean(view)
        ssim_col = rows[:, COL["ssim"]]
        ssim_vals = ssim_col[~np.isnan(ssim_col)]
        return {"rows": rows, "names": list(make_error_names if make3d else kitti_error_names), "depth": depth, "epe": epe, "view": view,
                "depth_mean": mean(depth), "epe_mean": float(mean(epe)), "rmse_mean": float(vm[0]), "mea_mean": float(vm[1]), "psnr_mean": float(vm[2]),
                "ssim": ssim_vals, "ssim_mean": float(mean(ssim_vals))}


def _out(out, device):
    """out=None: a table of one row of its own; a MetricRow: that row (and its table's workspace)."""
    if out is None:
        return MetricTable(1, device).row(0)
    if not isinstance(out, MetricRow):
        raise TypeError("out must be a MetricRow (MetricTable.row(i)) or None, got " + type(out).__name__)
    return out


def depth_errors(pred_disp, gt, mode, use_median=False, min_d=1.0, max_d=None, out=None):
    """compute_kitti_errors(*disps_to_depths_<mode>(gt, pred_disp)) of one frame on the device -> the row's tensor (columns COLUMNS; the seven
    metrics first, in the order of kitti_error_names / make_error_names).  mode: 'kitti2015' (gt is a disparity), 'eigen' (Eigen crop, gt is a
    depth), 'make3d' (compute_make_errors: mask 0 < gt < max_d, always median-scaled, log10 term).  max_d defaults to 80, make3d 70."""
    if mode not in MODES:
        raise ValueError("mode must be one of {}, got {!r}".format(", ".join(MODES), mode))
    pred, H, W = _frame(pred_disp, "pred_disp")
    g, gh, gw = _frame(gt, "gt")
    if (gh, gw) != (H, W):
        raise ValueError("pred_disp is {} x {} but gt is {} x {}".format(H, W, gh, gw))
    fb = focal_baseline(mode, W)
    max_d = (70.0 if mode == "make3d" else 80.0) if max_d is None else float(max_d)
    row = _out(out, pred.device)
    t, lib = row.table, L.lib()
    scale = None
    if use_median or mode == "make3d":
        scale = t.scale
        L.check(lib.falnet_depth_median_scale(L.ptr(pred), L.ptr(g), H, W, MODES[mode], float(fb), max_d, L.ptr(scale), L.ptr(t.workspace),
                                              L.stream_ptr()), "depth_median_scale")
    L.check(lib.falnet_depth_errors(L.ptr(pred), L.ptr(g), H, W, MODES[mode], float(fb), L.ptr(scale), float(min_d), max_d, L.ptr(row.tensor),
                                    L.ptr(t.workspace), L.stream_ptr()), "depth_errors")
    return row.tensor


def median_scale(pred_disp, gt, mode, max_d=None):
    """{factor, median of gt[mask], median of pred[mask], n} of one frame as 4 doubles on the device: np.median(gt) / np.median(pred) of the
    depths the host chain forms, exact."""
    pred, H, W = _frame(pred_disp, "pred_disp")
    g, gh, gw = _frame(gt, "gt")
    if (gh, gw) != (H, W):
        raise ValueError("pred_disp is {} x {} but gt is {} x {}".format(H, W, gh, gw))
    t = MetricTable(1, pred.device)
    max_d = (70.0 if mode == "make3d" else 80.0) if max_d is None else float(max_d)
    L.check(L.lib().falnet_depth_median_scale(L.ptr(pred), L.ptr(g), H, W, MODES[mode], float(focal_baseline(mode, W)), max_d, L.ptr(t.scale),
                                              L.ptr(t.workspace), L.stream_ptr()), "depth_median_scale")
    return t.scale


def epe(pred_disp, target, sparse, out=None):
    """realEPE(pred_disp, target, sparse) on the device: pred_disp (B, 1, h, w) sampled bilinearly (align_corners=True) at the size of target
    (B, 1, H, W); mean |target - up| over target != 0 (sparse) or everywhere -> the row's tensor (columns 'epe', 'epe_n')."""
    pred, target = _map(pred_disp, "pred_disp"), _map(target, "target")
    if pred.dim() != 4 or target.dim() != 4 or pred.shape[1] != 1 or target.shape[1] != 1 or pred.shape[0] != target.shape[0]:
        raise ValueError("epe: expected (B, 1, h, w) and (B, 1, H, W), got {} and {}".format(tuple(pred.shape), tuple(target.shape)))
    row = _out(out, pred.device)
    B, _, H, W = target.shape
    L.check(L.lib().falnet_epe(L.ptr(pred), pred.shape[2], pred.shape[3], L.ptr(target), B, H, W, int(bool(sparse)), L.ptr(row.tensor),
                               L.ptr(row.table.workspace), L.stream_ptr()), "epe")
    return row.tensor


def view_errors(p_im, right, mean=MEAN, out=None):
    """get_rmse / get_mea / get_psnr of the synthesised view p_im against the real one, both (B, 3, H, W) normalised by `mean`, on the device
    -> the row's tensor (columns 'rmse', 'mea', 'psnr' and the sums behind them)."""
    x, y = _map(p_im, "p_im"), _map(right, "right")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape != y.shape:
        raise ValueError("view_errors: expected two (B, 3, H, W) images, got {} and {}".format(tuple(x.shape), tuple(y.shape)))
    row = _out(out, x.device)
    B, _, H, W = x.shape
    L.check(L.lib().falnet_view_errors(L.ptr(x), L.ptr(y), float(mean[0]), float(mean[1]), float(mean[2]), B, H, W, L.ptr(row.tensor),
                                       L.ptr(row.table.workspace), L.stream_ptr()), "view_errors")
    return row.tensor


def ssim(p_im, right, mean=MEAN, out=None):
    """Structural similarity (Wang et al. 2004: 11 x 11 Gaussian window of sigma 1.5, valid windows, data range 255) of the synthesised view p_im
    against the real one, both (B, 3, H, W) normalised by `mean`, on get_psnr's operands round(clamp(255 (p_im + mean), 0, 255)) and 255 (right +
    mean); window sums in f64 on the device -> the row's tensor (column 'ssim': the mean over the B * 3 * (H - 10) * (W - 10) windows)."""
    x, y = _map(p_im, "p_im"), _map(right, "right")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape != y.shape:
        raise ValueError("ssim: expected two (B, 3, H, W) images, got {} and {}".format(tuple(x.shape), tuple(y.shape)))
    row = _out(out, x.device)
    B, _, H, W = x.shape
    lib = L.lib()
    ws = row.table.ssim_workspace(lib.falnet_ssim_workspace_bytes(B, 3, H, W, 5))  # (a frame too small for one window: the kernel's error below)
    L.check(lib.falnet_ssim_metric(L.ptr(x), L.ptr(y), float(mean[0]), float(mean[1]), float(mean[2]), B, H, W, L.ptr(row.tensor), L.ptr(ws),
                                   L.stream_ptr()), "ssim_metric")
    return row.tensor
