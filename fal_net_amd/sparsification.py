"""Sparsification curves of the confidence maps on the device (csrc/sort.hip, csrc/sparsify.hip): does a per-pixel score predict the depth error?

The pixels that count for the depth errors are removed in order of decreasing predicted uncertainty and a metric is recomputed on the rest; the
curve is compared with the oracle curve (pixels removed in order of their true error) and with the constant random curve (the metric on all
pixels).  AUSE is the area between score and oracle (lower is better), AURG the area between random and score (higher is better).

  argsort_u32(keys)                         the stable segmented radix argsort behind it (falnet_sort_u32), np.argsort(kind="stable") per segment
  curves(pred_disp, gt, mode, scores, ...)  one frame: n and the abs_rel / rms / d1 curves of every score and of the three oracles, one row of doubles
  SparsificationTable                       (frames, row) doubles on the device, NaN until written, read once; result() forms AUSE / AURG on the host
  SCORES, stats_needed, score_maps          the named scores of Test_KITTI.py --sparsification and how they come out of confidence.stats

The definition is in include/falnet_hip.h (falnet_sparsify) and, as numpy, in tests/_sparsify_ref.py.  The pixel set, the median factor and the
depths are those of metrics.depth_errors.  There is no host fallback: CUDA tensors only."""
import numpy as np
import torch

from . import _lib as L
from .metrics import MODES, _frame, focal_baseline

METRICS = ("abs_rel", "rms", "d1")  # d1 = 1 - a1: every curve falls as the worst pixels go
SCORES = {"std": 1, "entropy": 1, "conf": -1, "relstd": 1}  # +1: larger is more uncertain; -1: larger is more confident
MAX_SCORES, MAX_SEGMENTS, MAX_N = 4, 8, 1 << 24
MIN_STEPS, MAX_STEPS, DEFAULT_STEPS = 2, 100, 50


def row_length(n_scores, steps):
    return 1 + (3 * n_scores + 3) * steps


def check_names(names):
    """The score names of a run, in order; ValueError on an unknown one, a repeated one or none."""
    names = [names] if isinstance(names, str) else list(names)
    bad = [k for k in names if k not in SCORES]
    if bad or not names or len(set(names)) != len(names):
        raise ValueError("sparsification: scores are a subset of {} (each once), got {}".format(",".join(SCORES), names))
    return names


def check_steps(steps):
    steps = int(steps)
    if not MIN_STEPS <= steps <= MAX_STEPS:
        raise ValueError("sparsification: steps must lie in [{}, {}], got {}".format(MIN_STEPS, MAX_STEPS, steps))
    return steps


def stats_needed(names):
    """The statistics confidence.stats has to return for these scores (relstd = std / mean)."""
    need = set()
    for k in check_names(names):
        need |= {"std", "mean"} if k == "relstd" else {k}
    from .confidence import KINDS
    return tuple(k for k in KINDS if k in need)


def score_maps(st, names):
    """confidence.stats output -> {name: (map, sign)} as curves() takes it; relstd is one f32 division on the device."""
    return {k: ((st["std"] / st["mean"]) if k == "relstd" else st[k], SCORES[k]) for k in check_names(names)}


def _cuda(x, what):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("fal_net_amd.sparsification runs on an MI355X only (no CPU fallback); {} is {}".format(
            what, "on " + str(x.device) if torch.is_tensor(x) else type(x).__name__))
    return x


def argsort_u32(keys):
    """keys: (segments, n) or (n,) 32-bit integers on the device, read as unsigned (torch.uint32, or int32 storage of the same bits) -> int32
    tensor of the same shape: along the last axis, the indices that sort the keys ascending, equal keys in index order.  segments <= 8,
    n <= 2^24; `keys` is not modified."""
    _cuda(keys, "keys")
    if keys.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or keys.dim() not in (1, 2):
        raise ValueError("argsort_u32: expected (segments, n) or (n,) int32 / uint32 keys, got {} {}".format(keys.dtype, tuple(keys.shape)))
    segments, n = (1 if keys.dim() == 1 else keys.shape[0]), keys.shape[-1]
    k2 = keys.contiguous().view(torch.int32).reshape(segments, n)
    if not 1 <= segments <= MAX_SEGMENTS or n > MAX_N:
        raise ValueError("argsort_u32: {} segments of {} keys (1 to {} segments, at most 2^24 keys each)".format(segments, n, MAX_SEGMENTS))
    perm = torch.empty_like(k2)
    if n > 0:
        lib = L.lib()
        ws = torch.empty(int(lib.falnet_sort_u32_workspace_bytes(n, segments)) // 8, dtype=torch.int64, device=keys.device)
        L.check(lib.falnet_sort_u32(L.ptr(k2), n, segments, L.ptr(perm), L.ptr(ws), L.stream_ptr()), "sort_u32")
    return perm.view(keys.shape)


class SparsificationRow:
    """Row `index` of a SparsificationTable: what curves() takes as `out`."""

    def __init__(self, table, index):
        self.table, self.index = table, index

    @property
    def tensor(self):
        return self.table.table[self.index]


class SparsificationTable:
    """Owns the results table -- (n_frames, row_length) doubles on the device, NaN where nothing was written -- and the workspaces of the kernels
    (grown to the largest frame seen).  `names`: what the scores of every row are called, in order (at most four); `steps`: the cuts S of every curve.  row(i) hands out row i
    (the table grows on the device when i is beyond it), result() reads everything back ONCE.  extra: what summary() says besides the areas."""
    key = "sparsification"

    def __init__(self, n_frames, names=(), steps=DEFAULT_STEPS, device="cuda", extra=None):
        self.extra = dict(extra or {})
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("fal_net_amd.sparsification runs on an MI355X only (no CPU fallback); asked for " + str(device))
        self.names = [str(k) for k in names]
        if len(self.names) > MAX_SCORES or len(set(self.names)) != len(self.names):
            raise ValueError("sparsification: at most {} scores, each named once, got {}".format(MAX_SCORES, self.names))
        self.steps = check_steps(steps)
        self.width = row_length(len(self.names), self.steps)
        self.table = torch.full((max(int(n_frames), 1), self.width), float("nan"), dtype=torch.float64, device=self.device)
        self.workspace = None  # falnet_sparsify's, sized on first use
        self.metrics_workspace = torch.empty(int(L.lib().falnet_metrics_workspace_bytes()) // 8, dtype=torch.int64, device=self.device)
        self.scale = torch.empty(4, dtype=torch.float64, device=self.device)  # {factor, median gt, median pred, n}: select -> scatter kernel
        self.n = 0  # rows handed out

    def row(self, i):
        if i >= self.table.shape[0]:  # a loader of unknown length: double, on the device (no host read)
            grown = torch.full((max(2 * self.table.shape[0], i + 1), self.width), float("nan"), dtype=torch.float64, device=self.device)
            grown[:self.table.shape[0]] = self.table
            self.table = grown
        self.n = max(self.n, i + 1)
        return SparsificationRow(self, i)

    def workspace_for(self, H, W, n_scores):
        need = int(L.lib().falnet_sparsify_workspace_bytes(H, W, n_scores)) // 8
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(max(need, 1), dtype=torch.int64, device=self.device)
        return self.workspace

    def rows(self):
        """The rows handed out so far as a host array -- one copy, one synchronisation."""
        return self.table[:self.n].cpu().numpy()

    def result(self):
        """One read of the table -> {'rows', 'names', 'metrics', 'steps', 'n': the counted pixels per frame, 'frames': how many frames have
        n >= 1, 'ause' / 'aurg': {score: {metric: per-frame array}} over those frames, 'ause_mean' / 'aurg_mean': {score: {metric: float}},
        'curves_mean': {score: {metric: list of S}}, 'oracle_mean': {metric: list of S}}.  No frame with a pixel: the means are NaN."""
        return summarize(self.rows(), self.names, self.steps)

    def frame(self, f):
        """An inference.Frame with ground truth into the next row; one without is passed over.  The errors are those of `f.disp`, the disparity the
        run evaluates AFTER post-processing; the scores (self.names, from SCORES) are statistics of the logits of one more disparity-only forward
        of the plain view (f.stats): with ms_pp or the flip post-processing the scores describe the first of the two blended forwards."""
        if f.target is None:
            return
        st = f.stats(stats_needed(self.names))
        curves(f.disp, f.target, f.mode, score_maps(st, self.names), use_median=f.use_median, steps=self.steps, out=self.row(self.n))

    def summary(self):
        """The run's extra JSON line: the mean areas per score (one more read of the table)."""
        res = self.result()
        return dict({"scores": res["names"], "steps": res["steps"], "frames": res["frames"], "ause": res["ause_mean"], "aurg": res["aurg_mean"]},
                    **self.extra)


def area(curve):
    """Trapezoid of S samples at spacing 1 / S, in f64: dx * (sum - (first + last) / 2)."""
    curve = np.asarray(curve, np.float64)
    return (1.0 / curve.shape[-1]) * (curve.sum(-1) - (curve[..., 0] + curve[..., -1]) / 2)


def split_row(rows, n_scores, steps):
    """(frames, row_length) -> (n (frames,), score curves (frames, n_scores, 3, S), oracle curves (frames, 3, S))."""
    rows = np.asarray(rows, np.float64).reshape(-1, row_length(n_scores, steps))
    body = rows[:, 1:].reshape(len(rows), n_scores + 1, 3, steps)
    return rows[:, 0], body[:, :n_scores], body[:, n_scores]


def summarize(rows, names, steps):
    n, sc, orc = split_row(rows, len(names), steps)
    ok = n >= 1  # NaN (never written) compares false
    sc, orc = sc[ok], orc[ok]
    with np.errstate(invalid="ignore"):
        ause = area(sc - orc[:, None]) if len(names) else np.zeros((len(sc), 0, 3))
        aurg = area(sc[..., :1] - sc) if len(names) else np.zeros((len(sc), 0, 3))
    mean = lambda a: a.mean(0) if len(a) else np.full(a.shape[1:], np.nan)  # noqa: E731
    per = lambda a: {k: {m: a[:, i, j] for j, m in enumerate(METRICS)} for i, k in enumerate(names)}  # noqa: E731
    avg = lambda a: {k: {m: float(mean(a)[i, j]) for j, m in enumerate(METRICS)} for i, k in enumerate(names)}  # noqa: E731
    return {"rows": np.asarray(rows), "names": list(names), "metrics": list(METRICS), "steps": steps, "n": n, "frames": int(ok.sum()),
            "ause": per(ause), "aurg": per(aurg), "ause_mean": avg(ause), "aurg_mean": avg(aurg),
            "curves_mean": {k: {m: mean(sc)[i, j].tolist() for j, m in enumerate(METRICS)} for i, k in enumerate(names)},
            "oracle_mean": {m: mean(orc)[j].tolist() for j, m in enumerate(METRICS)}}


def curves(pred_disp, gt, mode, scores, use_median=False, min_d=1.0, max_d=None, steps=DEFAULT_STEPS, out=None):
    """One frame -> the row's tensor of 1 + (3 len(scores) + 3) steps doubles on the device: n, then per score (in the dict's order) its
    abs_rel, rms and d1 curves, then the oracle abs_rel, rms and d1 curves.  pred_disp, gt, mode, use_median, min_d, max_d: as
    metrics.depth_errors (with use_median, and always for make3d, the factor comes from falnet_depth_median_scale).  scores: {name: (map, sign)}
    with maps of the frame's size and sign +1 (larger is more uncertain) or -1 (larger is more confident); at most four.  out: a
    SparsificationRow whose table has the same number of scores and the same steps, or None."""
    if mode not in MODES:
        raise ValueError("mode must be one of {}, got {!r}".format(", ".join(MODES), mode))
    pred, H, W = _frame(_cuda(pred_disp, "pred_disp"), "pred_disp")
    g, gh, gw = _frame(_cuda(gt, "gt"), "gt")
    if (gh, gw) != (H, W):
        raise ValueError("pred_disp is {} x {} but gt is {} x {}".format(H, W, gh, gw))
    steps = check_steps(steps)
    if len(scores) > MAX_SCORES:
        raise ValueError("sparsification: at most {} scores, got {}".format(MAX_SCORES, len(scores)))
    sc, keep = L.Scores(), []
    sc.n = len(scores)
    for i, (name, (m, sign)) in enumerate(scores.items()):
        m, mh, mw = _frame(_cuda(m, "score " + str(name)), "score " + str(name))
        if (mh, mw) != (H, W):
            raise ValueError("score {} is {} x {} but the frame is {} x {}".format(name, mh, mw, H, W))
        if sign not in (1, -1):
            raise ValueError("score {}: sign must be +1 or -1, got {!r}".format(name, sign))
        keep.append(m)
        sc.map[i], sc.sign[i] = m.data_ptr(), int(sign)
    if out is None:
        out = SparsificationTable(1, list(scores), steps, pred.device).row(0)
    elif not isinstance(out, SparsificationRow):
        raise TypeError("out must be a SparsificationRow (SparsificationTable.row(i)) or None, got " + type(out).__name__)
    t = out.table
    if t.width != row_length(sc.n, steps):
        raise ValueError("out: the table's rows hold {} doubles, {} scores at {} steps need {}".format(t.width, sc.n, steps, row_length(sc.n, steps)))
    fb = focal_baseline(mode, W)
    max_d = (70.0 if mode == "make3d" else 80.0) if max_d is None else float(max_d)
    lib, scale = L.lib(), None
    if use_median or mode == "make3d":
        scale = t.scale
        L.check(lib.falnet_depth_median_scale(L.ptr(pred), L.ptr(g), H, W, MODES[mode], float(fb), max_d, L.ptr(scale), L.ptr(t.metrics_workspace),
                                              L.stream_ptr()), "depth_median_scale")
    L.check(lib.falnet_sparsify(L.ptr(pred), L.ptr(g), H, W, MODES[mode], float(fb), L.ptr(scale), float(min_d), max_d, sc, steps, L.ptr(out.tensor),
                                L.ptr(t.workspace_for(H, W, sc.n)), L.stream_ptr()), "sparsify")
    return out.tensor
