"""Per-pixel statistics of the MED head's distribution over the disparity planes, and point clouds filtered by them (csrc/med_stats.hip,
csrc/compact.hip; inference only, no gradient).

The forward reduces each pixel's distribution p_n over the N planes to its expectation; this module reads more out of the same logits:

  mean     sum p_n d_n, the forward's `disp`             std      sqrt(sum p_n (d_n - mean)^2) in pixels
  entropy  -sum p_n ln p_n / ln N, in [0, 1]             arg      the first index of the largest logit
  conf     the probability mass on arg - 1 .. arg + 1    peak     the expectation over those planes alone (no "flying pixels" at depth edges)

  stats(dlog0, min_disp, max_disp, which)                    the raw wrapper of falnet_med_stats_fwd: one launch for any subset
  from_model(model, left, min_disp, max_disp, which)         one no_grad disparity-only forward of the model, then stats over its logits
  compact(records, score, threshold)                         ordered stream compaction (falnet_compact_records) of 4- or 15-byte records
  filter_point_cloud(img, disp, score, threshold, ...)       dumps.point_cloud, then only the vertices with score >= threshold
  StatsWriter                                                 stats/<frame>_<kind>.png and the filtered Point_cloud/<frame>.ply of Test_KITTI.py

There is no host fallback: CUDA tensors only."""
import os

import torch

from . import _lib as L
from . import med_logits as M
from .med_logits import MAX_PLANES  # noqa: F401  (part of this module's interface)

KINDS = ("mean", "std", "entropy", "arg", "conf", "peak")  # bit k of `which` is KINDS[k]


def which_bits(which):
    """The names in `which` as the bit mask of falnet_med_stats_fwd and in the order the launch writes them; ValueError on an unknown name, a
    repeated one or none at all."""
    names = [which] if isinstance(which, str) else list(which)
    bad = [k for k in names if k not in KINDS]
    if bad:
        raise ValueError("confidence: unknown statistic(s) {}: choose from {}".format(", ".join(map(str, bad)), ", ".join(KINDS)))
    if not names or len(set(names)) != len(names):
        raise ValueError("confidence: `which` must name at least one statistic and each only once, got {}".format(names))
    bits = sum(1 << KINDS.index(k) for k in names)
    return bits, [k for k in KINDS if k in names]


def stats(dlog0, min_disp, max_disp, which=("std", "conf", "peak")):
    """dlog0 (B, N, H, W) planar f32 logits, min_disp / max_disp: B values in pixels -> {name: (B, 1, H, W) f32} for the names in `which`.
    Every argument is checked before the launch."""
    bits, order = which_bits(which)
    (dlog0, _, mn, mx), (B, N, H, W) = M.check_logits("confidence.stats", dlog0, min_disp, max_disp)
    out = torch.empty(B, len(order), H, W, dtype=torch.float32, device=dlog0.device)
    L.check(L.lib().falnet_med_stats_fwd(L.ptr(dlog0), L.ptr(mn), L.ptr(mx), bits, L.ptr(out), B, N, H, W, L.stream_ptr()), "med_stats_fwd")
    return {k: out[:, i:i + 1] for i, k in enumerate(order)}


def from_model(model, left, min_disp, max_disp, which=("std", "conf", "peak")):
    """One no_grad disparity-only forward of `model` (FAL_netA / B / C, any compute dtype: the logits are planar f32 in all of them), then the
    statistics of the plan's own logits with the plan's prologue-processed min_disp / max_disp.  -> (stats as stats(), the forward's disparity
    (B, 1, H, W))."""
    which_bits(which)
    with torch.no_grad():
        buf, disp = M.forward_logits(model, left, min_disp, max_disp)
        st = stats(buf["dlog0"], buf["min_disp"], buf["max_disp"], which)
    return st, disp


def compact(records, score, threshold, count=None, workspace=None):
    """Ordered stream compaction on the device: records (n, 15) u8 or (n,) of a 4-byte type, score (n,) f32 -> (out, count): `out` has the
    shape of `records`, its first count[0] records are the ones with score >= threshold in index order (a NaN score is dropped), the rest of
    it is not written; `count` is a 1-element int64 tensor on the device (nothing is read back here)."""
    if not (records.is_cuda and score.is_cuda):
        raise RuntimeError("fal_net_amd.confidence runs on an MI355X only (no CPU fallback)")
    n = score.numel()
    rec_bytes = records.element_size() if records.dim() == 1 else records.shape[-1] * records.element_size()
    if rec_bytes not in (4, 15) or records.numel() * records.element_size() != n * rec_bytes or n < 1:
        raise ValueError("confidence.compact: {} records of {} bytes for {} scores (records of 4 or 15 bytes, one score each)".format(
            records.shape[0] if records.dim() else 0, rec_bytes, n))
    if not records.is_contiguous():
        raise ValueError("confidence.compact: records must be contiguous")
    score = M.f32(score, "score", "confidence").reshape(-1)
    lib = L.lib()
    out = torch.empty_like(records)
    count = torch.empty(1, dtype=torch.int64, device=records.device) if count is None else count
    if workspace is None:
        workspace = torch.empty(max(int(lib.falnet_compact_workspace_bytes(n)) // 8, 1), dtype=torch.int64, device=records.device)
    L.check(lib.falnet_compact_records(L.ptr(records), rec_bytes, L.ptr(score), float(threshold), n, L.ptr(out), L.ptr(count), L.ptr(workspace),
                                       L.stream_ptr()), "compact_records")
    return out, count


def filter_point_cloud(img, disp, score, threshold, packed=True, focal=None, baseline=None, **kw):
    """dumps.point_cloud(img, disp, focal, baseline, packed, ...) with only the vertices whose score (B, 1, H, W) is >= threshold, in pixel
    order.  -> (kept, counts): per sample b, kept[b] is (counts[b], 15) u8 PLY records (packed) or (6, counts[b]) f32 rows x, z, -y, r, g, b;
    the B counts come to the host in one copy, after every launch."""
    from . import dumps
    pc = dumps.point_cloud(img, disp, focal, baseline, packed=packed, **kw)
    B, n = pc.shape[0], disp.shape[-2] * disp.shape[-1]
    if tuple(score.shape) != (B, 1) + tuple(disp.shape[-2:]):
        raise ValueError("confidence.filter_point_cloud: score {} does not match the disparity {}".format(tuple(score.shape), tuple(disp.shape)))
    score = M.f32(score, "score", "confidence").view(B, n)
    counts = torch.empty(B, dtype=torch.int64, device=pc.device)
    ws = torch.empty(max(int(L.lib().falnet_compact_workspace_bytes(n)) // 8, 1), dtype=torch.int64, device=pc.device)
    outs = []
    for b in range(B):
        if packed:
            outs.append(compact(pc[b].contiguous(), score[b], threshold, counts[b:b + 1], ws)[0])
        else:  # the six rows are six compactions by the same scores
            outs.append(torch.stack([compact(pc[b, r], score[b], threshold, counts[b:b + 1], ws)[0] for r in range(6)]))
    kept = counts.cpu().tolist()  # the one copy
    return [o[:c] if packed else o[:, :c] for o, c in zip(outs, kept)], kept


def check_min_conf(value, name="min_conf"):
    """A confidence threshold, or None for no filter; ValueError unless 0 < value <= 1 (a NaN fails both comparisons)."""
    if value is not None and not 0.0 < value <= 1.0:
        raise ValueError("{} must lie in (0, 1], got {}".format(name, value))
    return value


class StatsWriter:
    """Test_KITTI.py --stats / --pc-min-conf: writes stats/{frame:010d}_{kind}.png under `save_path` -- std and peak through dumps.disparity_png
    (plasma, p95-normalised), entropy and conf through dumps.feature_u8, arg as the grey rint(255 a / (N - 1)) -- and, with `pc_min_conf`, the
    frame's point cloud with only the vertices of conf >= pc_min_conf as Point_cloud/{frame:010d}.ply (the PLY header carries the kept count).
    Its folder is its own, as dumps.SweepWriter's: FrameWriter and DUMP_KINDS do not know about it.  The means of std, entropy and conf of
    every frame stay on the device until summary()."""
    CLI_KINDS = ("std", "entropy", "arg", "conf", "peak")
    key = "stats"

    def __init__(self, save_path, kinds=(), pc_min_conf=None, ply_format="binary"):
        bad = [k for k in kinds if k not in self.CLI_KINDS]
        if bad:
            raise ValueError("unknown statistic(s) {}: choose from {}".format(", ".join(bad), ", ".join(self.CLI_KINDS)))
        check_min_conf(pc_min_conf, "pc_min_conf")
        self.save_path, self.kinds, self.pc_min_conf, self.ply_format = save_path, tuple(kinds), pc_min_conf, ply_format
        self.folder = os.path.join(save_path, "stats")
        self.pc_folder = os.path.join(save_path, "Point_cloud")
        if self.kinds:
            os.makedirs(self.folder, exist_ok=True)
        if pc_min_conf is not None:
            os.makedirs(self.pc_folder, exist_ok=True)
        self.files = self.frames = self.kept = self.vertices = 0
        self._means = []

    @property
    def which(self):
        """What a frame's stats() has to hold: the kinds written, the three the summary averages, conf for the filter."""
        need = set(self.kinds) | ({"std", "entropy", "conf"} if self.kinds else set()) | ({"conf"} if self.pc_min_conf is not None else set())
        return tuple(k for k in KINDS if k in need)

    def file(self, i, kind):
        return os.path.join(self.folder, "{:010d}_{}.png".format(i, kind))

    def frame(self, f):
        """An inference.Frame: the statistics of the logits of one more disparity-only forward (f.stats); the filtered point cloud is made of
        `f.disp`, the disparity the run evaluates."""
        st = f.stats(self.which)
        B, _, H, W = f.left.shape
        self.write(f.index, f.left, f.disp, st, f.model._plan(B, H, W, f.left.device).buf["dlog0"].shape[1])

    def write(self, i, left, disp, st, n_planes):
        """Frame `i` (batch size 1): left (1, 3, H, W) normalised input, disp (1, 1, H, W) the disparity the cloud is made of, st: stats() with
        at least self.which, n_planes: N."""
        from PIL import Image
        from . import dumps
        for k in self.kinds:
            if k in ("std", "peak"):
                img = dumps.disparity_png(st[k])[0]
            elif k == "arg":
                img = torch.round(st[k][0, 0] * 255.0 / float(n_planes - 1)).to(torch.uint8)
            else:
                img = dumps.feature_u8(st[k])[0, 0]
            Image.fromarray(img.cpu().numpy()).save(self.file(i, k))
            self.files += 1
        if self.kinds:
            self._means.append(torch.stack([st[k].mean() for k in ("std", "entropy", "conf")]))
        if self.pc_min_conf is not None:
            focal, baseline = dumps.camera_for_width(disp.shape[-1])
            packed = self.ply_format == "binary"
            kept, counts = filter_point_cloud(left, disp, st["conf"], self.pc_min_conf, packed=packed, focal=focal, baseline=baseline)
            name = os.path.join(self.pc_folder, "{:010d}.ply".format(i))
            if packed:
                dumps.save_ply(name, packed=kept[0].cpu().numpy(), ply_format="binary")
            else:
                dumps.save_ply(name, planar=kept[0].cpu().numpy(), ply_format="ascii")
            self.kept += counts[0]
            self.vertices += disp.shape[-2] * disp.shape[-1]
        self.frames += 1

    def summary(self):
        """The run's extra JSON line: the means over all frames (one read of the device), the files written, the kept fraction of the clouds."""
        out = {"frames": self.frames}
        if self.kinds:
            m = torch.stack(self._means).mean(0).tolist() if self._means else [float("nan")] * 3
            out.update({"kinds": list(self.kinds), "files": self.files, "mean_std": m[0], "mean_entropy": m[1], "mean_conf": m[2]})
        if self.pc_min_conf is not None:
            out.update({"pc_min_conf": self.pc_min_conf, "pc_kept": self.kept, "pc_vertices": self.vertices,
                        "pc_kept_fraction": self.kept / self.vertices if self.vertices else float("nan")})
        return out
