"""Connected components of a depth or disparity map on the device (csrc/components.hip: falnet_components), and the speckle filter they make: the
pieces of a map smaller than K pixels dropped from a point cloud, a pseudo-LiDAR scan or a mesh.

A pixel is valid when lo < v <= hi (and, with a score map, score >= threshold); two 4-neighbours are joined when both are valid and
max(v) <= min(v) (1 + max_jump) -- the mesh's keep rule, a ratio, so it means the same on a depth and on a disparity.  A pixel's label is the smallest
pixel index of its component (-1 when invalid), its size the component's pixel count (0 when invalid).

  label(map, max_jump, lo, hi, ...)              (labels | None, sizes, info): int32 maps in the input's shape, per image (components, valid, largest)
  size_score(map, ...)                           the sizes as f32: the `score` of mesh.build, pseudo_lidar.unproject or confidence.filter_point_cloud,
                                                 with threshold = K
  filter_point_cloud(img, disp, min_component)   dumps.point_cloud with only the vertices in components of at least K pixels
  ComponentsSummary                              the `components` JSON line of Test_KITTI.py --min-component

The result is defined in include/falnet_hip.h; the numpy restatement it is tested against is tests/_components_ref.py.  Nothing here
needs a GPU to import; `label` does: like the rest of the package it has no CPU fallback and raises on a CPU tensor."""
import torch

MAX_MIN_COMPONENT = 1 << 24  # an f32 holds every size up to here exactly


def check_min_component(value, name="min_component"):
    """A component size threshold, or None for no filter; ValueError unless it is a whole number with 1 <= value <= 2^24."""
    if value is None:
        return value
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 1 <= value <= MAX_MIN_COMPONENT or int(value) != value:  # a NaN fails the range
        raise ValueError("{} must be a whole number in [1, 2^24], got {}".format(name, value))
    return int(value)


def check_jump(max_jump, name="max_jump"):
    """ValueError unless max_jump >= 0 (infinity joins all valid neighbours; a NaN fails the comparison)."""
    if not max_jump >= 0.0:
        raise ValueError("components: {} must be >= 0 (inf joins all valid neighbours), got {}".format(name, max_jump))
    return float(max_jump)


def _maps(x, what, shape=None, device=None):
    """A CUDA (H, W), (B, H, W) or (B, 1, H, W) tensor as contiguous f32."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("fal_net_amd.components.label runs on an MI355X only (no CPU fallback); {} is {}".format(
            what, "on " + str(x.device) if torch.is_tensor(x) else type(x).__name__))
    if x.dim() not in (2, 3, 4) or (x.dim() == 4 and x.shape[1] != 1):
        raise ValueError("components: {} must be (H, W), (B, H, W) or (B, 1, H, W), got {}".format(what, tuple(x.shape)))
    if shape is not None and (tuple(x.shape) != shape or x.device != device):
        raise ValueError("components: {} {} on {} does not match the map {} on {}".format(what, tuple(x.shape), x.device, shape, device))
    return x.detach().to(torch.float32).contiguous()


def label(map, max_jump=0.05, lo=0.0, hi=float("inf"), score=None, threshold=None, want_labels=True):
    """map: (H, W), (B, H, W) or (B, 1, H, W) CUDA f32 -> (labels, sizes, info): labels (None with want_labels=False) and sizes int32 in the map's
    shape on its device, info = [(components, valid pixels, largest component)] per image.  score (the map's shape) and threshold go together.  One
    falnet_components call for the whole batch, then ONE host read: the 3 B + 1 info words.  RuntimeError when the kernels report a cut loop."""
    from . import _lib as L
    m = _maps(map, "map")
    if (score is None) != (threshold is None):
        raise ValueError("components.label: score and threshold go together")
    sc = None if score is None else _maps(score, "score", tuple(map.shape), map.device)
    ratio = 1.0 + check_jump(float(max_jump))  # in double; the c_float argument rounds it once
    lo, hi = float(lo), float(hi)
    if not 0.0 <= lo < hi:
        raise ValueError("components.label: need 0 <= lo < hi (hi may be inf), got {} and {}".format(lo, hi))
    H, W = int(m.shape[-2]), int(m.shape[-1])
    B = m.numel() // max(H * W, 1)
    lib = L.lib()
    ws_bytes = int(lib.falnet_components_workspace_bytes(B, H, W))
    if ws_bytes <= 0:
        raise ValueError("components.label: {} maps of {} x {} are outside what falnet_components takes (B >= 1, 1 <= H W < 2^30, B H W < 2^31)".format(B, H, W))
    dev = m.device
    labels = torch.empty(m.shape, dtype=torch.int32, device=dev) if want_labels else None
    sizes = torch.empty(m.shape, dtype=torch.int32, device=dev)
    info = torch.empty(3 * B + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.falnet_components(L.ptr(m), L.ptr(sc), 0.0 if threshold is None else float(threshold), lo, hi, ratio, B, H, W, L.ptr(labels), L.ptr(sizes),
                                      L.ptr(info), L.ptr(ws), L.stream_ptr()), "components")
    words = info.cpu().tolist()  # the one read
    if words[-1] != 0:
        raise RuntimeError("components.label: the kernels cut a loop short (status {}): the labels are not valid".format(words[-1]))
    return labels, sizes, [tuple(words[3 * b:3 * b + 3]) for b in range(B)]


def size_score(map, max_jump=0.05, lo=0.0, hi=float("inf"), score=None, threshold=None):
    """The component size of every pixel as f32, in the map's shape: exact below 2^24 and monotone above, so `score=size_score(...), threshold=K` with
    K <= 2^24 keeps exactly the pixels in components of at least K pixels (an invalid pixel has size 0)."""
    return label(map, max_jump, lo, hi, score, threshold, want_labels=False)[1].to(torch.float32)


def filter_point_cloud(img, disp, min_component, max_jump=0.05, lo=0.0, hi=float("inf"), score=None, threshold=None, **kw):
    """confidence.filter_point_cloud(img, disp, sizes, K, ...) with the component sizes of `disp` (B, 1, H, W): only the vertices in components of at
    least `min_component` pixels, in pixel order.  score / threshold enter the components, not the cloud."""
    from . import confidence
    K = check_min_component(min_component)
    if K is None:
        raise ValueError("components.filter_point_cloud: min_component is needed")
    sizes = size_score(disp, max_jump, lo, hi, score, threshold)
    return confidence.filter_point_cloud(img, disp, sizes, float(K), **kw)


class ComponentsSummary:
    """Test_KITTI.py --min-component K: the run's `components` JSON line.  frame() labels the disparity the run evaluates with every positive finite
    value valid (no depth bound, no confidence: the writers apply their own) and keeps the frame's numbers; what stays on the device until
    summary() is the count of valid pixels in components below K."""
    key = "components"

    def __init__(self, min_component, max_jump=0.05):
        self.min_component, self.max_jump = check_min_component(min_component), check_jump(max_jump)
        if self.min_component is None:
            raise ValueError("ComponentsSummary: min_component is needed")
        self.frames = self.components = self.valid = self.largest = 0
        self._small, self._valid = [], []

    def frame(self, f):
        """An inference.Frame: `f.disp`, the disparity the run evaluates."""
        self.add(f.disp)

    def add(self, disp):
        _, sizes, info = label(disp, self.max_jump, want_labels=False)
        self._small.append(((sizes > 0) & (sizes < self.min_component)).reshape(len(info), -1).sum(1))
        for comps, valid, largest in info:
            self.frames += 1
            self.components += comps
            self.valid += valid
            self._valid.append(valid)
            self.largest = max(self.largest, largest)
        return info

    def summary(self):
        """frames, mean components and valid pixels per frame, the mean over the frames of the share of a frame's valid pixels that lie in components
        below K (a frame without a valid pixel counts as 0), the largest component of the run."""
        nan = float("nan")
        small = torch.cat(self._small).cpu().tolist() if self._small else []  # one read of the device
        shares = [s / v if v else 0.0 for s, v in zip(small, self._valid)]
        return {"frames": self.frames, "min_component": self.min_component, "max_jump": self.max_jump,
                "mean_components": self.components / self.frames if self.frames else nan, "mean_valid": self.valid / self.frames if self.frames else nan,
                "mean_small_share": sum(shares) / len(shares) if shares else nan, "largest": self.largest}
