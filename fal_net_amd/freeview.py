"""Free-viewpoint rendering from the logits of one forward (csrc/med_pose.hip; inference only, no gradient).

The network's probability volume over N fronto-parallel disparity planes plus the left image is a multiplane image of the scene.  Plane n is
the plane Z = fx b / s_n of the left camera (s_n = d_n (W - 1) / W, the head's table), and each plane induces a homography between a target
camera and the left image, so any nearby camera -- off the baseline, dollied, turned, zoomed -- is one more plane sweep.  `views.sweep` is
the special case "identity rotation, centre on the x axis".

  camera(H, W, fx, fy, cx, cy)                   the source intrinsics K (nominal KITTI camera by default)
  pose(K, centre, yaw, pitch, roll, zoom, K_t)   the 12 float64 values (A, E) of one target camera; centre in BASELINES, angles in degrees
  paths.orbit / paths.dolly / paths.pan          lists of pose() keyword sets for n frames
  warp(dlog0, left, min_disp, max_disp, poses)   the raw wrapper of falnet_med_pose_fwd (launches of at most 8 poses)
  render(model, left, min_disp, max_disp, poses) one no_grad disparity-only forward of the model, then warp over its logits
  fill_views(out, max_disp, beta)                the holes of warp()'s views and disparities filled from the background (fal_net_amd/inpaint.py)
  FreeviewWriter(save_path)                      Freeview/{frame:010d}_p{pose:02d}.png and ..._cover.png (write_filled: ..._filled.png)

Geometry: target camera with centre c (source-camera coordinates), rotation R (X_t = R (X_s - c)) and intrinsics K_t:
    A = K R^T K_t^-1      E = K c / (fx b)
target pixel (x, y): q = A (x, y, 1), u0 = q_x / q_z, v0 = q_y / q_z; plane n is sampled at u_n = s_n E_x + w_n u0, v_n = s_n E_y + w_n v0,
w_n = 1 - s_n E_z, iff q_z > 0 and w_n > 0.  Check: R = I, K_t = K, c = (t b, 0, 0) gives A = I, E = (t, 0, 0), u_n = x + t s_n, v_n = y --
the sweep's view t.  Outputs: view = sum_n P_n bilinear(left), disp = sum_n d_n P_n, cover = sum_n P_n omega_n in [0, 1] (omega_n: the
bilinear weights of the taps inside the image): cover says where the view is extrapolated rather than seen.

There is no host fallback: CUDA tensors only."""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import med_logits as M
from .med_logits import MAX_PLANES  # noqa: F401  (part of this module's interface)

MAX_POSES = 8      # poses per launch (PO_MAXV of csrc/med_pose.hip)
OUTPUTS = ("view", "disp", "cover")


def camera(H, W, fx=None, fy=None, cx=None, cy=None):
    """K (3, 3) float64 of the source camera.  Defaults: the focal length of myUtils.width_to_focal where the width is in the table, else
    721.5377 W / 1242 (the 1242-pixel KITTI camera scaled to the width); fy = fx; the principal point at ((W - 1) / 2, (H - 1) / 2)."""
    from .myUtils import width_to_focal
    if fx is None:
        fx = width_to_focal[W] if W in width_to_focal else 721.5377 * W / 1242
    fy = fx if fy is None else fy
    cx = (W - 1) / 2 if cx is None else cx
    cy = (H - 1) / 2 if cy is None else cy
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)


def rotation(yaw=0.0, pitch=0.0, roll=0.0):
    """R = Rz(roll) Ry(yaw) Rx(pitch), angles in degrees, float64 (x right, y down, z forward; X_t = R (X_s - c))."""
    y, p, r = (math.radians(float(a)) for a in (yaw, pitch, roll))
    rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]], dtype=np.float64)
    ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]], dtype=np.float64)
    rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]], dtype=np.float64)
    return rz @ ry @ rx


def pose(K, centre=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, roll=0.0, zoom=1.0, K_t=None):
    """The 12 float64 values (A row-major, then E) of one target camera.  centre: its position in the source camera's frame in BASELINES
    (E = K c / (fx b) depends on c / b only); yaw, pitch, roll in degrees; zoom scales the target focal lengths (of K_t, default K)."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    Kt = np.array(K if K_t is None else K_t, dtype=np.float64).reshape(3, 3)
    Kt[0, 0] *= float(zoom)
    Kt[1, 1] *= float(zoom)
    A = K @ rotation(yaw, pitch, roll).T @ np.linalg.inv(Kt)
    E = K @ np.asarray(centre, dtype=np.float64).reshape(3) / K[0, 0]
    return np.concatenate([A.reshape(9), E])


class paths:
    """Camera paths as lists of pose() keyword sets, n frames each (pure host helpers)."""

    @staticmethod
    def orbit(n, rx, ry, yaw=0.0, pitch=0.0):
        """Frame i sits at (rx cos a, ry sin a, 0) baselines, a = 2 pi i / n: the first at (rx, 0, 0), the last one step before the loop
        closes.  yaw / pitch (degrees) toe the camera in towards the scene: frame i turns by yaw cos a and pitch sin a."""
        out = []
        for i in range(int(n)):
            a = 2.0 * math.pi * i / int(n)
            out.append({"centre": (rx * math.cos(a), ry * math.sin(a), 0.0), "yaw": yaw * math.cos(a), "pitch": pitch * math.sin(a)})
        return out

    @staticmethod
    def dolly(n, z0, z1):
        """Along the optical axis from z0 to z1 baselines, both ends included (n = 1: z0); positive is forward."""
        return [{"centre": (0.0, 0.0, _lerp(z0, z1, i, n))} for i in range(int(n))]

    @staticmethod
    def pan(n, yaw0, yaw1):
        """On the spot from yaw0 to yaw1 degrees, both ends included (n = 1: yaw0)."""
        return [{"yaw": _lerp(yaw0, yaw1, i, n)} for i in range(int(n))]


def _lerp(a, b, i, n):
    return float(a) if int(n) < 2 else float(a) + (float(b) - float(a)) * i / (int(n) - 1)


def check_poses(poses):
    """The poses as an (V, 12) float64 array; ValueError on what the library would refuse (none, a wrong size, a non-finite entry, a third
    row of A that is all zero).  A pose is the 12 values of pose(), or a pair (A (3, 3), E (3,))."""
    recs = []
    for p in poses:
        if isinstance(p, (tuple, list)) and len(p) == 2:
            p = np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(-1), np.asarray(p[1], dtype=np.float64).reshape(-1)])
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size != 12:
            raise ValueError("freeview: a pose is 12 values (A then E), got {}".format(p.size))
        recs.append(p)
    if not recs:
        raise ValueError("freeview: no pose given")
    recs = np.ascontiguousarray(np.stack(recs))
    if not np.isfinite(recs).all():
        raise ValueError("freeview: pose(s) {} hold a non-finite entry".format(np.nonzero(~np.isfinite(recs).all(1))[0].tolist()))
    flat = np.nonzero((recs[:, 6:9] == 0.0).all(1))[0]
    if flat.size:
        raise ValueError("freeview: pose(s) {}: the third row of A is all zero".format(flat.tolist()))
    return recs


def check_want(want):
    want = tuple(want)
    if not want or any(w not in OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError("freeview: want must be a non-empty subset of {} (each once), got {!r}".format(OUTPUTS, want))
    return want


def warp(dlog0, left, min_disp, max_disp, poses, want=OUTPUTS):
    """dlog0 (B, N, H, W) planar f32 logits, left (B, 3, H, W), min_disp / max_disp: B values in pixels, poses: any number of pose() records.
    -> {"view": (B, V, 3, H, W), "disp": (B, V, 1, H, W), "cover": (B, V, 1, H, W)} restricted to `want`.  Every argument is checked
    before the first launch."""
    recs = check_poses(poses)
    want = check_want(want)
    (dlog0, left, mn, mx), (B, N, H, W) = M.check_logits("freeview.warp", dlog0, min_disp, max_disp, left, with_left=True)
    V = len(recs)
    dev = dlog0.device
    chans = {"view": 3, "disp": 1, "cover": 1}
    out = {k: torch.empty(B, V, chans[k], H, W, dtype=torch.float32, device=dev) for k in want}
    lib, st = L.lib(), L.stream_ptr()

    def launch(part, bufs):
        part = np.ascontiguousarray(part)
        L.check(lib.falnet_med_pose_fwd(L.ptr(dlog0), L.ptr(left), L.ptr(mn), L.ptr(mx), part.ctypes.data_as(ctypes.c_void_p), len(part),
                                        L.ptr(bufs.get("view")), L.ptr(bufs.get("disp")), L.ptr(bufs.get("cover")), B, N, H, W, st), "med_pose_fwd")
    M.launch_in_parts(recs, MAX_POSES, out, launch)
    return out


FILL_BETA = 4.0  # fill_views' default bias: chosen from the step-scene table of DESIGN.md section 7i (a 16-wide hole comes out 96 % background), not tuned


def fill_views(out, max_disp, beta=FILL_BETA, floor=2.0 ** -10):
    """The holes of warp()'s result filled (fal_net_amd/inpaint.py): `out` needs "view" (B, V, 3, H, W), "cover" and "disp" (B, V, 1, H, W);
    max_disp: B values in pixels, the guide's scale per sample.  One C = 4 call over all B V images: the colour channels as they are (view is
    premultiplied by cover already), disp cover as the fourth premultiplied channel, weight = cover, guide = disp: what a hole receives comes
    from the side of SMALLER disparity, the background.  beta in [0, 8]; the default 4.0 is a choice read off the step-scene table (DESIGN.md
    section 7i), not a tuned value.  -> {"view": (B, V, 3, H, W), "disp": (B, V, 1, H, W)}, un-premultiplied and fully weighted."""
    from . import inpaint
    beta, floor = inpaint.check_params(beta, floor)
    missing = [k for k in OUTPUTS if k not in out]
    if missing:
        raise ValueError("freeview.fill_views: the result of warp() lacks {}".format(missing))
    view, disp, cover = out["view"], out["disp"], out["cover"]
    if view.dim() != 5 or view.shape[2] != 3 or tuple(disp.shape) != tuple(view.shape[:2]) + (1,) + tuple(view.shape[3:]) or cover.shape != disp.shape:
        raise ValueError("freeview.fill_views: expected view (B, V, 3, H, W) with disp and cover (B, V, 1, H, W), got {}, {} and {}".format(
            tuple(view.shape), tuple(disp.shape), tuple(cover.shape)))
    B, V = view.shape[:2]
    if not torch.is_tensor(max_disp) or max_disp.numel() != B:
        raise ValueError("freeview.fill_views: max_disp must hold one value per sample (B={})".format(B))
    scale = M.f32(max_disp, "max_disp", "freeview").reshape(B, 1).expand(B, V).contiguous()
    filled = inpaint.fill(torch.cat([view, disp * cover], 2), cover, guide=disp, guide_scale=scale, beta=beta, floor=floor)
    return {"view": filled[:, :, :3].contiguous(), "disp": filled[:, :, 3:].contiguous()}


def render(model, left, min_disp, max_disp, poses, want=OUTPUTS, fill=None):
    """One no_grad disparity-only forward of `model` (FAL_netA / B / C, any compute dtype: the logits are planar f32 in all of them), then
    warp over the plan's own logits with the plan's prologue-processed min_disp / max_disp, as views.render reaches them.
    -> (the dict of warp(), the forward's disparity (B, 1, H, W)).  fill=beta adds "view_filled" and "disp_filled" (fill_views with that
    beta; all three outputs are rendered for it and those not in `want` dropped again); fill=None does exactly what it did before."""
    recs = check_poses(poses)
    want = check_want(want)
    if fill is not None:
        from . import inpaint
        inpaint.check_params(fill, 2.0 ** -10)
    with torch.no_grad():
        buf, disp = M.forward_logits(model, left, min_disp, max_disp)
        out = warp(buf["dlog0"], buf["left"], buf["min_disp"], buf["max_disp"], recs, want if fill is None else OUTPUTS)
        if fill is not None:
            filled = fill_views(out, buf["max_disp"], beta=fill)
            out = {k: out[k] for k in want}
            out["view_filled"], out["disp_filled"] = filled["view"], filled["disp"]
    return out, disp


class FreeviewWriter:
    """Writes free-viewpoint frames under `save_path`: Freeview/{frame:010d}_p{pose:02d}.png through dumps.image_u8 and
    Freeview/{frame:010d}_p{pose:02d}_cover.png through dumps.feature_u8.  The folder is its own: dumps.DUMP_KINDS and dumps.FrameWriter do
    not know about it.  The mean cover over everything written is kept on the device and read once, by summary().  poses: the target cameras
    frame() renders, as pose keyword sets (what `paths` returns); fill_beta: also their hole-filled views (fill_views with that bias) as
    ..._filled.png; extra: what summary() says besides the counts."""
    folder = "Freeview"
    key = "freeview"

    def __init__(self, save_path, poses=(), fill_beta=None, extra=None):
        self.save_path, self.poses, self.fill_beta, self.extra = save_path, list(poses), fill_beta, dict(extra or {})
        self.path = os.path.join(save_path, self.folder)
        os.makedirs(self.path, exist_ok=True)
        self.files = 0
        self.frames = 0
        self.filled = 0
        self._cover_sum = None
        self._cover_n = 0

    def file(self, i, p, cover=False):
        return os.path.join(self.path, "{:010d}_p{:02d}{}.png".format(i, p, "_cover" if cover else ""))

    def frame(self, f):
        """An inference.Frame's views and cover maps from self.poses around the nominal camera of the frame's size, from the logits of one more
        disparity-only forward (render)."""
        K = camera(f.left.shape[-2], f.left.shape[-1])
        out, _ = render(f.model, f.left, f.min_disp, f.max_disp, [pose(K, **kw) for kw in self.poses], want=("view", "cover"), fill=self.fill_beta)
        self.write(f.index, out["view"], out["cover"])
        if self.fill_beta is not None:
            self.write_filled(f.index, out["view_filled"])

    def write(self, i, views, cover):
        """views (1, V, 3, H, W), cover (1, V, 1, H, W) of frame `i`."""
        from PIL import Image
        from . import dumps
        rgb = dumps.image_u8(views[0]).cpu().numpy()          # (V, H, W, 3)
        grey = dumps.feature_u8(cover[0]).cpu().numpy()       # (V, 1, H, W)
        for p in range(rgb.shape[0]):
            Image.fromarray(rgb[p]).save(self.file(i, p))
            Image.fromarray(grey[p, 0]).save(self.file(i, p, cover=True))
            self.files += 2
        s = cover.sum(dtype=torch.float64)
        self._cover_sum = s if self._cover_sum is None else self._cover_sum + s
        self._cover_n += cover.numel()
        self.frames += 1

    def write_filled(self, i, filled):
        """filled (1, V, 3, H, W), the hole-filled views of frame `i` (fill_views): Freeview/{frame:010d}_p{pose:02d}_filled.png."""
        from PIL import Image
        from . import dumps
        rgb = dumps.image_u8(filled[0]).cpu().numpy()         # (V, H, W, 3)
        for p in range(rgb.shape[0]):
            Image.fromarray(rgb[p]).save(os.path.join(self.path, "{:010d}_p{:02d}_filled.png".format(i, p)))
            self.files += 1
        self.filled += rgb.shape[0]

    def summary(self):
        out = {"frames": self.frames, "files": self.files,
               "mean_cover": float(self._cover_sum) / self._cover_n if self._cover_n else None}
        if self.filled:
            out["filled"] = self.filled
        return dict(out, **self.extra)
