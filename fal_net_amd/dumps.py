"""Test-time outputs of the reference's test script computed on the device (reference Test_KITTI.py:211-253,303-317, myUtils.py:339-394):
plasma-coloured disparity PNGs, the input image and the synthesised view as 8-bit images, occlusion / feature maps as grey PNGs, the
local normalisation and a coloured point cloud (PLY).  The kernels are csrc/dump.hip; what reaches the host is a finished byte buffer.

There is no host fallback: every function here takes CUDA tensors and raises on anything else.  `FrameWriter` is the only part that touches
the disk (Pillow for PNG, plain file writes for PLY)."""
import os

import numpy as np
import torch

from . import _lib as L

MEAN = (0.411, 0.432, 0.45)  # Train_Stage1_K.py:127 -- what the loader subtracted
_LUT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plasma_lut.txt")
_lut_dev = {}

PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])  # 15 bytes, no padding
DUMP_KINDS = ("disp", "input", "pan", "pc", "feats")


def plasma_lut():
    """matplotlib's 'plasma' colour map as 256 RGBA byte rows (tools/make_plasma_lut.py wrote the file; matplotlib is not needed here)."""
    lut = np.ascontiguousarray(np.loadtxt(_LUT_PATH, dtype=np.uint8))
    assert lut.shape == (256, 4) and lut.dtype == np.uint8
    return lut


def _lut_on(device):
    key = str(device)
    if key not in _lut_dev:
        _lut_dev[key] = torch.from_numpy(plasma_lut()).to(device).contiguous()
    return _lut_dev[key]


def _planar(x, dims=4):
    if not x.is_cuda:
        raise RuntimeError("fal_net_amd.dumps runs on an MI355X only (no CPU fallback); input is on " + str(x.device))
    assert x.dim() == dims, f"expected a {dims}-d tensor, got {tuple(x.shape)}"
    return x.detach().to(torch.float32).contiguous()


def _bytes(n, device):
    """n output bytes in an allocation rounded up to whole 32-bit words (the kernels store words)."""
    return torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=device)


def percentile(x, q, return_order_stats=False):
    """np.percentile(x[b], q) for every sample b of x (B, ...) -> (B,) f32 on the device, exact (radix select; numpy's default linear
    interpolation between the two neighbouring order statistics).  return_order_stats: also the (B, 2) order statistics themselves."""
    x = _planar(x, x.dim())
    B = x.shape[0]
    n = x[0].numel()
    lib = L.lib()
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    words = int(lib.falnet_percentile_workspace_bytes(B)) // 4
    ws = torch.empty(words, dtype=torch.int32, device=x.device)
    L.check(lib.falnet_percentile_f32(L.ptr(x), n, B, float(q), L.ptr(out), L.ptr(ws), L.stream_ptr()), "percentile_f32")
    if return_order_stats:
        return out, ws.view(B, words // B)[:, 4:6].contiguous().view(torch.float32)
    return out


def disparity_png(disp, p95=None):
    """Test_KITTI.py:213-216 (np.percentile, clip, rint, plt.imsave(cmap='plasma', vmin=0, vmax=256)): disp (B, 1, H, W) -> (B, H, W, 4) u8 RGBA
    on the device.  p95: (B,) device tensor; default = percentile(disp, 95)."""
    disp = _planar(disp)
    B, C, H, W = disp.shape
    assert C == 1
    p95 = percentile(disp, 95.0) if p95 is None else p95.detach().to(torch.float32).contiguous().view(-1)
    assert p95.numel() == B and p95.is_cuda
    out = torch.empty(B, H, W, 4, dtype=torch.uint8, device=disp.device)
    L.check(L.lib().falnet_disp_to_plasma_u8(L.ptr(disp), L.ptr(p95), L.ptr(_lut_on(disp.device)), L.ptr(out), B, H, W, L.stream_ptr()), "disp_to_plasma_u8")
    return out


def image_u8(x, mean=MEAN):
    """Test_KITTI.py:229-241: normalised planar image (B, 3, H, W) -> (B, H, W, 3) u8, rint(255 (x + mean)) saturated to [0, 255] (the reference's
    astype(uint8) wraps out-of-range values; this saturates -- the one deliberate difference)."""
    x = _planar(x)
    B, C, H, W = x.shape
    assert C == 3
    n = B * H * W * 3
    buf = _bytes(n, x.device)
    L.check(L.lib().falnet_image_to_u8(L.ptr(x), float(mean[0]), float(mean[1]), float(mean[2]), L.ptr(buf), B, H, W, L.stream_ptr()), "image_to_u8")
    return buf[:n].view(B, H, W, 3)


def feature_u8(x):
    """Test_KITTI.py:248-253: rint(clip(255 |x|, 0, 255)) as u8, same shape as x."""
    x = _planar(x, x.dim())
    n = x.numel()
    buf = _bytes(n, x.device)
    L.check(L.lib().falnet_feature_to_u8(L.ptr(x), L.ptr(buf), n, L.stream_ptr()), "feature_to_u8")
    return buf[:n].view(x.shape)


def local_normalization(img, win=3, mean=MEAN, return_stats=False):
    """local_normalization of Test_KITTI.py:303-317 on the device (the reference moves the image to the CPU for it).  return_stats: also the
    window mean and standard deviation the quotient is made of."""
    x = _planar(img)
    B, C, H, W = x.shape
    assert C == 3
    out = torch.empty_like(x)
    mu = torch.empty_like(x) if return_stats else None
    sigma = torch.empty_like(x) if return_stats else None
    L.check(L.lib().falnet_local_norm(L.ptr(x), float(mean[0]), float(mean[1]), float(mean[2]), L.ptr(out), L.ptr(mu), L.ptr(sigma), int(win), B, H, W,
                                      L.stream_ptr()), "local_norm")
    return (out, mu, sigma) if return_stats else out


def point_cloud(img, disp, focal=None, baseline=None, packed=False, mean=MEAN, rgb_scale=255.0):
    """get_point_cloud of myUtils.py:339-373 from the normalised image (B, 3, H, W) and the disparity (B, 1, H, W): colour = (img + mean) *
    rgb_scale.  focal / baseline: the camera (pixels, metres); default = the KITTI tables by image width (KeyError on another width, as in the
    reference).  packed=False -> (B, 6, H W) f32, rows x, z, -y, r, g, b (the reference's layout); packed=True -> (B, H W, 15) u8, the
    binary-PLY vertex records (PLY_VERTEX)."""
    from .myUtils import width_to_baseline, width_to_focal
    disp = _planar(disp)
    img = _planar(img)
    B, C, H, W = disp.shape
    assert C == 1 and img.shape == (B, 3, H, W)
    focal = width_to_focal[W] if focal is None else focal
    baseline = width_to_baseline[W] if baseline is None else baseline
    n = H * W
    if packed:
        buf = _bytes(B * n * 15, img.device)
        planar = None
    else:
        buf = None
        planar = torch.empty(B, 6, n, dtype=torch.float32, device=img.device)
    L.check(L.lib().falnet_point_cloud(L.ptr(img), float(mean[0]), float(mean[1]), float(mean[2]), float(rgb_scale), L.ptr(disp), float(focal),
                                       float(baseline), L.ptr(planar), L.ptr(buf), B, H, W, L.stream_ptr()), "point_cloud")
    return buf[:B * n * 15].view(B, n, 15) if packed else planar


# ---- PLY files ---------------------------------------------------------------------------------------------------------------------------
def check_ply_format(ply_format):
    if ply_format not in ("binary", "ascii"):
        raise ValueError("ply_format must be 'binary' or 'ascii', got {!r}".format(ply_format))


def _ply_header(fmt, n, normals=False, faces=None):
    """The header of a point cloud; normals: nx ny nz after the coordinates; faces: a count -- the face element of a mesh (mesh.save_ply)."""
    return ("ply\nformat {} 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n{}"
            "property uchar diffuse_red\nproperty uchar diffuse_green\nproperty uchar diffuse_blue\n{}end_header\n").format(
                fmt, n, "property float nx\nproperty float ny\nproperty float nz\n" if normals else "",
                "" if faces is None else "element face {}\nproperty list uchar int vertex_indices\n".format(faces))


def pack_vertices(pc):
    """(6, n) array of rows x, y, z, r, g, b -> n PLY_VERTEX records: what the device's packed output holds (colours truncated like int(),
    saturated to a byte)."""
    pc = np.asarray(pc)
    rec = np.empty(pc.shape[1], dtype=PLY_VERTEX)
    for k, name in enumerate(PLY_VERTEX.names):
        rec[name] = pc[k] if k < 3 else np.clip(np.trunc(pc[k]), 0, 255)
    return rec


def save_ply(file_name, planar=None, packed=None, ply_format="binary"):
    """One point cloud to `file_name`.  'ascii': the reference's file (myUtils.py:378-394: '{:f} {:f} {:f} {:d} {:d} {:d}' lines, colours through
    int()) from the planar (6, n) array, formatted a block of vertices at a time; 'binary': binary_little_endian with the same six properties,
    the packed records written as one buffer."""
    check_ply_format(ply_format)
    if ply_format == "ascii":
        pc = np.asarray(planar)
        n = pc.shape[1]
        with open(file_name, "w+") as f:
            f.write(_ply_header("ascii", n))
            block = 1 << 16
            for s in range(0, n, block):
                rows = np.empty((min(block, n - s), 6), dtype=object)
                rows[:, :3] = pc[:3, s:s + block].T.astype(np.float64)
                rows[:, 3:] = pc[3:, s:s + block].T.astype(np.int64)  # int(): truncation toward zero
                f.write(("%f %f %f %d %d %d\n" * len(rows)) % tuple(rows.ravel()))
        return
    rec = pack_vertices(planar) if packed is None else np.ascontiguousarray(packed).view(np.uint8).reshape(-1, 15)
    with open(file_name, "wb") as f:
        f.write(_ply_header("binary_little_endian", len(rec)).encode("ascii"))
        f.write(rec.tobytes())


def camera_for_width(w):
    """(focal, baseline) for a frame `w` pixels wide: the KITTI calibration tables, or -- a frame that is not a KITTI width has no calibration --
    the 1242-pixel camera scaled to the width, so that a synthetic frame still gives a cloud of the same shape."""
    from .myUtils import width_to_baseline, width_to_focal
    if w in width_to_focal:
        return width_to_focal[w], width_to_baseline[w]
    return width_to_focal[1242] * w / 1242.0, width_to_baseline[1242]


class FrameWriter:
    """Writes the per-frame outputs of the reference's test script under `save_path`, in its folders (Test_KITTI.py:140-158) and under its
    file names: l_disp/{:010d}.png, 'Input im'/{:010d}.png, Pan/{:010d}.png, Point_cloud/{:010d}.ply, feats/{:010d}_l{layer}_c{channel}.png.
    `what`: any subset of DUMP_KINDS.  Every image is finished on the device; the host copies bytes and encodes files."""
    folders = {"disp": "l_disp", "input": "Input im", "pan": "Pan", "pc": "Point_cloud", "feats": "feats"}
    key = "dump"

    def __init__(self, save_path, what, ply_format="binary"):
        what = tuple(what)
        bad = [k for k in what if k not in DUMP_KINDS]
        if bad:
            raise ValueError("unknown dump kind(s) {}: choose from {}".format(", ".join(bad), ", ".join(DUMP_KINDS)))
        check_ply_format(ply_format)
        self.save_path, self.what, self.ply_format = save_path, what, ply_format
        self.paths = {k: os.path.join(save_path, d) for k, d in self.folders.items()}
        for p in self.paths.values():  # the reference creates all five, whatever is saved
            os.makedirs(p, exist_ok=True)

    @property
    def needs_views(self):
        """True when the frame loop has to run the model with ret_pan / ret_subocc as well (synthesised view, occlusion masks)."""
        return "pan" in self.what or "feats" in self.what

    def file(self, kind, i, layer=None, channel=None):
        if kind == "feats":
            return os.path.join(self.paths[kind], "{:010d}_l{}_c{}.png".format(i, layer, channel))
        return os.path.join(self.paths[kind], "{:010d}.{}".format(i, "ply" if kind == "pc" else "png"))

    def frame(self, f):
        """An inference.Frame to disk (Test_KITTI.py:189-194,211-253).  The synthesised view and the occlusion masks come from one more forward with
        ret_pan / ret_subocc, only where they are wanted; the feature maps are the reference's [local_normalization(input), maskL, maskRL] (its
        `dispr / 100` is not an output of this model's forward)."""
        pan = feats = None
        if self.needs_views:
            pan, _, mask_l, mask_rl = f.model(f.left, f.min_disp, f.max_disp, ret_disp=True, ret_subocc=True, ret_pan=True)
            feats = [local_normalization(f.left), mask_l, mask_rl]
        self.write(f.index, f.left, f.disp, pan=pan, feats=feats)

    def write(self, i, left, disp, pan=None, feats=None):
        """Frame `i` (batch size 1, as the reference's loop): left (1, 3, H, W) normalised input, disp (1, 1, H, W), pan: the synthesised view,
        feats: list of (1, C, H, W) maps, one grey PNG per channel."""
        from PIL import Image
        if "disp" in self.what:
            Image.fromarray(disparity_png(disp)[0].cpu().numpy()).save(self.file("disp", i))  # (H, W, 4) u8 -> RGBA, as plt.imsave writes
        if "input" in self.what:
            Image.fromarray(image_u8(left)[0].cpu().numpy()).save(self.file("input", i))
        if "pan" in self.what and pan is not None:
            Image.fromarray(image_u8(pan)[0].cpu().numpy()).save(self.file("pan", i))
        if "pc" in self.what:
            focal, baseline = camera_for_width(disp.shape[-1])
            if self.ply_format == "binary":
                save_ply(self.file("pc", i), packed=point_cloud(left, disp, focal, baseline, packed=True)[0].cpu().numpy(), ply_format="binary")
            else:
                save_ply(self.file("pc", i), planar=point_cloud(left, disp, focal, baseline)[0].cpu().numpy(), ply_format="ascii")
        if "feats" in self.what and feats is not None:
            for layer, f in enumerate(feats):
                grey = feature_u8(f)[0].cpu().numpy()
                for c in range(grey.shape[0]):
                    Image.fromarray(grey[c]).save(self.file("feats", i, layer, c))


class SweepWriter:
    """Writes the views of a baseline sweep (fal_net_amd/views.py) under `save_path`: Sweep/{frame:010d}_v{view:02d}.png through image_u8, and
    the disparity in the right view's own frame (the t = 1 view) as r_disp/{frame:010d}.png through disparity_png.  Its two folders are its
    own: FrameWriter, DUMP_KINDS and the reference's five folders do not know about them.  fractions: the baseline fractions frame() renders;
    extra: what summary() says besides the file count."""
    folders = {"sweep": "Sweep", "r_disp": "r_disp"}
    key = "sweep"

    def __init__(self, save_path, fractions=(), extra=None):
        self.save_path, self.fractions, self.extra = save_path, list(fractions), dict(extra or {})
        self.paths = {k: os.path.join(save_path, d) for k, d in self.folders.items()}
        for p in self.paths.values():
            os.makedirs(p, exist_ok=True)
        self.files = 0

    def file(self, kind, i, view=None):
        if kind == "sweep":
            return os.path.join(self.paths[kind], "{:010d}_v{:02d}.png".format(i, view))
        return os.path.join(self.paths[kind], "{:010d}.png".format(i))

    def frame(self, f):
        """An inference.Frame's views at self.fractions and the disparity in the right view's own frame (t = 1), all from the logits of one more
        disparity-only forward (views.render)."""
        from . import views as V
        ts = list(self.fractions)
        if 1.0 not in ts:
            ts.append(1.0)  # rendered for its disparity only
        imgs, disps, _ = V.render(f.model, f.left, f.min_disp, f.max_disp, ts)
        self.write(f.index, imgs[:, :len(self.fractions)], right_disp=disps[:, ts.index(1.0)])

    def summary(self):
        return dict(self.extra, files=self.files)

    def write(self, i, views, right_disp=None):
        """Frame `i` (batch size 1): views (1, V, 3, H, W) normalised images, right_disp (1, 1, H, W) the t = 1 disparity or None."""
        from PIL import Image
        assert views.dim() == 5 and views.shape[0] == 1 and views.shape[2] == 3, tuple(views.shape)
        rgb = image_u8(views[0]).cpu().numpy()  # the V views as one batch: (V, H, W, 3) u8
        for j in range(rgb.shape[0]):
            Image.fromarray(rgb[j]).save(self.file("sweep", i, j))
            self.files += 1
        if right_disp is not None:
            Image.fromarray(disparity_png(right_disp)[0].cpu().numpy()).save(self.file("r_disp", i))
            self.files += 1
