"""Triangle meshes from predicted depth: the pixel grid triangulated and cut where depth jumps, on the device (csrc/mesh.hip: falnet_mesh_build).
A mesh vertex IS the point cloud's vertex of its pixel (dumps.point_cloud, packed records); a triangle is kept when its three vertices are valid
(min_depth < z <= max_depth, score >= threshold) and every edge has max(z) <= min(z) (1 + max_jump) -- a ratio of depths, hence of disparities: the
same number of MED planes near and far.  Vertices no kept triangle names are dropped and the rest re-indexed, both record streams in pixel order.

  build(img, disp, ...)              per sample (vertex records (nv, 15 | 27) u8, face records (nf, 13) u8) on the device, and the counts
  save_ply(file, vertices, faces)    a binary or ASCII PLY file with `element face`
  MeshWriter                         Mesh/<frame>.ply of Test_KITTI.py --mesh

The result is defined operation by operation (include/falnet_hip.h); the numpy restatement it is tested against is
tests/_mesh_ref.py.  Nothing here needs a GPU to import; `build` does: like the rest of the package it has no CPU fallback and raises on a CPU
tensor."""
import os

import numpy as np
import torch

from .confidence import check_min_conf
from .dumps import MEAN, PLY_VERTEX, _ply_header, check_ply_format

PLY_VERTEX_NORMALS = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                               ("red", "u1"), ("green", "u1"), ("blue", "u1")])  # 27 bytes, no padding
PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])  # 13 bytes: uchar 3, three indices
MAX_Z = 200.0  # the point cloud caps z here: max_depth stays below it


def check_depths(min_depth, max_depth, max_jump):
    """ValueError unless 0 <= min_depth < max_depth < 200 and max_jump >= 0 (infinity allowed, NaN not): what falnet_mesh_build takes."""
    if not 0.0 <= min_depth < max_depth < MAX_Z:
        raise ValueError("mesh: need 0 <= min_depth < max_depth < {:g}, got {} and {}".format(MAX_Z, min_depth, max_depth))
    if not max_jump >= 0.0:
        raise ValueError("mesh: max_jump must be >= 0 (inf keeps every valid triangle), got {}".format(max_jump))


def build(img, disp, focal=None, baseline=None, max_jump=0.05, min_depth=0.0, max_depth=80.0, score=None, threshold=None, normals=False, mean=MEAN,
          rgb_scale=255.0):
    """img (B, 3, H, W) normalised image, disp (B, 1, H, W) disparity, CUDA tensors -> (meshes, counts): meshes[b] = (vertices (nv, 15) u8 -- or
    (nv, 27) with normals=True --, faces (nf, 13) u8) on the device, counts[b] = (nv, nf).  focal / baseline: the camera (pixels, metres); default =
    the KITTI tables by image width (KeyError on another width, as dumps.point_cloud).  score (B, 1, H, W) and threshold go together: only vertices with
    score >= threshold are valid.  One falnet_mesh_build per sample; the 2 B counts come to the host in ONE copy, after every launch."""
    from . import _lib as L
    from .dumps import _planar
    from .myUtils import width_to_baseline, width_to_focal
    for name, t in (("img", img), ("disp", disp)) + ((("score", score),) if score is not None else ()):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("fal_net_amd.mesh.build runs on an MI355X only (no CPU fallback); {} is {}".format(
                name, "on " + str(t.device) if torch.is_tensor(t) else type(t).__name__))
    if (score is None) != (threshold is None):
        raise ValueError("mesh.build: score and threshold go together")
    check_depths(float(min_depth), float(max_depth), float(max_jump))
    disp, img = _planar(disp.detach()), _planar(img.detach())
    B, C, H, W = disp.shape
    if C != 1 or tuple(img.shape) != (B, 3, H, W):
        raise ValueError("mesh.build: image {} does not match the disparity {}".format(tuple(img.shape), tuple(disp.shape)))
    if score is not None:
        if tuple(score.shape) != (B, 1, H, W) or score.device != disp.device:
            raise ValueError("mesh.build: score {} does not match the disparity {}".format(tuple(score.shape), tuple(disp.shape)))
        score = _planar(score.detach())
    focal = width_to_focal[W] if focal is None else focal
    baseline = width_to_baseline[W] if baseline is None else baseline
    lib = L.lib()
    ws_bytes = int(lib.falnet_mesh_workspace_bytes(H, W))
    if ws_bytes <= 0:
        raise ValueError("mesh.build: a {} x {} map is outside what falnet_mesh_build takes (1 <= H W < 2^28)".format(H, W))
    dev = disp.device
    rec, n, nq = 27 if normals else 15, H * W, max(H - 1, 0) * max(W - 1, 0)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(B, 2, dtype=torch.int64, device=dev)
    outs = []
    with torch.cuda.device(dev):
        for b in range(B):
            # worst case: every pixel a vertex, two triangles per quad; rounded up to whole dwords
            v = torch.empty((n * rec + 3) // 4 * 4, dtype=torch.uint8, device=dev)
            f = torch.empty((2 * nq * 13 + 3) // 4 * 4 + 4, dtype=torch.uint8, device=dev)
            L.check(lib.falnet_mesh_build(L.ptr(img[b]), float(mean[0]), float(mean[1]), float(mean[2]), float(rgb_scale), L.ptr(disp[b]), float(focal),
                                          float(baseline), L.ptr(score[b]) if score is not None else None, 0.0 if threshold is None else float(threshold),
                                          float(min_depth), float(max_depth), float(max_jump), H, W, int(bool(normals)), L.ptr(v), L.ptr(f), L.ptr(counts[b]),
                                          L.ptr(ws), L.stream_ptr()), "mesh_build")
            outs.append((v, f))
    kept = [tuple(c) for c in counts.cpu().tolist()]  # the one copy
    return [(v[:nv * rec].view(nv, rec), f[:nf * 13].view(nf, 13)) for (v, f), (nv, nf) in zip(outs, kept)], kept


# ---- PLY files ---------------------------------------------------------------------------------------------------------------------------------------
def _records(x, width, what):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if a.size % width:
        raise ValueError("mesh.save_ply: {} hold {} bytes, no multiple of the {}-byte record".format(what, a.size, width))
    return a.reshape(-1, width)


def save_ply(file_name, vertices, faces, normals=False, ply_format="binary"):
    """One mesh to `file_name` from the records build() returns (tensors on any device, or arrays): 'binary' writes binary_little_endian, the two
    record buffers as they are; 'ascii' formats the same records on the host ('%f' coordinates as dumps.save_ply, '3 i j k' faces)."""
    check_ply_format(ply_format)
    vdt = PLY_VERTEX_NORMALS if normals else PLY_VERTEX
    v, f = _records(vertices, vdt.itemsize, "vertices"), _records(faces, PLY_FACE.itemsize, "faces")
    if ply_format == "binary":
        with open(file_name, "wb") as out:
            out.write(_ply_header("binary_little_endian", len(v), normals, len(f)).encode("ascii"))
            out.write(v.tobytes())
            out.write(f.tobytes())
        return
    vr, fr = np.frombuffer(v.tobytes(), vdt), np.frombuffer(f.tobytes(), PLY_FACE)
    floats = [n for n in vdt.names if vdt[n].kind == "f"]
    line = " ".join(["%f"] * len(floats) + ["%d"] * 3) + "\n"
    with open(file_name, "w") as out:
        out.write(_ply_header("ascii", len(vr), normals, len(fr)))
        block = 1 << 16
        for s in range(0, len(vr), block):
            part = vr[s:s + block]
            rows = np.empty((len(part), len(floats) + 3), dtype=object)
            for k, n in enumerate(floats):
                rows[:, k] = part[n].astype(np.float64)
            for k, n in enumerate(("red", "green", "blue")):
                rows[:, len(floats) + k] = part[n].astype(np.int64)
            out.write((line * len(rows)) % tuple(rows.ravel()))
        for s in range(0, len(fr), block):
            idx = fr["v"][s:s + block].astype(np.int64)
            out.write(("3 %d %d %d\n" * len(idx)) % tuple(idx.ravel()))


class MeshWriter:
    """Test_KITTI.py --mesh: writes Mesh/{frame:010d}.ply under `save_path`, the frame's depth mesh with the camera of dumps.camera_for_width.  Its
    folder is its own, as dumps.SweepWriter's: FrameWriter and DUMP_KINDS do not know about it.  min_conf: with it, write() needs the frame's
    confidence map and only vertices of conf >= min_conf are valid.
    min_component = K: a speckle filter.  The frame's component sizes (components.size_score of the disparity, joined at component_jump -- default:
    max_jump --, the depth bounds as disparity bounds lo = fb / max_depth and hi = fb / min_depth or infinity, and with min_conf the confidence map as
    the components' score, so that a low-confidence pixel has size 0) become build's score with threshold K: only the vertices in components of at
    least K pixels are valid, and build sees only the size map.  An approximation at the bounds: the components judge the bound on the disparity, build
    on its own f32 chain z = fb / (d + 1e-4f), so a pixel within rounding of a bound can count towards a size and still be dropped by build, or the
    reverse."""
    key = "mesh"

    def __init__(self, save_path, max_jump=0.05, max_depth=80.0, min_depth=0.0, min_conf=None, normals=False, ply_format="binary", min_component=None,
                 component_jump=None):
        from .components import check_jump, check_min_component
        check_depths(float(min_depth), float(max_depth), float(max_jump))
        check_min_conf(min_conf)
        check_ply_format(ply_format)
        self.min_component = check_min_component(min_component)
        self.component_jump = check_jump(max_jump if component_jump is None else component_jump, "component_jump")
        self.save_path, self.min_conf, self.normals, self.ply_format = save_path, min_conf, bool(normals), ply_format
        self.kw = dict(max_jump=float(max_jump), max_depth=float(max_depth), min_depth=float(min_depth))
        self.folder = os.path.join(save_path, "Mesh")
        os.makedirs(self.folder, exist_ok=True)
        self.frames = self.vertices = self.faces = self.quads = 0

    def file(self, i):
        return os.path.join(self.folder, "{:010d}.ply".format(i))

    def frame(self, f):
        """An inference.Frame: `f.disp`, the disparity the run evaluates, as a mesh; the confidence map (f.conf(): one more disparity-only forward)
        only when the writer filters by it."""
        self.write(f.index, f.left, f.disp, conf=f.conf() if self.min_conf is not None else None)

    def write(self, i, left, disp, conf=None):
        """Frame `i` (batch size 1): left (1, 3, H, W) normalised input, disp (1, 1, H, W), conf (1, 1, H, W) the confidence map (needed with min_conf)."""
        from . import dumps
        if self.min_conf is not None and conf is None:
            raise ValueError("MeshWriter: min_conf = {} needs the frame's confidence map".format(self.min_conf))
        use = self.min_conf is not None
        focal, baseline = dumps.camera_for_width(disp.shape[-1])
        score, threshold = (conf, self.min_conf) if use else (None, None)
        if self.min_component is not None:
            from . import components
            fb, lo_z = focal * baseline, self.kw["min_depth"]
            score = components.size_score(disp, self.component_jump, lo=fb / self.kw["max_depth"], hi=fb / lo_z if lo_z > 0.0 else float("inf"),
                                          score=score, threshold=threshold).view(disp.shape)
            threshold = float(self.min_component)
        meshes, counts = build(left, disp, focal, baseline, score=score, threshold=threshold, normals=self.normals, **self.kw)
        save_ply(self.file(i), meshes[0][0], meshes[0][1], normals=self.normals, ply_format=self.ply_format)
        self.frames += 1
        self.vertices += counts[0][0]
        self.faces += counts[0][1]
        self.quads += (disp.shape[-2] - 1) * (disp.shape[-1] - 1)
        return counts[0]

    def summary(self):
        """The run's extra JSON line: frames, mean vertices and faces per frame, the kept fraction of the 2 (H - 1) (W - 1) faces."""
        nan = float("nan")
        out = {"frames": self.frames, "vertices": self.vertices, "faces": self.faces,
               "mean_vertices": self.vertices / self.frames if self.frames else nan, "mean_faces": self.faces / self.frames if self.frames else nan,
               "kept_fraction": self.faces / (2 * self.quads) if self.quads else nan, "max_jump": self.kw["max_jump"], "max_depth": self.kw["max_depth"],
               "normals": self.normals}
        if self.min_conf is not None:
            out["min_conf"] = self.min_conf
        if self.min_component is not None:
            out["min_component"] = self.min_component
        return out
