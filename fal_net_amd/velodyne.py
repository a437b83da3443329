"""Velodyne ground truth of the original Eigen test split (reference: Datasets/Kitti_eigen_test_original.py, which reads a ready-made
`<frame>.npy` depth map beside each image and leaves making it to Monodepth's `generate_depth_map`): the raw-KITTI file handling on the host --
calibration files, the projection matrix, the scan, the paths of a list line -- and the projection itself on the device (csrc/velo.hip:
falnet_velo_project).

The projection's result is defined operation by operation (include/falnet_hip.h); the host restatement it is tested against is
tests/_velo_ref.py.  Nothing here needs a GPU to import; `project` does: like the rest of the package it has no CPU fallback and raises on a CPU
tensor.  The host side of the way back (fal_net_amd/pseudo_lidar.py: unproject) is here too: backprojection_matrix, nominal_matrix, focal_baseline."""
import ctypes as C
import os

import numpy as np
import torch


def read_calib_file(path):
    """KITTI's calibration text ('key: v v v ...' per line) -> {key: float64 array}.  Lines whose values do not parse as numbers (calib_time: a
    date) are skipped, as Monodepth's reader skips them."""
    out = {}
    with open(path) as f:
        for line in f:
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            try:
                out[key.strip()] = np.array([float(v) for v in value.split()], dtype=np.float64)
            except ValueError:
                pass
    return out


def projection_matrix(calib_dir, cam=2):
    """The 3 x 4 float64 matrix that takes a homogeneous Velodyne point to the image plane of camera `cam` (2: left colour, 3: right colour):
    P_rect_0<cam> . [R_rect_00 | 0; 0 1] . [R T; 0 0 0 1] from calib_cam_to_cam.txt and calib_velo_to_cam.txt, as two float64 np.dot's in
    Monodepth's order."""
    if int(cam) not in (2, 3):
        raise ValueError("cam must be 2 or 3, got {!r}".format(cam))
    cam2cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo2cam = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    for name, d, keys in (("calib_cam_to_cam.txt", cam2cam, ("R_rect_00", "P_rect_0%d" % int(cam))), ("calib_velo_to_cam.txt", velo2cam, ("R", "T"))):
        for k in keys:
            if k not in d:
                raise KeyError("{} has no numeric entry {!r}".format(os.path.join(calib_dir, name), k))
    v2c = np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"].reshape(3, 1)))
    v2c = np.vstack((v2c, np.array([0.0, 0.0, 0.0, 1.0])))
    r_rect = np.eye(4)
    r_rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    p_rect = cam2cam["P_rect_0%d" % int(cam)].reshape(3, 4)
    return np.dot(np.dot(p_rect, r_rect), v2c)


def backprojection_matrix(P):
    """The 3 x 4 float64 Q = [M^-1 | M^-1 . P[:, 3]] of a 3 x 4 projection matrix P with M = P[:, :3]: a pixel (v, u) of depth d -- the
    projection's third homogeneous coordinate -- is the Velodyne point X = d (Q[:, :3] . (u + 1, v + 1, 1)) - Q[:, 3] (falnet_velo_unproject)."""
    Pm = np.asarray(P, dtype=np.float64)
    if Pm.shape != (3, 4):
        raise ValueError("P: expected a 3 x 4 matrix, got shape {}".format(Pm.shape))
    m_inv = np.linalg.inv(Pm[:, :3])
    return np.hstack((m_inv, np.dot(m_inv, Pm[:, 3:4])))


def nominal_matrix(H, W, focal):
    """A projection matrix for a frame without calibration: K . axes with focal length `focal`, the principal point at the image centre
    (W / 2, H / 2), the Velodyne axes turned into the camera's (x forward -> z, y left -> -x, z up -> -y) and no translation."""
    if not (H > 0 and W > 0 and focal > 0):
        raise ValueError("nominal_matrix: H, W and focal must be positive, got {} {} {}".format(H, W, focal))
    K = np.array([[float(focal), 0.0, W / 2.0], [0.0, float(focal), H / 2.0], [0.0, 0.0, 1.0]])
    axes = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    return np.hstack((np.dot(K, axes), np.zeros((3, 1))))


def decompose(P):
    """(K, R, t) of a 3 x 4 projection matrix P = K [R | t]: K upper triangular with a positive diagonal, R a rotation (det R = +1), by numpy's QR
    of the reversed rows (an RQ decomposition) of M = P[:, :3], and t = K^-1 P[:, 3].  A matrix whose M has a negative determinant is the same
    projection with the opposite sign: it is decomposed as -P.  nominal_matrix gives its own K and axes and t = 0."""
    Pm = np.asarray(P, dtype=np.float64)
    if Pm.shape != (3, 4):
        raise ValueError("P: expected a 3 x 4 matrix, got shape {}".format(Pm.shape))
    det = np.linalg.det(Pm[:, :3])
    if not np.isfinite(det) or det == 0.0:
        raise ValueError("decompose: the left 3 x 3 block of P is singular")
    if det < 0.0:
        Pm = -Pm
    M = Pm[:, :3]
    flip = np.eye(3)[::-1]
    q, r = np.linalg.qr(np.dot(flip, M).T)  # flip M = r^T q^T  =>  M = (flip r^T flip) (flip q^T)
    K, R = np.dot(flip, np.dot(r.T, flip)), np.dot(flip, q.T)
    sign = np.diag(np.where(np.diag(K) < 0.0, -1.0, 1.0))  # K sign . sign R: the diagonal positive, the product unchanged
    K, R = np.dot(K, sign), np.dot(sign, R)
    return K, R, np.linalg.solve(K, Pm[:, 3])


def focal_baseline(calib_dir, cam=2):
    """focal length times stereo baseline of the colour pair in calib_cam_to_cam.txt, f . |P_rect_02[0, 3] - P_rect_03[0, 3]| / f with f the focal
    length of camera `cam`: depth = focal_baseline / disparity for a disparity in pixels of that camera's image."""
    if int(cam) not in (2, 3):
        raise ValueError("cam must be 2 or 3, got {!r}".format(cam))
    path = os.path.join(calib_dir, "calib_cam_to_cam.txt")
    cam2cam = read_calib_file(path)
    for k in ("P_rect_02", "P_rect_03"):
        if k not in cam2cam:
            raise KeyError("{} has no numeric entry {!r}".format(path, k))
    p2, p3 = cam2cam["P_rect_02"].reshape(3, 4), cam2cam["P_rect_03"].reshape(3, 4)
    f = (p2 if int(cam) == 2 else p3)[0, 0]
    return float(f * abs(p2[0, 3] - p3[0, 3]) / f)


def load_scan(path):
    """A raw scan (velodyne_points/data/<frame>.bin) as an (N, 4) float32 array: x forward, y left, z up, reflectance."""
    size = os.path.getsize(path)
    if size % 16:
        raise ValueError("{}: {} bytes is not a whole number of 16-byte points (x, y, z, reflectance as float32): the file is truncated "
                         "or is not a Velodyne scan".format(path, size))
    return np.fromfile(path, np.float32).reshape(-1, 4)


def raw_paths(left_rel, raw_root):
    """A left-image entry of the reference's list, '<date>_drive_<n>_sync_02/<frame>.jpg' -> (the scan
    <raw_root>/<date>/<date>_drive_<n>_sync/velodyne_points/data/<frame>.bin, the calibration directory <raw_root>/<date>) of the raw KITTI tree."""
    folder, name = os.path.split(left_rel.replace("\\", "/"))
    folder = os.path.basename(folder)
    frame = os.path.splitext(name)[0]
    if not folder.endswith(("_sync_02", "_sync_03")) or len(folder) < 19 or not frame:
        raise ValueError("{!r} is not '<date>_drive_<n>_sync_0<cam>/<frame>.<ext>'".format(left_rel))
    drive, date = folder[:-3], folder[:10]
    return os.path.join(raw_root, date, drive, "velodyne_points", "data", frame + ".bin"), os.path.join(raw_root, date)


def project(points, P, H, W, vel_depth=False, out=None):
    """The scan `points` (CUDA f32 (N, 4): x, y, z, reflectance) through the 3 x 4 float64 matrix `P` into an (H, W) f32 depth map on the same
    device: per pixel the depth of the closest point that lands on it, 0 where none does (falnet_velo_project).  vel_depth: a point's depth is its
    x instead of its camera z.  out: an (H, W) f32 CUDA tensor to write into (every pixel is written).  Bit-identical for any order of the points."""
    from . import _lib as L
    if not torch.is_tensor(points) or not points.is_cuda:
        raise RuntimeError("fal_net_amd.velodyne.project runs on an MI355X only (no CPU fallback); points is {}".format(
            "on " + str(points.device) if torch.is_tensor(points) else type(points).__name__))
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4:
        raise ValueError("points: expected an (N, 4) float32 tensor, got {} {}".format(tuple(points.shape), points.dtype))
    Pm = np.ascontiguousarray(np.asarray(P, dtype=np.float64))
    if Pm.shape != (3, 4):
        raise ValueError("P: expected a 3 x 4 matrix, got shape {}".format(Pm.shape))
    H, W = int(H), int(W)
    points = points.detach().contiguous()
    if out is None:
        out = torch.empty((max(H, 0), max(W, 0)), dtype=torch.float32, device=points.device)
    elif (not torch.is_tensor(out) or out.device != points.device or out.dtype != torch.float32 or tuple(out.shape) != (H, W)
          or not out.is_contiguous()):
        raise ValueError("out: expected a contiguous ({}, {}) float32 tensor on {}".format(H, W, points.device))
    p12 = (C.c_double * 12)(*Pm.reshape(-1).tolist())
    with torch.cuda.device(points.device):
        L.check(L.lib().falnet_velo_project(L.ptr(points), int(points.shape[0]), p12, H, W, int(bool(vel_depth)), L.ptr(out), L.stream_ptr()),
                "velo_project")
    return out
