"""Float64 reference of the free-viewpoint plane sweep (csrc/med_pose.hip, fal_net_amd/freeview.py) for element-wise tests.

Written from the definition on the float64 image of the stored float32 inputs (_head_ref.make_inputs); s_n = _head_ref.plane_shifts,
d_n = oracle.falnet_oracle.plane_disparities, the softmax is torch.softmax, the blend is summed in the oracle's order (p = 0; p = p + ...).
A pose is 12 float64 values, A (3 x 3, row-major) then E:

    q = A (x, y, 1)    u0 = q_x / q_z    v0 = q_y / q_z
    w_n = 1 - s_n E_z    u_n = s_n E_x + w_n u0    v_n = s_n E_y + w_n v0          sampled iff q_z > 0 and w_n > 0
    L'_n = bilinear(dlog0_n, u_n, v_n)    four taps (floor v, floor u) .. (floor v + 1, floor u + 1), zero outside the image; 0 when not sampled
    P = softmax_n L'_n
    view = sum_n P_n bilinear(left, u_n, v_n)    disp = sum_n d_n P_n    cover = sum_n P_n omega_n   (omega_n: weights of the taps inside the image)

Magnitudes in the manner of _sweep_ref: the view's is sum_n P_n sum_taps |left tap| over the taps inside the image (the kernel's fractions come
from a float32 plane table and carry an absolute error of about ulp(s)); disp's and cover's are their own values (every term is non-negative).
Comparator, unit roundoffs and eta are _head_ref's:  |got - ref| <= u |ref| + c mag + eta.

Precondition, asserted here: bilinear sampling with zero padding is continuous in the coordinate, the only discontinuities are the two
visibility tests, so every |w_n| >= WMARGIN and every |q_z| >= QMARGIN |K^-1 q| over the case.  The norm is taken of the ray in CAMERA units:
q is "the ray direction in source pixel coordinates", whose pixel-unit norm is the pixel's distance from the image origin -- the identity at
the evaluation width has q = (x, y, 1) and 1 / 1242 < 1e-3 at its right edge, and would fail a test on |q| itself although its q_z is 1
everywhere.  K^-1 leaves q_z as it is, so the test reads: the ray makes a cosine of at least 1e-3 with the optical axis.  A (case, pose set) that
fails the precondition is replaced, never masked.

Coefficients: COEF below was measured on an MI355X against this reference: worst (|got - ref| - u |ref| - eta) / mag over every (case, pose
set) of CASES, its logit families and seeds 0, 1, 2, per output and per _head_ref.disp_class (raw figures: profiles/freeview_vs_f64.txt,
written by tools/measure_freeview.py), then _head_ref.round_up_coef: times 4, rounded up to a power of two.
"""
import functools
import math

import numpy as np
import torch

import _head_ref as R
from oracle import falnet_oracle as O

f64 = torch.float64
WMARGIN = 1e-3
QMARGIN = 1e-3

# (B, N, H, W, maxd); inputs are _head_ref.make_inputs' (mx_b = maxd (1 - 0.07 b), mn = mx 2 / 300)
CASES = [
    (1, 2, 3, 40, 30.0),      # smallest N
    (2, 7, 5, 40, 30.0),      # B > 1 with per-sample max_disp
    (1, 9, 4, 77, 120.0),     # odd width, a one-plane tail chunk
    (1, 7, 19, 70, 30.0),     # more than one tile in both directions, ragged in both
    (2, 49, 9, 128, 300.0),   # the benchmark's N
    (1, 128, 3, 64, 300.0),   # N at the limit, shifts far wider than the image
    (1, 49, 2, 1242, 300.0),  # the evaluation width
]
# (the kernel has ONE path over sizes: a tile grid with ragged edges and a chunk loop with a ragged tail; the views-NULL instantiation is
# taken by the output-subset test.  No case is added.)
SMALL = CASES[:2]
SET_NAMES = ("I", "S", "D", "Y", "G", "O", "F", "N9")


def families(case):
    """All four on the first two cases, a and b elsewhere."""
    return R.ALL_FAMILIES if case in SMALL else ("a", "b")


def listed():
    """[(case, set name, family)] of every comparison."""
    return [(c, s, f) for c in CASES for s in SET_NAMES for f in families(c)]


# ------------------------------------------------------------------------------------------------------------------- poses
def case_camera(case):
    """The source camera the pose sets of a case are built around: KITTI's focal length over width, the principal point at the image centre."""
    _, _, H, W, _ = case
    fx = 721.5377 * W / 1242
    return np.array([[fx, 0.0, (W - 1) / 2], [0.0, fx, (H - 1) / 2], [0.0, 0.0, 1.0]])


def _rot(yaw=0.0, pitch=0.0, roll=0.0):
    y, p, r = (math.radians(a) for a in (yaw, pitch, roll))
    rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
    ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
    rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]])
    return rz @ ry @ rx


def make_pose(K, centre=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, roll=0.0, zoom=1.0):
    """(A, E) as 12 float64 from the explicit construction: A = K R^T K_t^-1, E = K c / fx, c in baselines."""
    Kt = K.copy()
    Kt[0, 0] *= zoom
    Kt[1, 1] *= zoom
    A = K @ _rot(yaw, pitch, roll).T @ np.linalg.inv(Kt)
    E = K @ np.asarray(centre, dtype=np.float64) / K[0, 0]
    return np.concatenate([A.reshape(9), E])


def pose_set(case, name):
    """The poses of set `name` for `case`, each 12 float64 (A then E)."""
    K = case_camera(case)
    _, _, H, W, maxd = case
    eye = np.eye(3).reshape(9)
    if name == "I":
        return [np.concatenate([eye, [0.0, 0.0, 0.0]])]
    if name == "S":  # pure baseline: the sweep's views t
        return [np.concatenate([eye, [t, 0.0, 0.0]]) for t in (1.0, -0.5, 1.9)]
    if name == "D":  # dolly with s_max E_z = 2.5 > 1: the nearest planes lie behind the target camera, the far ones are sampled
        ez = 2.5 / (maxd * (W - 1) / W)
        return [make_pose(K, centre=(0.0, 0.0, ez * K[0, 0]))]
    if name == "Y":
        return [make_pose(K, yaw=3.0)]
    if name == "G":
        return [make_pose(K, centre=(0.4, -0.3, 0.2), roll=10.0, zoom=1.3)]
    if name == "O":  # turned away: q_z < 0 on every pixel
        return [make_pose(K, yaw=180.0)]
    if name in ("F", "N9"):
        eight = [np.concatenate([eye, [0.0, 0.0, 0.0]]), np.concatenate([eye, [1.0, 0.0, 0.0]]), make_pose(K, yaw=3.0), make_pose(K, pitch=2.0),
                 make_pose(K, centre=(0.4, -0.3, 0.2), roll=10.0, zoom=1.3), make_pose(K, centre=(0.0, 0.0, -0.3)),
                 make_pose(K, centre=(-0.3, 0.1, 0.0), zoom=0.8), make_pose(K, centre=(0.2, 0.2, 0.1), roll=-5.0)]
        return eight if name == "F" else eight + [np.concatenate([eye, [-0.5, 0.0, 0.0]])]
    raise ValueError(name)


# COEF[output][class of _head_ref.disp_class]: 4 x the worst observed coefficient, rounded up to a power of two; the observed worst (MI355X,
# seeds 0-2) with the case, pose set, family and seed that produced it beside each.
COEF = {
    "view": {"d30": 2.0 ** -13,    # 2.296e-05  (2, 7, 5, 40, 30) S d seed 2, pose 2 (t = 1.9)
             "wide": 2.0 ** -7},   # 1.001e-03  (1, 49, 2, 1242, 300) S b seed 0, pose 1 (t = -0.5)
    "disp": {"d30": 2.0 ** -12,    # 3.916e-05  (2, 7, 5, 40, 30) S d seed 1, pose 2 (t = 1.9)
             "wide": 2.0 ** -9},   # 3.884e-04  (1, 49, 2, 1242, 300) G b seed 1, pose 0
    "cover": {"d30": 2.0 ** -12,   # 4.209e-05  (2, 7, 5, 40, 30) S d seed 2, pose 2 (t = 1.9)
              "wide": 2.0 ** -6},  # 2.475e-03  (1, 49, 2, 1242, 300) G b seed 1, pose 0
}
# (At the pure-baseline poses alone: view 2.296e-05 / 1.001e-03, disp 3.916e-05 / 3.178e-04 -- none above _sweep_ref.COEF of its class
# (2^-13 / 2^-6, 2^-12 / 2^-9).  The d30 figures are __expf at arguments of about -100 (family d), as the head's; the wide ones are the float32
# plane table: s_n carries a relative error of about 1e-6, 3e-4 pixels at s = 300, times the logit difference of neighbouring taps.  cover's
# magnitude is its own value, which is small where little of the view is seen: the same absolute error in the warped softmax weighs more.)


def coef(output, case):
    c = COEF[output][R.disp_class(case)]
    assert c is not None, f"COEF[{output!r}] has not been measured"
    return c


# ------------------------------------------------------------------------------------------------------------------- precondition
def _rays(pose, H, W):
    A = torch.tensor(np.asarray(pose[:9], dtype=np.float64).reshape(3, 3))
    x = torch.arange(W, dtype=f64).view(1, W).expand(H, W)
    y = torch.arange(H, dtype=f64).view(H, 1).expand(H, W)
    q = [A[i, 0] * x + A[i, 1] * y + A[i, 2] for i in range(3)]
    return q[0], q[1], q[2]


def margins(inp, poses, K):
    """(min |w_n|, min |q_z| / |K^-1 q|) over the samples, planes, pixels and poses of a case."""
    B, N, H, W = inp["dlog0"].shape
    s = R.plane_shifts(inp["mn"], inp["mx"], N, W)
    Kinv = torch.tensor(np.linalg.inv(K))
    wm, qm = float("inf"), float("inf")
    for p in poses:
        wm = min(wm, float((1.0 - s * float(p[11])).abs().min()))
        qx, qy, qz = _rays(p, H, W)
        r = [Kinv[i, 0] * qx + Kinv[i, 1] * qy + Kinv[i, 2] * qz for i in range(3)]
        qm = min(qm, float((qz.abs() / torch.sqrt(r[0] ** 2 + r[1] ** 2 + r[2] ** 2)).min()))
    return wm, qm


def assert_margins(inp, poses, K):
    wm, qm = margins(inp, poses, K)
    assert wm >= WMARGIN, f"some |w_n| = {wm:.3g} < {WMARGIN}: a plane sits on the target camera's own plane -- replace the case or pose"
    assert qm >= QMARGIN, f"some |q_z| = {qm:.3g} |K^-1 q| < {QMARGIN}: a ray grazes the source image plane -- replace the case or pose"
    return wm, qm


# ------------------------------------------------------------------------------------------------------------------- reference
def _taps(u, v, samp, H, W, swap=False):
    """The four taps of coordinates (u, v): [(row index, column index, weight, inside-and-sampled)].  The coordinate is clamped into
    [-2, W + 1] x [-2, H + 1] first, which changes no value: beyond -1 and W (H) every tap is outside."""
    u, v = u.clamp(-2.0, W + 1.0), v.clamp(-2.0, H + 1.0)
    x0, y0 = torch.floor(u), torch.floor(v)
    ax, ay = u - x0, v - y0
    wx, wy = (1.0 - ax, ax), (1.0 - ay, ay)
    x0, y0 = x0.long(), y0.long()
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            yi, xi = (y0 + dx, x0 + dy) if swap else (y0 + dy, x0 + dx)
            inside = samp & (yi >= 0) & (yi <= H - 1) & (xi >= 0) & (xi <= W - 1)
            out.append((yi, xi, wy[dy] * wx[dx], inside))
    return out


def _read(img, yi, xi, inside):
    B, C, H, W = img.shape
    idx = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
    val = img.reshape(B, C, H * W).gather(2, idx.reshape(B, C, H * W)).view(B, C, H, W)
    return torch.where(inside, val, torch.zeros_like(val))


def reference(inp, poses, K=None, mutate=None):
    """Float64 view (B, V, 3, H, W), disp and cover (B, V, 1, H, W) and their magnitudes for `poses`: dict(view, disp, cover, mag_view, mag_disp,
    mag_cover).  K: the source camera, for the precondition (None: not checked).  mutate: None, or a deliberate error for the host tests:
    'ey' (E_y negated), 'swap' (rows and columns of the taps swapped), 'novis' (both visibility tests dropped)."""
    dlog0, left, mn, mx = inp["dlog0"].to(f64), inp["left"].to(f64), inp["mn"].to(f64), inp["mx"].to(f64)
    B, N, H, W = dlog0.shape
    if K is not None:
        assert_margins(inp, poses, K)
    d = O.plane_disparities(mn.view(B, 1, 1), mx.view(B, 1, 1), N)  # (B, N)
    s = R.plane_shifts(inp["mn"], inp["mx"], N, W).view(B, N, 1, 1)
    views, disps, covers, mags = [], [], [], []
    for p in poses:
        ex, ey, ez = (float(e) for e in p[9:12])
        if mutate == "ey":
            ey = -ey
        qx, qy, qz = _rays(p, H, W)
        front = qz > 0
        if mutate == "novis":
            front = torch.ones_like(front)
        safe = torch.where(front, qz, torch.ones_like(qz))
        u0, v0 = (qx / safe).view(1, 1, H, W), (qy / safe).view(1, 1, H, W)
        w = 1.0 - s * ez
        u, v = s * ex + w * u0, s * ey + w * v0                                   # (B, N, H, W)
        samp = front.view(1, 1, H, W) & ((w > 0) if mutate != "novis" else torch.ones_like(w, dtype=torch.bool))
        samp = samp.expand(B, N, H, W)
        taps = _taps(u, v, samp, H, W, swap=mutate == "swap")
        lw = sum(wgt * _read(dlog0, yi, xi, ins) for yi, xi, wgt, ins in taps)    # not sampled, or every tap outside: 0
        omega = sum(torch.where(ins, wgt, torch.zeros_like(wgt)) for _, _, wgt, ins in taps)
        P = torch.softmax(lw, 1)
        view, mag = 0, 0
        for n in range(N):
            col, absn = 0, 0
            for yi, xi, wgt, ins in taps:
                t = _read(left, yi[:, n:n + 1].expand(B, 3, H, W), xi[:, n:n + 1].expand(B, 3, H, W), ins[:, n:n + 1].expand(B, 3, H, W))
                col = col + wgt[:, n:n + 1] * t
                absn = absn + t.abs()
            view = view + col * P[:, n:n + 1]
            mag = mag + absn * P[:, n:n + 1]
        views.append(view)
        mags.append(mag)
        disps.append((d.view(B, N, 1, 1) * P).sum(1, keepdim=True))
        covers.append((omega * P).sum(1, keepdim=True))
    disp, cover = torch.stack(disps, 1), torch.stack(covers, 1)
    return {"view": torch.stack(views, 1), "disp": disp, "cover": cover, "mag_view": torch.stack(mags, 1), "mag_disp": disp, "mag_cover": cover}


@functools.lru_cache(maxsize=None)
def cached_inputs(case, family, seed=0):
    return R.make_inputs(case, family, seed)


@functools.lru_cache(maxsize=None)
def cached(case, set_name, family, seed=0):
    """(inputs, poses, reference) of a listed comparison, computed once per process; callers must not modify any of them."""
    inp = cached_inputs(case, family, seed)
    poses = pose_set(case, set_name)
    return inp, poses, reference(inp, poses, case_camera(case))


def compare_outputs(case, got, ref, coefs=None):
    """[(output, pose index, comparator result)] of every output in `got` (dict of CPU tensors (B, V, C, H, W)) against `ref`."""
    out = []
    for k in ("view", "disp", "cover"):
        if got.get(k) is None:
            continue
        c = coef(k, case) if coefs is None else coefs[k]
        for v in range(ref[k].shape[1]):
            out.append((k, v, R.compare(got[k][:, v], ref[k][:, v], ref["mag_" + k][:, v], torch.float32, c)))
    return out
