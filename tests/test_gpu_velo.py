"""GPU: the Velodyne projection kernel (fal_net_amd/velodyne.py: project, csrc/velo.hip) against its definition on the host (tests/_velo_ref.py:
spec, which tests/test_velo_host.py ties to Monodepth's original formulation).  Every comparison is torch.equal: both sides do the same
correctly rounded float64 operations in the same order, and an integer minimum has no order, so there is no tolerance anywhere.  The device path
is never compared with itself, except where the property IS self-agreement (order independence, two runs)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _velo_ref as R  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import velodyne  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# (seed, H, W, points, scale of the first two rows of P); 13 x 7 with 257 points: the point count is no multiple of the block, nearly every pixel collides
SCANS = {"375x1242": (0, 375, 1242, 120000, 1.0), "37x124": (1, 37, 124, 5000, 0.1), "13x7": (5, 13, 7, 257, 0.01)}
DEPTH_BOUND, GATE = 2.8e-7, 1e-4  # tests/test_gpu_metrics.py: device metrics against the host chain, eigen mode


@functools.lru_cache(maxsize=None)
def scan_case(name, vel_depth=False):
    """(P, points, H, W, the host definition's map) of a seeded scan; computed once per session and left unchanged."""
    seed, H, W, n, scale = SCANS[name]
    P, pts = R.kitti_like_P(scale), R.seeded_scan(seed, n)
    return P, pts, H, W, R.spec(P, pts, H, W, vel_depth)


def device_map(P, pts, H, W, **kw):
    return velodyne.project(torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)).to(DEV), P, H, W, **kw)


def check(P, pts, H, W, tag, **kw):
    got = device_map(P, pts, H, W, **kw)
    want = torch.from_numpy(R.spec(P, pts, H, W, **kw))
    assert got.dtype == torch.float32 and tuple(got.shape) == (H, W) and got.is_cuda
    diff = int((got.cpu() != want).sum())
    print(f"{tag}: {int((want > 0).sum())} pixels set, {diff} differ")
    assert torch.equal(got.cpu(), want), tag
    return got.cpu().numpy()


# ---- seeded scans ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCANS))
def test_seeded_scan_equals_spec(name):
    P, pts, H, W, want = scan_case(name)
    got = device_map(P, pts, H, W).cpu()
    n_set, n_kept = int((want > 0).sum()), int((pts[:, 0] >= 0).sum())
    print(f"{name}: {n_set} of {H * W} pixels set by at most {n_kept} points, {int((got.numpy() != want).sum())} differ")
    assert n_set > 0 and (name != "13x7" or (len(pts) % 64 != 0 and n_set <= 20))  # 13 x 7: 79 points land on 20 pixels
    assert torch.equal(got, torch.from_numpy(want))


def test_vel_depth_equals_spec():
    P, pts, H, W, want = scan_case("37x124", True)
    got = device_map(P, pts, H, W, vel_depth=True).cpu()
    assert torch.equal(got, torch.from_numpy(want)) and not np.array_equal(want, scan_case("37x124")[4])


# ---- crafted points: one rule each ----------------------------------------------------------------------------------------------------------------
P_XYZ = np.array([[0.0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]])  # s = (y, z, x): u = rint(y / x) - 1, v = rint(z / x) - 1, depth x
P_YZ = np.array([[0.0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])   # s = (y, y, z): u = v = rint(y / z) - 1, depth z, whatever x >= 0 is


def test_two_points_on_one_pixel_in_both_orders():
    pts = np.array([[2, 6, 4, 0.5], [4, 12, 8, 0.25]], np.float32)  # both on (v, u) = (1, 2), depths 2 and 4
    for order in (pts, pts[::-1]):
        m = check(P_XYZ, order, 4, 5, "two points")
        assert m[1, 2] == 2 and m.sum() == 2


def test_negative_and_positive_depth_on_one_pixel_is_zero():
    pts = np.array([[1, -4, -2, 0], [1, 6, 3, 0], [1, 4, 4, 0], [1, -6, -2, 0]], np.float32)  # (1, 1): -2 and 3; (0, 0): 4; (2, 2): -2
    for order in (pts, pts[::-1]):
        m = check(P_YZ, order, 3, 3, "negative and positive")
        assert m[1, 1] == 0 and m[0, 0] == 4 and m[2, 2] == 0 and m.sum() == 4


def test_point_slightly_behind_is_dropped():
    behind = np.array([[-1e-6, 6, 3, 0]], np.float32)  # would land on (1, 1) with depth 3
    assert check(P_YZ, behind, 3, 3, "x slightly below 0").sum() == 0
    assert check(P_YZ, np.array([[0, 6, 3, 0], [-0.0, 4, 4, 0]], np.float32), 3, 3, "x = 0 and x = -0").tolist() == [[4, 0, 0], [0, 3, 0], [0, 0, 0]]


def test_borders_and_one_pixel_outside_each():
    H, W = 5, 7  # depth x = 1: u = y - 1, v = z - 1
    inside = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (2, 0), (2, W - 1), (0, 3), (H - 1, 3)]  # on every border and corner
    outside = [(-1, 3), (H, 3), (2, -1), (2, W), (-1, -1), (H, W)]  # one pixel beyond each
    pts = np.array([[1, u + 1, v + 1, 0] for v, u in inside + outside], np.float32)
    m = check(P_XYZ, pts, H, W, "borders")
    want = np.zeros((H, W), np.float32)
    for v, u in inside:
        want[v, u] = 1
    assert np.array_equal(m, want)
    assert check(P_XYZ, np.array([[1, u + 1, v + 1, 0] for v, u in outside], np.float32), H, W, "outside only").sum() == 0


def test_half_goes_to_even():
    # x = 2, y = 2 k + 1: s_0 / s_2 = k + 0.5 exactly; z = 2: v = 0
    pts = np.array([[2, 2 * k + 1, 2, 0] for k in range(6)], np.float32)  # 0.5 1.5 2.5 3.5 4.5 5.5 -> 0 2 2 4 4 6 -> u = -1 1 1 3 3 5
    m = check(P_XYZ, pts, 1, 7, "half to even")
    assert m.tolist() == [[0, 2, 0, 2, 0, 2, 0]]
    m = check(P_XYZ, np.array([[2, 5, 2, 0], [2, 7, 2, 0]], np.float32), 1, 7, "2.5 and 3.5")  # even k rounds down, odd k rounds up
    assert m.tolist() == [[0, 2, 0, 2, 0, 0, 0]]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_nan_and_infinity_in_each_coordinate(bad):
    for P, H, W, tag in ((P_XYZ, 4, 5, "integer P"), (R.kitti_like_P(0.1), 37, 124, "KITTI-like P")):
        good = np.array([2, 6, 4, 0], np.float32) if P is P_XYZ else np.array([10, 1, 0.5, 0], np.float32)
        pts = [good]
        for c in range(4):  # the reflectance too: it is ignored
            p = good.copy()
            p[c] = bad
            pts.append(p)
        m = check(P, np.stack(pts), H, W, f"{bad} {tag}")
        assert np.isfinite(m).all() and (m > 0).sum() == 1  # the good point (the bad reflectance lands on it too); nothing else


def test_s2_equal_zero():
    pts = np.array([[1, 6, 0, 0], [1, -6, 0, 0], [1, 0, 0, 0], [1, 4, 4, 0]], np.float32)  # y / 0 = inf, -inf, NaN; then one good point
    m = check(P_YZ, pts, 3, 3, "s_2 = 0")
    assert m[0, 0] == 4 and m.sum() == 4


def test_depth_beyond_f32_stays_infinite():
    P = np.array([[8.0, 0, 0, 0], [4, 0, 0, 0], [4, 0, 0, 0]])  # u = 1, v = 0, depth 4 x
    m = check(P, np.array([[3e38, 0, 0, 0]], np.float32), 2, 3, "depth beyond f32")
    assert np.isinf(m[0, 1]) and (m != 0).sum() == 1


def test_no_points_gives_zeros():
    out = torch.full((6, 9), float("nan"), device=DEV)
    got = velodyne.project(torch.empty((0, 4), device=DEV), R.kitti_like_P(), 6, 9, out=out)
    assert got is out and torch.equal(got.cpu(), torch.zeros(6, 9))


# ---- order independence, full write-out -------------------------------------------------------------------------------------------------------------
def test_any_order_of_the_points_gives_the_same_map():
    P, pts, H, W, want = scan_case("37x124")
    rng = np.random.default_rng(9)
    for _ in range(3):
        got = device_map(P, pts[rng.permutation(len(pts))], H, W)
        assert torch.equal(got.cpu(), torch.from_numpy(want))
    P, pts, H, W, want = scan_case("375x1242")
    first = device_map(P, pts, H, W)
    for _ in range(3):
        assert torch.equal(device_map(P, pts[rng.permutation(len(pts))], H, W), first)
    assert torch.equal(first.cpu(), torch.from_numpy(want))


def test_out_buffer_is_written_everywhere_twice():
    P, pts, H, W, want = scan_case("375x1242")
    maps = []
    for _ in range(2):
        out = torch.full((H, W), float("nan"), device=DEV)
        assert device_map(P, pts, H, W, out=out) is out
        assert not bool(torch.isnan(out).any())
        maps.append(out)
    assert torch.equal(maps[0], maps[1]) and torch.equal(maps[0].cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError, match="out"):
        device_map(P, pts, H, W, out=torch.empty((H, W + 1), device=DEV))


# ---- argument checks: a message, and the device stays usable ------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_the_next_call_is_correct():
    P, pts, H, W, want = scan_case("13x7")
    t = torch.from_numpy(pts).to(DEV)
    out = torch.full((H, W), -7.0, device=DEV)
    bad_P = np.array(P)
    bad_P[1, 2] = np.inf
    nan_P = np.array(P)
    nan_P[2, 3] = np.nan
    p12 = (L.C.c_double * 12)(*np.asarray(P).reshape(-1).tolist())
    cases = [
        ("H = 0", "pixels", lambda: velodyne.project(t, P, 0, W)),
        ("W < 0", "pixels", lambda: L.check(L.lib().falnet_velo_project(L.ptr(t), len(pts), p12, H, -3, 0, L.ptr(out), L.stream_ptr()), "velo_project")),
        ("H W = 2^31", "pixels", lambda: L.check(L.lib().falnet_velo_project(L.ptr(t), len(pts), p12, 1 << 16, 1 << 15, 0, L.ptr(out), L.stream_ptr()), "velo_project")),
        ("negative n_points", "negative", lambda: L.check(L.lib().falnet_velo_project(L.ptr(t), -1, p12, H, W, 0, L.ptr(out), L.stream_ptr()), "velo_project")),
        ("inf in P", r"\[1\]\[2\].*not finite", lambda: velodyne.project(t, bad_P, H, W, out=out)),
        ("NaN in P", r"\[2\]\[3\].*not finite", lambda: velodyne.project(t, nan_P, H, W, out=out)),
        ("null points", "null points", lambda: L.check(L.lib().falnet_velo_project(None, 5, p12, H, W, 0, L.ptr(out), L.stream_ptr()), "velo_project")),
        ("null output", "null output", lambda: L.check(L.lib().falnet_velo_project(L.ptr(t), len(pts), p12, H, W, 0, None, L.stream_ptr()), "velo_project")),
        ("CPU tensor", "no CPU fallback", lambda: velodyne.project(torch.from_numpy(pts), P, H, W)),
    ]
    for tag, word, call in cases:
        with pytest.raises(RuntimeError, match=word):
            call()
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), tag  # nothing ran
        assert torch.equal(velodyne.project(t, P, H, W).cpu(), torch.from_numpy(want)), tag  # and the next valid call is correct
    with pytest.raises(ValueError):
        velodyne.project(t[:, :3], P, H, W)
    with pytest.raises(ValueError):
        velodyne.project(t.double(), P, H, W)
    with pytest.raises(ValueError):
        velodyne.project(t, P[:2], H, W)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_npy_layout_equals_scan_layout(tmp_path):
    """One 375 x 1242 frame of a fake raw-KITTI tree through inference.evaluate (tests/_velo_eval.py; a process of its own because the
    deterministic mode that makes two forwards of one frame agree is chosen when the package is imported): the seven metrics over the
    tool's .npy and over the scan projected in the loop are EQUAL, with the host metrics and with the device metrics; between those two modes they
    sit within the eigen-mode bound of tests/test_gpu_metrics.py."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_velo_eval.py"), str(tmp_path)], capture_output=True, text=True, timeout=600,
                       cwd=ROOT, env=dict(os.environ, FALNET_DETERMINISTIC="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(out)
    from fal_net_amd import myUtils as utils
    assert out["npy_equals_spec"] and out["valid_pixels"] > 10000
    for mode in ("host", "device"):
        a, b = out["npy"][mode], out["scan"][mode]
        assert list(a) == list(b) == utils.kitti_error_names
        assert all(np.isfinite(v) for v in a.values()) and a["abs_rel"] > 0
        assert all(a[k] == b[k] for k in a), (mode, a, b)
    host, dev = np.array(list(out["scan"]["host"].values())), np.array(list(out["scan"]["device"].values()))
    err = float(np.max(np.abs(dev - host) / np.maximum(np.abs(host), 1e-300)))
    print(f"device metrics vs host metrics on the projected ground truth: worst rel {err:.3e}")
    assert err <= min(DEPTH_BOUND, GATE)
