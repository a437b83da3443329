"""GPU: the pseudo-LiDAR back-projection (fal_net_amd/pseudo_lidar.py: unproject, csrc/lidar.hip) against its definition on the host
(tests/_lidar_ref.py: unproject_ref, which tests/test_lidar_host.py closes into a loop with the projection's definition).  Every comparison with the
reference is torch.equal or byte equality: both sides do the same correctly rounded float64 operations in the same order and compare against the same
table values, and an integer minimum has no order, so there is no tolerance.  The one bound is the round trip's (roundtrip_bound: the f32 rounding of
a record).  The device path is never compared with itself, except where the property IS self-agreement (two runs)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lidar_ref as LR  # noqa: E402
import _velo_ref as R  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import pseudo_lidar, velodyne  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INF = float("inf")
# H, W, scale of the first two rows of P.  13 x 7: one partial wave; 37 x 124: 4588 pixels, three workgroup tiles of 2048 with a partial last one;
# 375 x 1242: 228 tiles, the native KITTI frame
SIZES = {"13x7": (13, 7, 0.01), "37x124": (37, 124, 0.1), "375x1242": (375, 1242, 1.0)}
# 513 x 1025: 525 825 pixels, 257 tiles -- one more than the offset scan takes at a time, so its carried base decides the last tile's offset
CARRY_SIZE = {"513x1025": (513, 1025, 1.0)}
GUARD_ROWS = 64
GUARD_WORD = 0x5A5AA5A5  # as f32 a large finite number no record holds


@functools.lru_cache(maxsize=None)
def frame(name):
    """The inputs of one size, computed once per session and left unchanged: P, fb, the road-like depth, its disparity, a score and an intensity map."""
    H, W, scale = {**SIZES, **CARRY_SIZE}[name]
    rng = np.random.default_rng(17)
    P, depth = R.kitti_like_P(scale), LR.road_depth(3, H, W)
    fb = 721.5377 * scale * 0.54
    with np.errstate(divide="ignore"):
        disp = np.where(depth > 0, fb / depth.astype(np.float64), 0.0).astype(np.float32)
    return dict(H=H, W=W, P=P, fb=fb, depth=depth, disp=disp, score=rng.random((H, W), dtype=np.float32), inten=rng.random((H, W), dtype=np.float32))


@functools.lru_cache(maxsize=None)
def reference(name, form, with_score, with_inten, max_height, beams=0, az_bins=1024):
    f = frame(name)
    return LR.unproject_ref(f[form], f["P"], fb=f["fb"] if form == "disp" else None, score=f["score"] if with_score else None,
                            threshold=0.5 if with_score else None, intensity=f["inten"] if with_inten else 0.25, max_height=max_height, beams=beams,
                            az_bins=az_bins)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(capacity):
    """A (capacity + GUARD_ROWS, 4) f32 buffer filled with the guard pattern; its first `capacity` rows are the output."""
    return torch.full(((capacity + GUARD_ROWS) * 4,), GUARD_WORD, dtype=torch.int32, device=DEV).view(torch.float32).view(-1, 4)


def check(map, P, want, tag, capacity=None, **kw):
    """unproject into a guarded buffer: the kept records are `want` byte for byte; nothing beyond them and nothing behind the buffer is written."""
    H, W = map.shape
    beams = kw.get("beams", 0)
    capacity = (H * W if beams == 0 else min(H * W, beams * kw.get("az_bins", 1024))) if capacity is None else capacity
    buf = guarded(capacity)
    for k in ("score", "intensity"):
        if isinstance(kw.get(k), np.ndarray):
            kw[k] = dev(kw[k])
    got = pseudo_lidar.unproject(dev(map), P, out=buf[:capacity], **kw)
    assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 2 and got.shape[1] == 4
    n = got.shape[0]
    assert n == 0 or got.data_ptr() == buf.data_ptr()
    differ = int((got.cpu().view(torch.int32) != torch.from_numpy(want).view(torch.int32)).any(1).sum()) if n == len(want) else -1
    print(f"{tag}: {n} points (reference {len(want)}), {differ} records differ")
    assert n == len(want) and got.cpu().numpy().tobytes() == want.tobytes(), tag
    assert bool((buf[n:].view(torch.int32) == GUARD_WORD).all()), tag + ": written beyond the kept records"
    return got


# ---- dense mode ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_height", [1.0, INF], ids=["h1", "hinf"])
@pytest.mark.parametrize("form", ["depth", "disp"])
@pytest.mark.parametrize("name", list(SIZES))
def test_dense_equals_reference(name, form, max_height):
    f = frame(name)
    sizes = []
    for with_score in (False, True):
        for with_inten in (False, True):
            want = reference(name, form, with_score, with_inten, max_height)
            check(f[form], f["P"], want, f"{name} {form} score={with_score} intensity map={with_inten} max_height={max_height}",
                  fb=f["fb"] if form == "disp" else None, score=f["score"] if with_score else None, threshold=0.5 if with_score else None,
                  intensity=f["inten"] if with_inten else 0.25, max_height=max_height)
            sizes.append(len(want))
    assert sizes[0] == sizes[1] > sizes[2] == sizes[3] > 0  # the score drops about half; the intensity map changes no count
    if max_height == INF and form == "depth":
        assert sizes[0] == int((f["depth"] > 0).sum()) >= len(reference(name, form, False, False, 1.0))


def test_dense_past_one_chunk_of_tile_counts():
    """257 tiles: the records of the last tile sit behind the total of the first 256, which only the scan's second round hands on."""
    name = "513x1025"
    f = frame(name)
    want = reference(name, "depth", True, True, 1.0)
    check(f["depth"], f["P"], want, f"{name} depth score=True intensity map=True max_height=1.0", score=f["score"], threshold=0.5, intensity=f["inten"],
          max_height=1.0)
    idx = LR.kept_records(f["depth"], f["P"], None, f["score"], 0.5, f["inten"], 0.0, 80.0, 1.0)[0]
    assert len(idx) == len(want) and 0 < int((idx >= 256 * 2048).sum()) < len(idx)  # kept pixels on both sides of the 257th tile's first pixel


# ---- beam mode ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,beams,az_bins", [("37x124", 8, 16), ("375x1242", 64, 1024)], ids=["37x124-8x16", "375x1242-64x1024"])
def test_beams_equal_reference(name, beams, az_bins):
    f = frame(name)
    in_range = len(reference(name, "depth", False, True, 1.0))
    for form in ("depth", "disp"):
        want = reference(name, form, False, True, 1.0, beams, az_bins)
        check(f[form], f["P"], want, f"{name} {beams} x {az_bins} {form}", fb=f["fb"] if form == "disp" else None, intensity=f["inten"], beams=beams,
              az_bins=az_bins)
        print(f"{name}: {in_range} points below the ceiling, {len(want)} of {beams * az_bins} bins hold a winner")
        assert 0 < len(want) <= beams * az_bins
        if name == "37x124":
            assert in_range > 10 * len(want)  # nearly every bin collides
        else:
            assert len(want) > 10000 and in_range > 4 * len(want)


def test_constant_depth_ties_go_to_the_lowest_pixel_index():
    H, W, scale = SIZES["37x124"]
    P, const = R.kitti_like_P(scale), np.full((H, W), 10.0, np.float32)
    kw = dict(max_height=INF, beams=8, az_bins=16, elevation=(-20.0, 20.0), azimuth=(-40.0, 40.0))
    want = LR.unproject_ref(const, P, **kw)
    got = check(const, P, want, "constant depth", **kw).cpu().numpy()
    # independently of the reference's minimum: every pixel has the same depth, so a bin's winner is its first pixel in row-major order
    idx, rec, _ = LR.kept_records(const, P, max_height=INF)
    te, ta = LR.edge_tables(8, 16, kw["elevation"], kw["azimuth"])
    x, y, z = (rec[:, i].astype(np.float64) for i in range(3))
    beam, col = np.searchsorted(te, z / np.sqrt(x * x + y * y), "right") - 1, np.searchsorted(ta, y / x, "right") - 1
    first = {}
    for i, (b, c) in enumerate(zip(beam.tolist(), col.tolist())):
        if 0 <= b < 8 and 0 <= c < 16:  # the frame is a little wider than 80 degrees: its outermost columns fall outside
            first.setdefault(b * 16 + c, i)
    assert (col < 0).any() or (col >= 16).any()
    assert len(first) == len(got) and len(idx) > 20 * len(got)
    assert np.array_equal(got, rec[[first[b] for b in sorted(first)]])


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------------------------
def test_nan_inf_zero_and_negative_values():
    H, W, scale = SIZES["13x7"]
    P = R.kitti_like_P(scale)
    depth = np.full((H, W), 12.0, np.float32)
    depth[0, :6] = [np.nan, np.inf, -np.inf, 0.0, -3.0, 80.0]
    depth[1, :3] = [np.nextafter(np.float32(80), np.float32(81)), 1e-30, -0.0]
    want = LR.unproject_ref(depth, P, max_height=INF)
    assert len(want) == H * W - 7  # all but 80 and 1e-30 of the nine are dropped
    check(depth, P, want, "bad depths", max_height=INF)
    disp = np.full((H, W), 2.0, np.float32)
    disp[2, :7] = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, 1e-38]  # 20 / 1e-38: a depth beyond f32, infinite, dropped by max_depth
    want = LR.unproject_ref(disp, P, fb=20.0, max_height=INF)
    assert len(want) == H * W - 7
    check(disp, P, want, "bad disparities", fb=20.0, max_height=INF)
    score = np.full((H, W), 0.75, np.float32)
    score[3, :4] = [np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.inf]
    want = LR.unproject_ref(disp, P, fb=20.0, score=score, threshold=0.5, max_height=INF)
    assert len(want) == H * W - 9
    check(disp, P, want, "NaN score", fb=20.0, score=score, threshold=0.5, max_height=INF)
    for beams in (0, 4):  # the same bad values through the key pass
        want = LR.unproject_ref(depth, P, max_height=INF, beams=beams, az_bins=8)
        check(depth, P, want, f"bad depths, beams={beams}", max_height=INF, beams=beams, az_bins=8)


@pytest.mark.parametrize("beams", [0, 8], ids=["dense", "beams"])
def test_a_map_that_keeps_nothing_writes_nothing(beams):
    f = frame("37x124")
    for tag, m, kw in (("zeros", np.zeros_like(f["depth"]), {}), ("NaN", np.full_like(f["depth"], np.nan), {}), ("too far", f["depth"], dict(max_depth=2.0)),
                       ("below the floor", f["depth"], dict(max_height=-1000.0)), ("behind", np.where(f["depth"] > 0, -f["depth"], np.float32(-5)), dict(min_depth=-100.0))):
        got = check(m, f["P"], np.zeros((0, 4), np.float32), tag, beams=beams, az_bins=16, **kw)
        assert tuple(got.shape) == (0, 4)


# ---- capacity, refusals -------------------------------------------------------------------------------------------------------------------------------
def raw_call(f, out_t, count_t, **change):
    """falnet_velo_unproject on the 37 x 124 depth map with one argument changed -> the return code."""
    lib = L.lib()
    k = dict(map=f["map_t"], fb=0.0, score=None, threshold=0.0, imap=None, intensity=1.0, Q=f["q12"], min_depth=0.0, max_depth=80.0, max_height=1.0, H=f["H"], W=f["W"],
             beams=0, az_bins=1024, te=None, ta=None, out=out_t, capacity=0 if out_t is None else out_t.shape[0], count=count_t, ws=f["ws"])
    k.update(change)
    as_ptr = lambda v: L.ptr(v) if torch.is_tensor(v) or v is None else v  # noqa: E731
    return lib.falnet_velo_unproject(as_ptr(k["map"]), k["fb"], as_ptr(k["score"]), k["threshold"], as_ptr(k["imap"]), k["intensity"], k["Q"], k["min_depth"],
                                     k["max_depth"], k["max_height"], k["H"], k["W"], k["beams"], k["az_bins"], as_ptr(k["te"]), as_ptr(k["ta"]), as_ptr(k["out"]),
                                     k["capacity"], as_ptr(k["count"]), as_ptr(k["ws"]), L.stream_ptr())


@functools.lru_cache(maxsize=None)
def raw_frame():
    f = dict(frame("37x124"))
    f["map_t"] = dev(f["depth"])
    f["q12"] = (L.C.c_double * 12)(*velodyne.backprojection_matrix(f["P"]).reshape(-1).tolist())
    f["ws"] = torch.zeros(int(L.lib().falnet_lidar_workspace_bytes(f["H"], f["W"], 128, 4096)) // 8, dtype=torch.int64, device=DEV)  # room for every case
    te, ta = pseudo_lidar.edge_tables(8, 16)
    f["te"], f["ta"] = dev(te), dev(ta)
    return f


@pytest.mark.parametrize("beams", [0, 8], ids=["dense", "beams"])
def test_capacity_overflow_reports_the_true_count(beams):
    f = raw_frame()
    want = reference("37x124", "depth", False, False, 1.0, beams, 16)
    cap = len(want) // 3
    assert cap > 0
    buf, count = guarded(cap), torch.full((1,), -7, dtype=torch.int64, device=DEV)
    rc = raw_call(f, buf[:cap], count, beams=beams, az_bins=16, te=f["te"] if beams else None, ta=f["ta"] if beams else None, intensity=0.25)
    torch.cuda.synchronize()
    print(f"beams={beams}: capacity {cap}, count {int(count)}, reference {len(want)}")
    assert rc == 0 and int(count) == len(want)
    assert buf[:cap].cpu().numpy().tobytes() == want[:cap].tobytes()
    assert bool((buf[cap:].view(torch.int32) == GUARD_WORD).all())
    with pytest.raises(RuntimeError, match=f"{len(want)} points are kept"):
        pseudo_lidar.unproject(f["map_t"], f["P"], intensity=0.25, beams=beams, az_bins=16, out=guarded(cap)[:cap])
    # capacity 0 with no output at all: the count alone
    count.fill_(-7)
    assert raw_call(f, None, count, beams=beams, az_bins=16, te=f["te"] if beams else None, ta=f["ta"] if beams else None) == 0
    assert int(count) == len(want)


def test_every_refused_argument_returns_nonzero_and_writes_nothing():
    f = raw_frame()
    want = reference("37x124", "depth", False, False, 1.0)
    cap = f["H"] * f["W"]
    buf, count = guarded(cap), torch.full((1,), -7, dtype=torch.int64, device=DEV)
    nan_q = (L.C.c_double * 12)(*([1.0] * 5 + [float("inf")] + [1.0] * 6))
    te, ta = f["te"], f["ta"]
    odd = buf.view(-1)[2:2 + 4 * 8].view(-1, 4)  # 8 bytes into a record: not 16-byte aligned
    cases = [("null map", dict(map=None), "null map"), ("null Q", dict(Q=None), "null back-projection"), ("null count", dict(count=None), "null count"),
             ("null workspace", dict(ws=None), "null count or workspace"), ("null output", dict(out=None), "null output"),
             ("beams without tables", dict(beams=8, az_bins=16), "null edge table"), ("beams without the azimuth table", dict(beams=8, az_bins=16, te=te), "null edge table"),
             ("H = 0", dict(H=0), "pixels"), ("W < 0", dict(W=-3), "pixels"), ("H W = 2^31", dict(H=1 << 16, W=1 << 15), "pixels"),
             ("beams < 0", dict(beams=-1, te=te, ta=ta), "beams"), ("beams = 129", dict(beams=129, te=te, ta=ta), "beams"),
             ("az_bins = 0", dict(beams=8, az_bins=0, te=te, ta=ta), "az_bins"), ("az_bins = 4097", dict(beams=8, az_bins=4097, te=te, ta=ta), "az_bins"),
             ("az_bins = 0, dense", dict(az_bins=0), "az_bins"),
             ("max_depth inf", dict(max_depth=INF), "max_depth"), ("max_depth NaN", dict(max_depth=float("nan")), "max_depth"),
             ("capacity < 0", dict(capacity=-1), "capacity"), ("fb < 0", dict(fb=-1.0), "fb"), ("fb inf", dict(fb=INF), "fb"),
             ("inf in Q", dict(Q=nan_q), r"\[1\]\[1\].*not finite"), ("misaligned output", dict(out=odd), "16-byte")]
    for tag, change, word in cases:
        rc = raw_call(f, buf[:cap], count, **change)
        torch.cuda.synchronize()
        assert rc != 0, tag
        with pytest.raises(RuntimeError, match=word):
            L.check(rc, "velo_unproject")
        assert int(count) == -7 and bool((buf.view(torch.int32) == GUARD_WORD).all()), tag  # nothing ran
    assert raw_call(f, buf[:cap], count, intensity=0.25) == 0  # and the next valid call is correct
    assert int(count) == len(want) and buf[:len(want)].cpu().numpy().tobytes() == want.tobytes()
    m = f["map_t"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pseudo_lidar.unproject(m.cpu(), f["P"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pseudo_lidar.unproject(m, f["P"], score=m.cpu(), threshold=0.5)
    for bad in (dict(score=m), dict(threshold=0.5), dict(score=m[:5], threshold=0.5), dict(intensity=m[:, :5]), dict(beams=-1), dict(beams=129), dict(beams=4, az_bins=0),
                dict(fb=-2.0), dict(fb=INF), dict(out=torch.empty((5, 3), device=DEV)), dict(out=torch.empty((5, 4), device=DEV, dtype=torch.float64)),
                dict(beams=4, elevation=(5.0, -5.0))):
        with pytest.raises(ValueError):
            pseudo_lidar.unproject(m, f["P"], **bad)
    with pytest.raises(ValueError):
        pseudo_lidar.unproject(m, f["P"][:2])
    with pytest.raises(RuntimeError, match="max_depth"):
        pseudo_lidar.unproject(m, f["P"], max_depth=INF)


# ---- two runs, the closed loop ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes():
    f = frame("375x1242")
    m, s = dev(f["disp"]), dev(f["score"])
    for kw in (dict(), dict(beams=64, az_bins=1024), dict(beams=128, az_bins=4096, elevation=(-30.0, 30.0))):
        a = pseudo_lidar.unproject(m, f["P"], fb=f["fb"], score=s, threshold=0.25, **kw)
        b = pseudo_lidar.unproject(m, f["P"], fb=f["fb"], score=s, threshold=0.25, **kw)
        assert a.shape[0] > 0 and a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32)), kw


@pytest.mark.parametrize("name", list(SIZES))
def test_project_of_unproject_is_the_depth(name):
    """The closed loop on the device: every kept pixel lands on itself and its depth comes back within roundtrip_bound; every other pixel is 0."""
    f = frame(name)
    H, W, P, depth = f["H"], f["W"], f["P"], f["depth"]
    pts = pseudo_lidar.unproject(dev(depth), P, max_height=INF)
    back = velodyne.project(pts, P, H, W).cpu().numpy().reshape(-1)
    idx, _, d = LR.kept_records(depth, P, max_height=INF)
    assert pts.shape[0] == len(idx) == int((depth > 0).sum())
    err = np.abs(back[idx].astype(np.float64) - d.astype(np.float64))
    bound = LR.roundtrip_bound(P, pts.cpu().numpy(), d)
    moved = int((back[idx] == 0).sum()) + int((np.delete(back, idx) != 0).sum())
    print(f"{name}: {len(idx)} kept pixels, {moved} moved, worst depth error {float((err / bound).max()):.3f} of the bound")
    assert moved == 0 and (err <= bound).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------
def _child(script, argv, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, cwd=ROOT, env=dict(os.environ, FALNET_DETERMINISTIC="1"), capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


@pytest.mark.parametrize("extra", [[], ["--pl-beams", "16", "--pl-az-bins", "128", "--pl-min-conf", "0.5"]], ids=["dense", "beams-conf"])
def test_cli_end_to_end(tmp_path, extra):
    H, W = 128, 416
    argv = ["--synthetic", "--height", str(H), "--width", str(W), "--iters", "1", "--pseudo-lidar"] + extra
    out = _child("Test_KITTI.py", argv + ["--save-path", str(tmp_path / "cli")])
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and list(lines[0]) == ["pseudo_lidar"] and "nominal camera" in out, out
    s = lines[0]["pseudo_lidar"]
    path = tmp_path / "cli" / "Pseudo_lidar" / "{:010d}.bin".format(0)
    scan = velodyne.load_scan(str(path))
    print(s)
    assert s["frames"] == 1 and s["points"] == s["mean_points"] == len(scan) and s["calibration"] == "nominal"
    assert s["kept_fraction"] == pytest.approx(len(scan) / (H * W)) and s["beams"] == (16 if extra else 0)
    assert np.isfinite(scan).all() and (scan[:, 0] > 0).all() and (scan[:, 2] <= 1.0).all() and (scan[:, 3] == 1.0).all()
    # the same command line once more, in a process that also records what the scan is made of: the same file, and its projection is the run's depth
    _child(os.path.join("tests", "_lidar_cli.py"), [str(tmp_path / "rec")] + argv + ["--save-path", str(tmp_path / "again")])
    assert open(tmp_path / "again" / "Pseudo_lidar" / "{:010d}.bin".format(0), "rb").read() == open(path, "rb").read()
    rec = np.load(tmp_path / "rec" / "frame_0.npz")
    P, fb, disp = rec["P"], float(rec["fb"]), rec["disp"]
    assert disp.shape == (H, W) and np.array_equal(P, velodyne.nominal_matrix(H, W, 721.5377 * W / 1242.0))
    depth = (fb / disp.astype(np.float64)).astype(np.float32).reshape(-1)
    back = velodyne.project(dev(scan), P, H, W).cpu().numpy().reshape(-1)
    kept = np.flatnonzero(back)
    xyz1 = np.c_[scan[:, :3].astype(np.float64), np.ones(len(scan))]
    sh = [xyz1 @ P[i] for i in range(3)]
    pix = (np.rint(sh[1] / sh[2]).astype(np.int64) - 1) * W + np.rint(sh[0] / sh[2]).astype(np.int64) - 1  # the pixel each point lands on
    assert np.array_equal(np.sort(pix), kept) and len(kept) == len(scan)  # every point on a pixel of its own
    err = np.abs(back[pix].astype(np.float64) - depth[pix].astype(np.float64))
    bound = LR.roundtrip_bound(P, scan, depth[pix])
    print(f"{len(kept)} points, worst depth error {float((err / bound).max()) if len(err) else 0.0:.3f} of the bound")
    assert (err <= bound).all()
    # and the file is the definition's scan of the recorded disparity (and confidence), byte for byte
    want = LR.unproject_ref(disp, P, fb=fb, score=rec["conf"] if extra else None, threshold=0.5 if extra else None, beams=16 if extra else 0, az_bins=128)
    assert scan.tobytes() == want.tobytes()
    if extra:
        assert rec["conf"].shape == (H, W) and (rec["conf"].reshape(-1)[pix] >= 0.5).all() and len(scan) <= 16 * 128
    else:
        assert len(scan) > 0


def test_cli_original_split_takes_each_frames_calibration(tmp_path):
    """Dataset mode on a one-frame raw-KITTI tree: the scan is made with the frame's own calibration files, settings.txt names the switches -- and the same
    command without --pseudo-lidar writes no folder, no extra line and a settings.txt without them."""
    from PIL import Image
    H, W = 375, 1242
    root, raw = tmp_path / "data" / "Kitti_eigen_test_original", tmp_path / "raw"
    drive, frm = "2011_09_26_drive_0002_sync", "0000000069"
    rng = np.random.default_rng(11)
    for cam in ("_02", "_03"):
        os.makedirs(root / (drive + cam))
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / (drive + cam) / (frm + ".jpg"))
    scan_dir = raw / "2011_09_26" / drive / "velodyne_points" / "data"
    os.makedirs(scan_dir)
    R.seeded_scan(4, 20000).tofile(scan_dir / (frm + ".bin"))
    R.write_calib(str(raw / "2011_09_26"))
    lst = tmp_path / "list.txt"
    lst.write_text(f"{drive}_02/{frm}.jpg {drive}_03/{frm}.jpg\n")
    argv = ["-d", str(tmp_path / "data"), "-tn", "Kitti_eigen_test_original", "--velodyne-root", str(raw), "--test_list", str(lst), "--allow-seeded-weights",
            "-w", "0", "-mspp", "False"]
    out = _child("Test_KITTI.py", argv + ["--save-path", str(tmp_path / "res"), "--pseudo-lidar", "--pl-beams", "64", "--pl-max-height", "inf"])
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and list(lines[0]) == ["pseudo_lidar"] and lines[1]["frames"] == 1 and "nominal camera" not in out, out
    s = lines[0]["pseudo_lidar"]
    scan = velodyne.load_scan(str(tmp_path / "res" / "Pseudo_lidar" / "{:010d}.bin".format(0)))
    print(s)
    assert s["calibration"] == "frame" and s["beams"] == 64 and s["az_bins"] == 1024 and s["points"] == len(scan) and 0 < len(scan) <= 64 * 1024
    back = velodyne.project(dev(scan), R.compose_P(), H, W).cpu().numpy()
    assert int((back > 0).sum()) == len(scan)  # through the frame's own matrix every point is back on a pixel of its own
    fb = velodyne.focal_baseline(str(raw / "2011_09_26"))
    assert float(back.max()) <= 80.0 and float(back[back > 0].min()) >= np.float32(fb / 300.0) * (1 - 1e-6)  # depth = fb / disparity, disparity <= max_disp
    with_pl = dict(ln.split(":", 1) for ln in open(tmp_path / "res" / "settings.txt").read().splitlines())
    assert with_pl["pl_beams".rjust(15)].strip() == "64" and with_pl["pseudo_lidar".rjust(15)].strip() == "True"
    out = _child("Test_KITTI.py", argv + ["--save-path", str(tmp_path / "plain")])
    assert len([ln for ln in out.splitlines() if ln.startswith("{")]) == 1 and not os.path.exists(tmp_path / "plain" / "Pseudo_lidar")
    plain = dict(ln.split(":", 1) for ln in open(tmp_path / "plain" / "settings.txt").read().splitlines())
    hidden = {k.strip() for k in with_pl} - {k.strip() for k in plain}
    assert hidden == {"pseudo_lidar", "pl_beams", "pl_az_bins", "pl_max_depth", "pl_max_height", "pl_min_conf", "pl_calib"}
    assert all(plain[k] == with_pl[k] for k in plain if k.strip() != "save_path")
