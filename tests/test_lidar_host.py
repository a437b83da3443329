"""CPU: the host side of the pseudo-LiDAR scans -- the definition of the back-projection (tests/_lidar_ref.py) closed into a loop with the definition
of the projection (tests/_velo_ref.py: spec), the matrices and calibration values of fal_net_amd/velodyne.py, the edge tables and the .bin file of
fal_net_amd/pseudo_lidar.py, the refusals that need no device and the command line.  No GPU."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import _lidar_ref as LR
import _velo_ref as R
from fal_net_amd import pseudo_lidar, velodyne

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- project(unproject(depth)) == depth -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,scale", [(375, 1242, 1.0), (37, 124, 0.1), (13, 7, 0.01)], ids=["375x1242", "37x124", "13x7"])
def test_round_trip_through_the_projection(H, W, scale):
    """Every kept pixel lands on itself, no exception, and its depth comes back within roundtrip_bound."""
    P, depth = R.kitti_like_P(scale), LR.road_depth(3, H, W)
    idx, pts, d = LR.kept_records(depth, P, max_height=np.inf)
    assert np.array_equal(pts, LR.unproject_ref(depth, P, max_height=np.inf)) and np.array_equal(d, depth.reshape(-1)[idx])
    back = R.spec(P, pts, H, W).reshape(-1)
    valid = np.flatnonzero((depth.reshape(-1) > 0) & (depth.reshape(-1) <= 80))
    moved = int((back[idx] == 0).sum()) + int((np.delete(back, idx) != 0).sum())
    err = np.abs(back[idx].astype(np.float64) - d.astype(np.float64))
    bound = LR.roundtrip_bound(P, pts, d)
    print(f"{H}x{W}: {len(idx)} of {len(valid)} valid pixels kept, {moved} moved, worst depth error {float((err / bound).max()):.3f} of the bound")
    assert len(idx) > 0.9 * len(valid) > 0.8 * H * W  # the road is in front of the sensor: the 5 % holes are what is missing
    assert moved == 0
    assert (err <= bound).all()


def test_reference_rules_on_crafted_maps():
    P = velodyne.nominal_matrix(4, 6, 2.0)
    m = np.array([[1, np.nan, np.inf, 0, -1, 81], [80, 1, 1, 1, 1, 1], [2, 2, 2, 2, 2, 2], [3, 3, 3, 3, 3, 3]], np.float32)
    idx, pts, d = LR.kept_records(m, P, max_height=np.inf)
    assert idx.tolist() == [0] + list(range(6, 24))  # NaN, inf, 0, negative and beyond max_depth are dropped; exactly max_depth is kept
    assert np.array_equal(pts[:, 0], d) and (pts[:, 3] == 1).all()  # the nominal camera: x is the depth
    low = LR.kept_records(m, P, max_height=0.0)[0]
    assert set(low) < set(idx) and all(i // 6 >= 1 for i in low)  # z <= 0: the rows at and below the principal point (v + 1 >= 2)
    score = np.full((4, 6), 0.5, np.float32)
    score[1, 0], score[1, 1] = np.nan, 0.25
    assert LR.kept_records(m, P, score=score, threshold=0.5, max_height=np.inf)[0].tolist() == [0] + list(range(8, 24))
    disp = np.array([[4, 0, -2, np.nan, np.inf, 0.01]], np.float32)  # fb 8: depths 2, -, -, -, 0, 800
    idx, pts, d = LR.kept_records(disp, velodyne.nominal_matrix(1, 6, 2.0), fb=8.0, max_height=np.inf)
    assert idx.tolist() == [0] and d.tolist() == [2.0]
    inten = np.arange(24, dtype=np.float32).reshape(4, 6)
    assert LR.kept_records(m, P, intensity=inten, max_height=np.inf)[1][:, 3].tolist() == [0.0] + list(map(float, range(6, 24)))


def test_beam_reference_keeps_the_nearest_and_then_the_lowest_index():
    H, W = 6, 8
    P = velodyne.nominal_matrix(H, W, 4.0)
    const = np.full((H, W), 5.0, np.float32)
    kw = dict(max_height=np.inf, beams=2, az_bins=2, elevation=(-60.0, 60.0), azimuth=(-60.0, 60.0))
    idx, rec, _ = LR.kept_records(const, P, max_height=np.inf)
    got = LR.unproject_ref(const, P, **kw)
    # a constant depth: every key differs in the pixel index only, so each of the four bins keeps its first pixel in row-major order.
    # The image's upper rows are the upper beam (z up is -v) and its LEFT columns the larger azimuth (y left is -u)
    x, y, z = (rec[:, i].astype(np.float64) for i in range(3))
    beam, col = (z / np.sqrt(x * x + y * y) >= 0).astype(int), (y / x >= 0).astype(int)
    want = [rec[np.flatnonzero((beam == b) & (col == c))[0]] for b in range(2) for c in range(2)]
    assert np.array_equal(got, np.stack(want)) and len(got) == 4
    near = const.copy()
    near[H - 1, W - 1] = 4.0  # the last pixel of its bin, but the nearest
    got = LR.unproject_ref(near, P, **kw)
    assert got[0, 0] == 4.0 and np.array_equal(got[1:], np.stack(want)[1:])  # lower beam, right half: bin (0, 0)


# ---- matrices and calibration -----------------------------------------------------------------------------------------------------------------------
def test_backprojection_matrix_inverts_the_projection():
    P = R.compose_P()
    Q = velodyne.backprojection_matrix(P)
    m_inv = np.linalg.inv(P[:, :3])
    assert Q.dtype == np.float64 and Q.shape == (3, 4)
    assert np.array_equal(Q[:, :3], m_inv) and np.array_equal(Q[:, 3], np.dot(m_inv, P[:, 3])) and np.array_equal(Q, LR.backprojection(P))
    X = np.array([12.0, -3.0, -1.2])
    s = P[:, :3] @ X + P[:, 3]
    assert np.allclose(Q[:, :3] @ s - Q[:, 3], X, rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="3 x 4"):
        velodyne.backprojection_matrix(P[:, :3])


def test_nominal_matrix_axes_and_centre():
    P = velodyne.nominal_matrix(375, 1242, 721.5377)
    assert np.array_equal(P, np.array([[621.0, -721.5377, 0, 0], [187.5, 0, -721.5377, 0], [1, 0, 0, 0]]))
    s = P @ np.array([10.0, 0.0, 0.0, 1.0])  # a point straight ahead lands on the principal point with depth x
    assert s[2] == 10 and s[0] / s[2] == 621 and s[1] / s[2] == 187.5
    assert (P @ np.array([10.0, 1.0, 0.0, 1.0]))[0] < s[0] and (P @ np.array([10.0, 0.0, 1.0, 1.0]))[1] < s[1]  # left is -u, up is -v
    with pytest.raises(ValueError):
        velodyne.nominal_matrix(0, 5, 1.0)


def test_focal_baseline_from_calibration_files(tmp_path):
    d = str(tmp_path / "2011_09_26")
    R.write_calib(d)
    f = R.P_RECT_02[0, 0]
    want = f * abs(R.P_RECT_02[0, 3] - R.P_RECT_03[0, 3]) / f
    assert velodyne.focal_baseline(d) == want == velodyne.focal_baseline(d, cam=3) and abs(want - 721.5377 * 0.5327) < 0.05
    assert np.array_equal(velodyne.backprojection_matrix(velodyne.projection_matrix(d)), LR.backprojection(R.compose_P()))
    R.write_calib(d, cam3=False)
    with pytest.raises(KeyError, match="P_rect_03"):
        velodyne.focal_baseline(d)
    with pytest.raises(ValueError):
        velodyne.focal_baseline(d, cam=1)


# ---- edge tables, the file, refusals without a device -------------------------------------------------------------------------------------------------
def test_edge_tables_and_their_refusals():
    te, ta = pseudo_lidar.edge_tables(64, 1024)
    rt, ra = LR.edge_tables(64, 1024)
    assert te.dtype == ta.dtype == np.float64 and te.shape == (65,) and ta.shape == (1025,)
    assert np.array_equal(te, rt) and np.array_equal(ta, ra) and (np.diff(te) > 0).all() and (np.diff(ta) > 0).all()
    assert te[0] == np.tan(np.deg2rad(-24.8)) and abs(ta[-1] - 1) < 1e-15
    for bad in (dict(beams=0), dict(beams=129), dict(az_bins=0), dict(az_bins=4097), dict(elevation=(2.0, -24.8)), dict(azimuth=(-90.0, 45.0)),
                dict(azimuth=(0.0, 90.0)), dict(elevation=(1.0, 1.0))):
        with pytest.raises(ValueError):
            pseudo_lidar.edge_tables(**dict(dict(beams=4, az_bins=8), **bad))


def test_write_bin_reads_back_as_a_scan(tmp_path):
    pts = R.seeded_scan(4, 33)
    path = str(tmp_path / "0000000000.bin")
    assert pseudo_lidar.write_bin(path, torch.from_numpy(pts)) == 33 and os.path.getsize(path) == 33 * 16
    assert np.array_equal(velodyne.load_scan(path), pts)
    assert pseudo_lidar.write_bin(path, pts[:0]) == 0 and velodyne.load_scan(path).shape == (0, 4)
    for bad in (pts.astype(np.float64), pts[:, :3], pts.reshape(-1)):
        with pytest.raises(ValueError):
            pseudo_lidar.write_bin(path, bad)


def test_unproject_refuses_cpu_tensors_and_the_writer_its_bad_parameters(tmp_path):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pseudo_lidar.unproject(torch.ones(3, 4), R.kitti_like_P())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pseudo_lidar.unproject(np.ones((3, 4), np.float32), R.kitti_like_P())
    for bad in (dict(beams=200), dict(beams=4, az_bins=5000), dict(min_conf=0.0), dict(min_conf=1.5), dict(max_depth=float("inf")),
                dict(max_depth=0.0), dict(beams=4, elevation=(10.0, -10.0))):
        with pytest.raises(ValueError):
            pseudo_lidar.PseudoLidarWriter(str(tmp_path), **bad)
    w = pseudo_lidar.PseudoLidarWriter(str(tmp_path), beams=16, az_bins=128, min_conf=0.5)
    assert os.path.isdir(tmp_path / "Pseudo_lidar") and w.file(7).endswith(os.path.join("Pseudo_lidar", "0000000007.bin"))
    s = w.summary()
    assert s["frames"] == 0 and s["points"] == 0 and s["beams"] == 16 and s["az_bins"] == 128 and s["min_conf"] == 0.5 and np.isnan(s["mean_points"])
    with pytest.raises(ValueError, match="confidence"):
        w.write(0, torch.ones(1, 1, 3, 4), R.kitti_like_P(), 100.0)


# ---- command line -------------------------------------------------------------------------------------------------------------------------------------
def test_parser_and_what_settings_hide(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    mod = importlib.import_module("Test_KITTI")
    a = mod.parser.parse_args([])
    assert (a.pseudo_lidar, a.pl_beams, a.pl_az_bins, a.pl_max_depth, a.pl_max_height, a.pl_min_conf, a.pl_calib) == (False, 0, 1024, 80.0, 1.0, None, None)
    mod.check_family_args(a)
    assert set(mod.LIDAR_ARGS) <= set(vars(a)) and all(n.startswith(("pseudo_lidar", "pl_")) for n in mod.LIDAR_ARGS)
    assert set(mod.LIDAR_ARGS) <= set(mod.hidden_settings(a))  # settings.txt keeps its lines without --pseudo-lidar
    assert not set(mod.LIDAR_ARGS) & set(mod.hidden_settings(mod.parser.parse_args(["--pseudo-lidar"])))
    a = mod.parser.parse_args(["--pseudo-lidar", "--pl-beams", "64", "--pl-az-bins", "512", "--pl-max-depth", "60", "--pl-max-height", "inf",
                               "--pl-min-conf", "0.5", "--pl-calib", "/calib"])
    assert (a.pseudo_lidar, a.pl_beams, a.pl_az_bins, a.pl_max_depth, a.pl_max_height, a.pl_min_conf, a.pl_calib) == (True, 64, 512, 60.0, float("inf"), 0.5, "/calib")
    mod.check_family_args(a)
    for bad in (["--pl-beams", "129"], ["--pl-beams", "-1"], ["--pl-az-bins", "0"], ["--pl-az-bins", "4097"], ["--pl-max-depth", "inf"],
                ["--pl-max-depth", "0"], ["--pl-min-conf", "0"], ["--pl-min-conf", "1.5"]):
        with pytest.raises(SystemExit):
            mod.parser.parse_args(["--pseudo-lidar"] + bad)
    for alone in (["--pl-beams", "8"], ["--pl-min-conf", "0.5"], ["--pl-calib", "/calib"], ["--pl-max-height", "2"]):
        with pytest.raises(SystemExit, match="--pseudo-lidar"):
            mod.check_family_args(mod.parser.parse_args(alone))
    for name in ("save", "save_pc"):  # the reference's switches stay refused, with or without the new one
        with pytest.raises(SystemExit, match="out of scope"):
            mod.refuse_out_of_scope(mod.parser.parse_args(["--pseudo-lidar", "-" + name, "True"]))


def test_where_the_calibration_comes_from(tmp_path, monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    mod = importlib.import_module("Test_KITTI")
    from fal_net_amd import datasets as DS
    from fal_net_amd import metrics
    from fal_net_amd.myUtils import width_to_focal
    d = str(tmp_path / "2011_09_26")
    R.write_calib(d)
    # nominal: a KITTI width takes its own focal length and the eigen focal x baseline; another width the 1242-pixel camera scaled to it
    get, source = mod.lidar_calibration(mod.parser.parse_args(["--pseudo-lidar"]))
    P, fb = get(0, 375, 1242)
    assert source == "nominal" and np.array_equal(P, velodyne.nominal_matrix(375, 1242, width_to_focal[1242])) and fb == metrics.focal_baseline("eigen", 1242)
    P, fb = get(0, 128, 416)
    f = width_to_focal[1242] * 416 / 1242.0
    assert np.array_equal(P, velodyne.nominal_matrix(128, 416, f)) and abs(fb - f * 0.9982 * 0.54) < 1e-9
    # --pl-calib: one directory for every frame; a missing one stops before the first frame
    get, source = mod.lidar_calibration(mod.parser.parse_args(["--pseudo-lidar", "--pl-calib", d]))
    P, fb = get(5, 375, 1242)
    assert source == "pl-calib" and np.array_equal(P, R.compose_P()) and fb == velodyne.focal_baseline(d)
    with pytest.raises(FileNotFoundError):
        mod.lidar_calibration(mod.parser.parse_args(["--pseudo-lidar", "--pl-calib", str(tmp_path / "nowhere")]))
    # the original split with raw scans: each frame's own calibration directory, camera --velodyne-cam
    triples = [("l", "r", DS.VeloRef("scan.bin", d))]
    get, source = mod.lidar_calibration(mod.parser.parse_args(["--pseudo-lidar", "--velodyne-cam", "3"]), triples)
    P, fb = get(0, 375, 1242)
    assert source == "frame" and np.array_equal(P, R.compose_P(R.P_RECT_03)) and fb == velodyne.focal_baseline(d, 3)
    assert mod.lidar_calibration(mod.parser.parse_args(["--pseudo-lidar"]), [("l", "r", "gt.png")])[1] == "nominal"


def test_entry_points_in_header_binding_and_build():
    from fal_net_amd import _build, _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "falnet_hip.h")).read(), flags=re.S)
    assert re.search(r"\bfalnet_velo_unproject\s*\(", hdr) and re.search(r"\bfalnet_lidar_workspace_bytes\s*\(", hdr)
    sig = _lib.SIGNATURES["falnet_velo_unproject"]
    assert len(sig) == 21 and sig[-1] is _lib._P and sig[1] is _lib._D and sig[17] is _lib._L
    assert _lib.SIGNATURES["falnet_lidar_workspace_bytes"] == [_lib._I] * 4 and _lib._RESTYPES["falnet_lidar_workspace_bytes"] is _lib.C.c_int64
    assert "lidar.hip" in _build.SOURCES and _build.FILE_FLAGS["lidar.hip"] == ["-ffp-contract=off"]
    assert "lidar.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600  # the packaged autotune cache stays valid
    src = open(os.path.join(_build.CSRC, "lidar.hip")).read()
    assert "atomicMin" in src and "atomicAdd" not in src  # one integer minimum, nothing that depends on arrival order
    assert "rec_bytes == 4 || rec_bytes == 15" in open(os.path.join(_build.CSRC, "compact.hip")).read()  # compact.hip keeps refusing 16-byte records


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "fal_net_amd", "libfalnet_hip.so")), reason="library not built")
def test_workspace_bytes_and_refusals_without_a_device():
    """The size function and every argument check run before anything touches the device."""
    from fal_net_amd import _lib as L
    lib = L.lib()
    assert lib.falnet_lidar_workspace_bytes(375, 1242, 0, 1024) == 8 * ((375 * 1242 + 2047) // 2048)
    assert lib.falnet_lidar_workspace_bytes(375, 1242, 64, 1024) == 8 * (65536 + 32)
    assert lib.falnet_lidar_workspace_bytes(1, 1, 1, 1) == 16
    for bad in ((0, 5, 0, 1), (5, -1, 0, 1), (1 << 16, 1 << 15, 0, 1), (5, 5, -1, 1), (5, 5, 129, 1), (5, 5, 4, 0), (5, 5, 4, 4097), (5, 5, 0, 0)):
        assert lib.falnet_lidar_workspace_bytes(*bad) == 0, bad
    q = (L.C.c_double * 12)(*LR.backprojection(R.kitti_like_P()).reshape(-1).tolist())
    fake = L.C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
    base = dict(map=fake, fb=0.0, score=None, threshold=0.0, imap=None, intensity=1.0, Q=q, min_depth=0.0, max_depth=80.0, max_height=1.0, H=5, W=7, beams=0,
                az_bins=1024, te=None, ta=None, out=fake, capacity=35, count=fake, ws=fake, stream=None)
    nan_q = (L.C.c_double * 12)(*([float("nan")] + [1.0] * 11))
    cases = [("null map", dict(map=None), "null map"), ("null Q", dict(Q=None), "null back-projection"), ("null count", dict(count=None), "null count"),
             ("null workspace", dict(ws=None), "null count or workspace"), ("null output", dict(out=None), "null output"),
             ("null tables", dict(beams=4, az_bins=8), "null edge table"), ("null azimuth table", dict(beams=4, az_bins=8, te=fake), "null edge table"),
             ("H = 0", dict(H=0), "pixels"), ("W < 0", dict(W=-3), "pixels"), ("H W = 2^31", dict(H=1 << 16, W=1 << 15), "pixels"),
             ("beams < 0", dict(beams=-1), "beams"), ("beams > 128", dict(beams=129, te=fake, ta=fake), "beams"),
             ("az_bins = 0", dict(beams=4, az_bins=0, te=fake, ta=fake), "az_bins"), ("az_bins > 4096", dict(beams=4, az_bins=4097, te=fake, ta=fake), "az_bins"),
             ("max_depth inf", dict(max_depth=float("inf")), "max_depth"), ("max_depth NaN", dict(max_depth=float("nan")), "max_depth"),
             ("capacity < 0", dict(capacity=-1), "capacity"), ("fb < 0", dict(fb=-1.0), "fb"), ("fb NaN", dict(fb=float("nan")), "fb"),
             ("NaN in Q", dict(Q=nan_q), r"\[0\]\[0\].*not finite"), ("misaligned output", dict(out=L.C.c_void_p((1 << 20) + 8)), "16-byte"),
             ("misaligned count", dict(count=L.C.c_void_p((1 << 20) + 4)), "8-byte")]
    for tag, change, word in cases:
        k = dict(base, **change)
        rc = lib.falnet_velo_unproject(k["map"], k["fb"], k["score"], k["threshold"], k["imap"], k["intensity"], k["Q"], k["min_depth"], k["max_depth"],
                                       k["max_height"], k["H"], k["W"], k["beams"], k["az_bins"], k["te"], k["ta"], k["out"], k["capacity"], k["count"],
                                       k["ws"], k["stream"])
        assert rc != 0, tag
        assert re.search(word, lib.falnet_last_error().decode()), (tag, lib.falnet_last_error().decode())
