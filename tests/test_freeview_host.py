"""CPU: the pose algebra of fal_net_amd/freeview.py against the explicit 3-D construction, the float64 reference of the free-viewpoint plane sweep
(tests/_freeview_ref.py) held to account -- against the baseline sweep's reference, against mutations of itself, its precondition on every
listed (case, pose set) --, the --freeview command line, the wrapper's refusals and the binding's signature.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

import _freeview_ref as F
import _head_ref as R
import _sweep_ref as S

f64 = torch.float64
CASE = F.CASES[1]  # (2, 7, 5, 40, 30)


def _K():
    return np.array([[700.0, 0.0, 620.5], [0.0, 690.0, 187.0], [0.0, 0.0, 1.0]])


def test_pose_is_the_explicit_3d_construction():
    """The source pixel (u_n, v_n) of a target pixel, lifted to depth z_n = fx b / s_n, moved by X_t = R (X_s - c) and projected with K_t, lands
    back on the target pixel, for poses with every degree of freedom in use."""
    from fal_net_amd import freeview as FV
    K, b = _K(), 0.54
    rng = np.random.default_rng(0)
    for kw in (dict(centre=(0.4, -0.3, 0.2), roll=10.0, zoom=1.3), dict(centre=(-1.2, 0.5, -0.7), yaw=-4.0, pitch=2.5, roll=-20.0, zoom=0.8),
               dict(centre=(0.1, 0.2, 0.3), yaw=7.0, K_t=np.array([[500.0, 0.0, 300.0], [0.0, 510.0, 200.0], [0.0, 0.0, 1.0]]))):
        p = FV.pose(K, **kw)
        assert p.dtype == np.float64 and p.shape == (12,)
        A, E = p[:9].reshape(3, 3), p[9:]
        Kt = np.array(kw.get("K_t", K), dtype=np.float64)
        Kt[0, 0] *= kw.get("zoom", 1.0)
        Kt[1, 1] *= kw.get("zoom", 1.0)
        Rm = FV.rotation(kw.get("yaw", 0.0), kw.get("pitch", 0.0), kw.get("roll", 0.0))
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(Rm) - 1.0) < 1e-14
        c = np.asarray(kw["centre"]) * b  # metres
        worst = 0.0
        for _ in range(200):
            x, y = rng.uniform(0, 1241), rng.uniform(0, 374)
            s = rng.uniform(2.0, 300.0)  # pixels of disparity: the plane Z = fx b / s
            q = A @ np.array([x, y, 1.0])
            w = 1.0 - s * E[2]
            u, v = s * E[0] + w * q[0] / q[2], s * E[1] + w * q[1] / q[2]
            z = K[0, 0] * b / s
            Xs = z * np.linalg.solve(K, np.array([u, v, 1.0]))
            Xt = Rm @ (Xs - c)
            proj = Kt @ Xt
            assert (q[2] > 0 and w > 0) == (Xt[2] > 0 and q[2] > 0)  # sampled iff in front of both cameras (z > 0 in the source by construction)
            worst = max(worst, abs(proj[0] / proj[2] - x), abs(proj[1] / proj[2] - y))
        assert worst < 1e-9, (kw, worst)


def test_pose_special_cases():
    from fal_net_amd import freeview as FV
    K = _K()
    p = FV.pose(K)
    assert np.allclose(p[:9].reshape(3, 3), np.eye(3), rtol=0, atol=1e-12) and (p[9:] == 0.0).all()
    for t in (1.0, -0.5, 1.9):
        p = FV.pose(K, centre=(t, 0.0, 0.0))
        assert np.allclose(p[:9].reshape(3, 3), np.eye(3), rtol=0, atol=1e-12) and p[9] == t and p[10] == 0.0 and p[11] == 0.0
    p = FV.pose(K, zoom=2.0)  # the target pixel at the principal point looks along the axis; a step of one target pixel is half a source pixel
    A = p[:9].reshape(3, 3)
    assert np.allclose(A @ np.array([620.5, 187.0, 1.0]), [620.5, 187.0, 1.0]) and np.allclose(A @ np.array([622.5, 187.0, 1.0]), [621.5, 187.0, 1.0])
    # the nominal camera
    K = FV.camera(375, 1242)
    assert K[0, 0] == 721.5377 and K[1, 1] == 721.5377 and K[0, 2] == 620.5 and K[1, 2] == 187.0
    K = FV.camera(64, 128)
    assert K[0, 0] == 721.5377 * 128 / 1242 and K[0, 2] == 63.5 and K[1, 2] == 31.5
    K = FV.camera(10, 20, fx=5.0, cy=2.0)
    assert K.tolist() == [[5.0, 0.0, 9.5], [0.0, 5.0, 2.0], [0.0, 0.0, 1.0]]
    # this file's own construction of the pose sets agrees with the module's
    Kc = F.case_camera(CASE)
    assert np.array_equal(F.make_pose(Kc, centre=(0.4, -0.3, 0.2), roll=10.0, zoom=1.3), FV.pose(Kc, centre=(0.4, -0.3, 0.2), roll=10.0, zoom=1.3))


def test_paths():
    from fal_net_amd.freeview import paths
    o = paths.orbit(8, 0.5, 0.25, yaw=3.0)
    assert len(o) == 8 and o[0]["centre"] == (0.5, 0.0, 0.0) and o[0]["yaw"] == 3.0 and o[0]["pitch"] == 0.0
    assert np.allclose(o[2]["centre"], (0.0, 0.25, 0.0), atol=1e-15) and np.allclose(o[4]["centre"], (-0.5, 0.0, 0.0), atol=1e-15) and abs(o[4]["yaw"] + 3.0) < 1e-15
    assert np.allclose(o[-1]["centre"], (0.5 * math.cos(2 * math.pi * 7 / 8), 0.25 * math.sin(2 * math.pi * 7 / 8), 0.0))  # one step before the loop closes
    d = paths.dolly(5, -0.5, 0.5)
    assert len(d) == 5 and d[0] == {"centre": (0.0, 0.0, -0.5)} and d[-1] == {"centre": (0.0, 0.0, 0.5)} and d[2] == {"centre": (0.0, 0.0, 0.0)}
    p = paths.pan(3, -3.0, 3.0)
    assert p == [{"yaw": -3.0}, {"yaw": 0.0}, {"yaw": 3.0}]
    assert paths.dolly(1, 0.25, 1.0) == [{"centre": (0.0, 0.0, 0.25)}] and paths.pan(1, 2.0, 5.0) == [{"yaw": 2.0}] and len(paths.orbit(1, 1, 1)) == 1


@pytest.mark.parametrize("case", [CASE, (2, 49, 9, 128, 300.0)])
def test_pure_baseline_poses_are_the_sweeps_reference(case):
    inp = R.make_inputs(case, "a")
    ts = (1.0, -0.5, 1.9)
    ref = F.reference(inp, F.pose_set(case, "S"), F.case_camera(case))
    sref = S.reference(inp, ts)
    assert float((ref["view"] - sref["view"]).abs().max()) <= 1e-12 and float((ref["disp"] - sref["disp"]).abs().max()) <= 1e-12
    # cover: the in-range tap weights of the shifted row
    B, N, H, W = inp["dlog0"].shape
    shifts = R.plane_shifts(inp["mn"], inp["mx"], N, W)
    x = torch.arange(W, dtype=f64).view(1, 1, 1, W)
    for v, t in enumerate(ts):
        s = (shifts * t).view(B, N, 1, 1)
        k = torch.floor(s)
        a = s - k
        i0, i1 = x + k, x + k + 1
        omega = (1 - a) * ((i0 >= 0) & (i0 <= W - 1)) + a * ((i1 >= 0) & (i1 <= W - 1))
        P = torch.softmax(S.O.shift_planes(inp["dlog0"].to(f64), shifts * t), 1)
        want = (omega * P).sum(1, keepdim=True)
        assert float((ref["cover"][:, v] - want).abs().max()) <= 1e-12, t
    assert bool((ref["mag_view"] >= ref["view"].abs()).all()) and bool((ref["cover"] >= 0).all()) and bool((ref["cover"] <= 1 + 1e-15).all())


@pytest.mark.parametrize("case", [CASE, (1, 9, 4, 77, 120.0)])
def test_identity_is_the_left_image_and_the_forwards_disparity(case):
    inp = R.make_inputs(case, "b")
    ref = F.reference(inp, F.pose_set(case, "I"), F.case_camera(case))
    assert float((ref["view"][:, 0] - inp["left"].to(f64)).abs().max()) <= 1e-15
    assert float((ref["disp"][:, 0] - S.forward_disp(inp)).abs().max()) <= 1e-12
    assert float((ref["cover"] - 1.0).abs().max()) <= 1e-15


def test_turned_away_sees_nothing_and_dolly_drops_the_near_planes():
    inp = R.make_inputs(CASE, "a")
    ref = F.reference(inp, F.pose_set(CASE, "O"), F.case_camera(CASE))
    assert not bool(ref["view"].any()) and not bool(ref["cover"].any())
    B, N, H, W = inp["dlog0"].shape
    d = S.O.plane_disparities(inp["mn"].to(f64), inp["mx"].to(f64), N)
    assert float((ref["disp"][:, 0] - d.mean(1).view(B, 1, 1, 1)).abs().max()) <= 1e-12  # every logit 0: the uniform expectation
    p = F.pose_set(CASE, "D")[0]
    w = 1.0 - R.plane_shifts(inp["mn"], inp["mx"], N, W) * p[11]
    assert bool((w[:, -1] < 0).all()) and bool((w[:, 0] > 0).all())  # nearest plane behind the target camera, farthest in front


def test_precondition_of_every_listed_case_and_pose_set():
    """What keeps the GPU test from dropping cases: every (case, pose set) the issue lists is there and passes the precondition."""
    assert F.CASES == [(1, 2, 3, 40, 30.0), (2, 7, 5, 40, 30.0), (1, 9, 4, 77, 120.0), (1, 7, 19, 70, 30.0), (2, 49, 9, 128, 300.0),
                       (1, 128, 3, 64, 300.0), (1, 49, 2, 1242, 300.0)]
    assert F.SET_NAMES == ("I", "S", "D", "Y", "G", "O", "F", "N9")
    assert set(F.families(F.CASES[0])) == set("abcd") and set(F.families(F.CASES[1])) == set("abcd") and F.families(F.CASES[2]) == ("a", "b")
    assert len(F.listed()) == (4 + 4 + 2 * 5) * 8
    for case in F.CASES:
        inp = R.make_inputs(case, "a")
        K = F.case_camera(case)
        for name in F.SET_NAMES:
            poses = F.pose_set(case, name)
            wm, qm = F.assert_margins(inp, poses, K)
            assert wm >= F.WMARGIN and qm >= F.QMARGIN
            assert len(poses) == {"S": 3, "F": 8, "N9": 9}.get(name, 1)
        p = F.pose_set(case, "D")[0]
        s = R.plane_shifts(inp["mn"], inp["mx"], case[1], case[3])
        assert float(s.max() * p[11]) > 1.0  # s_max E_z > 1
        qz = F._rays(F.pose_set(case, "O")[0], case[2], case[3])[2]
        assert bool((qz < 0).all())
    # ... and the precondition does refuse: a plane on the target camera's own plane, a ray in the source image plane
    inp = R.make_inputs(CASE, "a")
    K = F.case_camera(CASE)
    s = R.plane_shifts(inp["mn"], inp["mx"], CASE[1], CASE[3])
    on_plane = np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.0 / float(s[0, 3])]])
    with pytest.raises(AssertionError):
        F.reference(inp, [on_plane], K)
    with pytest.raises(AssertionError):
        F.reference(inp, [F.make_pose(K, yaw=90.0 + math.degrees(math.atan2(10.0 - K[0, 2], K[0, 0])))], K)


@pytest.mark.parametrize("mutation,set_name", [("ey", "G"), ("swap", "G"), ("novis", "D")])
def test_mutations_break_the_bound(mutation, set_name):
    """The bound the GPU test uses is not vacuous: a reference with E_y negated, with the rows and columns of the taps swapped, or without the
    visibility tests lies outside it."""
    for case in (CASE, (2, 49, 9, 128, 300.0)):
        inp = R.make_inputs(case, "a")
        poses = F.pose_set(case, set_name)
        ref = F.reference(inp, poses, F.case_camera(case))
        wrong = F.reference(inp, poses, mutate=mutation)
        res = F.compare_outputs(case, {k: wrong[k].to(torch.float32) for k in ("view", "disp", "cover")}, ref)
        clean = F.compare_outputs(case, {k: ref[k].to(torch.float32) for k in ("view", "disp", "cover")}, ref)
        assert not [r for _, _, r in clean if r["bad"]]  # rounding the reference itself to float32 stays inside
        for what, v, r in res:
            assert r["bad"] > 0, (case, mutation, what, r)


def test_coefficients_follow_the_rule():
    for out in ("view", "disp", "cover"):
        for cls in ("d30", "wide"):
            c = F.COEF[out][cls]
            assert c is not None and math.log2(c) == round(math.log2(c)), (out, cls, c)
    for cls in ("d30", "wide"):  # with f64 coordinates the pure-baseline poses need no more than the sweep: nor does any pose here
        assert F.COEF["view"][cls] <= S.COEF["view"][cls] and F.COEF["disp"][cls] <= S.COEF["disp"][cls]
    assert F.coef("view", CASE) == F.COEF["view"]["d30"] and F.coef("cover", (1, 9, 4, 77, 120.0)) == F.COEF["cover"]["wide"]


def test_command_line():
    import Test_KITTI as T
    a = T.parser.parse_args([])
    assert a.freeview is None and a.freeview_path == "orbit" and a.freeview_amp == [0.5, 0.25, 0.5] and a.freeview_yaw == 3.0
    assert T.freeview_poses(a) is None
    a = T.parser.parse_args(["--freeview", "4"])
    poses = T.freeview_poses(a)
    assert len(poses) == 4 and poses[0] == {"centre": (0.5, 0.0, 0.0), "yaw": 3.0, "pitch": 0.0}
    a = T.parser.parse_args(["--freeview", "3", "--freeview-path", "dolly", "--freeview-amp", "1", "2", "0.75"])
    assert T.freeview_poses(a) == [{"centre": (0.0, 0.0, 0.0)}, {"centre": (0.0, 0.0, 0.375)}, {"centre": (0.0, 0.0, 0.75)}]
    a = T.parser.parse_args(["--freeview", "2", "--freeview-path", "pan", "--freeview-yaw", "5"])
    assert T.freeview_poses(a) == [{"yaw": -5.0}, {"yaw": 5.0}]
    for bad in (["--freeview", "0"], ["--freeview", "-2"], ["--freeview", "3", "--freeview-path", "spiral"], ["--freeview-amp", "1", "2"]):
        with pytest.raises(SystemExit):
            T.parser.parse_args(bad)
    with pytest.raises(SystemExit):  # the -save* switches stay refused
        T.refuse_out_of_scope(T.parser.parse_args(["-save", "True", "--freeview", "3"]))
    assert set(T.FREEVIEW_ARGS) <= set(vars(a))
    assert not set(T.FREEVIEW_ARGS) & set(T.hidden_settings(a))  # settings.txt keeps its lines without the switch
    assert set(T.FREEVIEW_ARGS) <= set(T.hidden_settings(T.parser.parse_args([])))


def test_wrapper_checks_need_no_device():
    from fal_net_amd import freeview as FV
    K = FV.camera(2, 8)
    good = FV.pose(K, centre=(0.5, 0.0, 0.0))
    assert FV.check_poses([good, (np.eye(3), np.zeros(3))]).shape == (2, 12)
    nan, flat = good.copy(), good.copy()
    nan[2] = float("nan")
    flat[6:9] = 0.0
    for bad in ([], [nan], [good, flat], [good[:11]], [np.full(12, float("inf"))]):
        with pytest.raises(ValueError):
            FV.check_poses(bad)
    for bad in ((), ("view", "view"), ("depth",)):
        with pytest.raises(ValueError):
            FV.check_want(bad)
    d0, lf, m = torch.zeros(1, 7, 2, 8), torch.zeros(1, 3, 2, 8), torch.ones(1)
    with pytest.raises(ValueError):  # refused before anything touches a device
        FV.warp(d0, lf, m, m, [nan])
    with pytest.raises(ValueError):
        FV.warp(d0, lf, m, m, [good], want=())
    with pytest.raises(ValueError):
        FV.warp(torch.zeros(1, 1, 2, 8), lf, m, m, [good])
    with pytest.raises(ValueError):
        FV.warp(d0, torch.zeros(1, 3, 2, 9), m, m, [good])
    with pytest.raises(ValueError):
        FV.warp(d0, lf, torch.ones(2), m, [good])
    with pytest.raises(RuntimeError):  # no CPU fallback
        FV.warp(d0, lf, m, m, [good])


def test_writer_has_its_own_folder(tmp_path):
    from fal_net_amd import dumps
    from fal_net_amd import freeview as FV
    w = FV.FreeviewWriter(str(tmp_path))
    assert os.listdir(tmp_path) == ["Freeview"]
    assert w.file(3, 7).endswith(os.path.join("Freeview", "0000000003_p07.png")) and w.file(3, 7, cover=True).endswith(os.path.join("Freeview", "0000000003_p07_cover.png"))
    assert w.summary() == {"frames": 0, "files": 0, "mean_cover": None}
    assert dumps.DUMP_KINDS == ("disp", "input", "pan", "pc", "feats") and "Freeview" not in dumps.FrameWriter.folders.values()


def test_signature():
    from fal_net_amd import _build, _lib
    sig = _lib.SIGNATURES["falnet_med_pose_fwd"]
    assert sig == [_lib._P] * 5 + [_lib._I] + [_lib._P] * 3 + [_lib._I] * 4 + [_lib._P]
    assert _lib.EXPECTED_VERSION == 600  # an added entry point, no changed one: falnet_version() stays
    assert "med_pose.hip" in _build.SOURCES and os.path.isfile(os.path.join(_build.CSRC, "med_pose.hip"))
    from fal_net_amd import ops
    assert "med_pose.hip" not in ops._TUNE_SOURCES  # the packaged autotune cache stays valid
