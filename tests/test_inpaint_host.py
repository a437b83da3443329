"""CPU: the float64 reference of the background-biased pull-push (tests/_inpaint_ref.py) held to the properties and the bias figures of its
definition, the host side of fal_net_amd/inpaint.py and freeview.fill_views (level counts, workspace sizes, refusals before anything touches a
device), the --freeview-fill command line and the binding's signature.  No GPU."""
import os

import numpy as np
import pytest
import torch

import _inpaint_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BUILT = os.path.exists(os.path.join(ROOT, "fal_net_amd", "libfalnet_hip.so"))
SIZES = [(375, 1242), (37, 124), (65, 63), (1, 1), (1, 2), (2, 1), (3, 5), (7, 9), (64, 64), (129, 200), (75, 250), (256, 512)]


def holes(H, W, seed, kept=0.3, ones=0.2):
    rng = np.random.default_rng(seed)
    w = np.where(rng.random((H, W)) < kept, rng.random((H, W)), 0.0)
    w[rng.random((H, W)) < ones] = 1.0
    return rng, w


def test_level_counts():
    assert [R.levels(*s) for s in ((375, 1242), (37, 124), (65, 63), (1, 1))] == [11, 7, 7, 0]
    assert R.level_sizes(3, 5) == [(3, 5), (2, 3), (1, 2), (1, 1)]
    assert R.workspace_floats(4, 3, 5, 2) == 2 * 6 * (6 + 2 + 1)


def test_constant_image_comes_back_constant():
    """To 3e-16 without a bias, the definition's own figure.  With a bias the last level alone rounds more often on the way to a filled pixel
    (F G, two passes of two products and a sum each for up(F G) and for up(G), the quotient, the final product and sum): at most 8 roundings
    of 2^-53 each on a value below 1; the levels above enter through convex combinations and add nothing to first order."""
    for H, W in ((37, 124), (65, 63), (7, 9)):
        for beta in (0.0, 4.0, 8.0):
            for seed in (1, 2, 3):
                rng, w = holes(H, W, seed)
                guide = rng.random((H, W)) * 80.0
                err = np.abs(R.fill(np.full((2, H, W), 0.7) * w, w, guide, 80.0, beta) - 0.7).max()
                assert err <= (3e-16 if beta == 0.0 else 8 * 2.0 ** -53), (H, W, beta, seed, err)


def test_full_weight_pixels_come_back_bit_for_bit_and_the_range_holds():
    H, W = 37, 124
    rng, w = holes(H, W, 2)
    colour = rng.uniform(-1.0, 1.0, (3, H, W))
    guide = rng.random((H, W)) * 100.0
    for beta in (0.0, 4.0):
        out = R.fill(colour * w, w, guide, 100.0, beta)
        assert np.array_equal(out[:, w == 1.0], colour[:, w == 1.0])
        kept = colour[:, w >= R.FLOOR]
        assert out.min() >= kept.min() - 1e-15 and out.max() <= kept.max() + 1e-15
        assert np.isfinite(out).all()


def test_one_kept_pixel_floods_and_nothing_gives_zero():
    H, W = 33, 70
    w = np.zeros((H, W))
    w[20, 11] = 0.625
    colour = np.array([0.25, -0.5])[:, None, None] * np.ones((2, H, W))
    out = R.fill(colour * w, w, np.full((H, W), 30.0), 60.0, 4.0)
    assert np.abs(out - colour).max() <= 1e-15
    assert not R.fill(np.full((2, H, W), np.nan), np.zeros((H, W)), np.full((H, W), np.nan), 60.0, 4.0).any()
    one = R.fill(np.array([[[0.3]]]), np.array([[0.5]]))  # 1 x 1: L = 0, out = c0 + (1 - w0) F_0
    assert one.shape == (1, 1, 1) and abs(one[0, 0, 0] - (0.3 + 0.5 * 0.6)) <= 1e-16


def test_beta_zero_is_the_plain_pull_push():
    for H, W in ((37, 124), (65, 63), (1, 2)):
        rng, w = holes(H, W, 3)
        v = rng.uniform(-1.0, 1.0, (3, H, W)) * w
        nan_guide = np.full((H, W), np.nan)
        assert np.array_equal(R.fill(v, w, nan_guide, 1.0, 0.0), R.plain_fill(v, w))  # exactly; and the guide is never read


def test_dropped_pixels_do_not_leak():
    H, W = 20, 31
    rng, w = holes(H, W, 4)
    w[w < 0.1] = np.float32(R.FLOOR) * 0.5  # below the floor, not zero
    v = rng.random((1, H, W)) * w
    keep = w >= R.FLOOR
    guide = rng.random((H, W))
    clean = R.fill(np.where(keep, v, 0.0), np.where(keep, w, 0.0), guide, 1.0, 2.0)
    dirty = R.fill(np.where(keep, v, np.nan), w, np.where(keep, guide, np.nan), 1.0, 2.0)
    assert 0 < keep.sum() < keep.size and np.isfinite(clean).all() and np.array_equal(dirty, clean)


BIAS = {32: (0.5000, 0.1827, 0.0388, 0.0009), 29: (0.5723, 0.2979, 0.1106, 0.0046)}


@pytest.mark.parametrize("edge", sorted(BIAS))
def test_bias_figures_of_the_step_scene(edge):
    """Mean fill inside the 16-wide hole over the edge: the definition's table to its printed digits, falling in beta; a bias in the pull alone
    does nothing on this scene."""
    v, w, guide, scale, hole = R.step_scene(edge)
    got = [float(R.fill(v, w, guide, scale, beta)[0][hole].mean()) for beta in (0.0, 2.0, 4.0, 8.0)]
    assert ["%.4f" % g for g in got] == ["%.4f" % b for b in BIAS[edge]], got
    dense = [float(R.fill(v, w, guide, scale, beta)[0][hole].mean()) for beta in np.linspace(0.0, 8.0, 17)]
    assert all(b < a for a, b in zip(dense, dense[1:])), dense
    pull_only = [float(R.fill(v, w, guide, scale, beta, bias_in_push=False)[0][hole].mean()) for beta in (0.0, 2.0, 4.0, 8.0)]
    assert ["%.4f" % g for g in pull_only] == ["%.4f" % BIAS[edge][0]] * 4, pull_only


def test_the_bound_is_the_derived_one():
    assert R.K == 17 + 28 + 20 and R.U32 == 2.0 ** -24
    assert R.bound(375, 1242, 2.0) == R.K * 12 * 2.0 ** -24 * 2.0
    inp = R.inputs(7, 9, 3, 2, "floor", 0)
    f = np.float32(R.FLOOR)
    assert set(np.unique(inp["weight"])) <= {np.float32(0), np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(1)), np.float32(1)}
    assert (inp["guide"] <= inp["guide_scale"][:, None, None, None]).all() and (inp["guide"] >= 0).all()  # the precondition of the g term of K
    ref, M = R.reference(inp, 4.0)
    assert ref.shape == (2, 3, 7, 9) and all(0.99 < m < 1.01 for m in M)
    assert R.magnitude(np.zeros((1, 2, 2)), np.zeros((2, 2))) == 0.0


@pytest.mark.skipif(not BUILT, reason="library not built")
def test_levels_and_workspace_agree_with_the_reference():
    from fal_net_amd import _lib as L
    from fal_net_amd import inpaint as IP
    for H, W in SIZES:
        assert IP.levels(H, W) == R.levels(H, W), (H, W)
        for C, images in ((1, 1), (3, 2), (4, 8)):
            assert IP.workspace_bytes(C, H, W, images) == 4 * R.workspace_floats(C, H, W, images), (C, H, W, images)
            assert 4 * images * (C + 2) * IP._pyramid_cells(H, W) == IP.workspace_bytes(C, H, W, images)
    lib = L.lib()
    assert lib.falnet_inpaint_levels(0, 5) == -1 and lib.falnet_inpaint_levels(1 << 16, 1 << 15) == -1
    assert lib.falnet_inpaint_workspace_bytes(5, 4, 4, 1) == -1 and lib.falnet_inpaint_workspace_bytes(1, 4, 4, 0) == -1
    assert lib.falnet_replay_op_index(b"falnet_inpaint_fwd") == -1
    for bad in ((0, 4, 4, 1), (5, 4, 4, 1), (1, 0, 4, 1), (1, 4, 4, 0), (1, 1 << 16, 1 << 15, 1)):
        with pytest.raises(ValueError):
            IP.workspace_bytes(*bad)
    with pytest.raises(ValueError):
        IP.levels(3, 0)


def test_wrapper_checks_need_no_device():
    from fal_net_amd import inpaint as IP
    v, w, g = torch.zeros(2, 3, 4, 6), torch.ones(2, 1, 4, 6), torch.zeros(2, 1, 4, 6)
    bad = [
        dict(values=torch.zeros(2, 5, 4, 6), weight=w),                      # C = 5
        dict(values=torch.zeros(4, 6), weight=torch.ones(4, 6)),             # no channel dimension
        dict(values=torch.zeros(2, 3, 0, 6), weight=torch.ones(2, 1, 0, 6)),  # H = 0
        dict(values=torch.zeros(0, 3, 4, 6), weight=torch.ones(0, 1, 4, 6)),  # no image
        dict(values=v, weight=torch.ones(2, 1, 4, 5)),
        dict(values=v, weight=torch.ones(1, 4, 6)),
        dict(values=v, weight=w, beta=-1.0),
        dict(values=v, weight=w, beta=8.5),
        dict(values=v, weight=w, beta=float("nan")),
        dict(values=v, weight=w, beta=float("inf")),
        dict(values=v, weight=w, floor=0.0),
        dict(values=v, weight=w, floor=1.5),
        dict(values=v, weight=w, floor=float("nan")),
        dict(values=v, weight=w, beta=2.0),                                  # no guide
        dict(values=v, weight=w, beta=2.0, guide=g),                         # no scale
        dict(values=v, weight=w, beta=2.0, guide_scale=3.0),
        dict(values=v, weight=w, beta=2.0, guide=g[:1], guide_scale=3.0),
        dict(values=v, weight=w, beta=2.0, guide=g, guide_scale=0.0),
        dict(values=v, weight=w, beta=2.0, guide=g, guide_scale=[1.0, -2.0]),
        dict(values=v, weight=w, beta=2.0, guide=g, guide_scale=[1.0, 2.0, 3.0]),
        dict(values=v, weight=w, beta=2.0, guide=g, guide_scale=torch.ones(3)),
        dict(values=v, weight=w, workspace=torch.zeros(10)),                 # too small
        dict(values=v, weight=w, workspace=torch.zeros(4096, dtype=torch.float64)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):  # refused before anything touches a device
            IP.fill(**kw)
    with pytest.raises(RuntimeError):  # no CPU fallback
        IP.fill(v, w)
    with pytest.raises(RuntimeError):
        IP.fill(v, w[:, 0], guide=g[:, 0], guide_scale=[2.0, 3.0], beta=4.0, workspace=torch.zeros(4096))


def test_fill_views_checks_need_no_device():
    from fal_net_amd import freeview as FV
    out = {"view": torch.zeros(1, 2, 3, 4, 6), "disp": torch.zeros(1, 2, 1, 4, 6), "cover": torch.ones(1, 2, 1, 4, 6)}
    mx = torch.ones(1)
    for kw in (dict(out={k: out[k] for k in ("view", "cover")}, max_disp=mx), dict(out=out, max_disp=torch.ones(2)), dict(out=out, max_disp=mx, beta=9.0),
               dict(out=out, max_disp=mx, floor=0.0), dict(out=dict(out, disp=torch.zeros(1, 2, 1, 4, 5)), max_disp=mx)):
        with pytest.raises(ValueError):
            FV.fill_views(**kw)
    with pytest.raises(RuntimeError):
        FV.fill_views(out, mx)
    assert FV.FILL_BETA == 4.0 and "not a tuned value" in FV.fill_views.__doc__


def test_writer_keeps_its_summary_until_filled_frames_are_written(tmp_path):
    from fal_net_amd import freeview as FV
    w = FV.FreeviewWriter(str(tmp_path))
    assert w.summary() == {"frames": 0, "files": 0, "mean_cover": None}
    assert callable(w.write_filled)


def test_command_line():
    import Test_KITTI as T
    a = T.parser.parse_args([])
    assert a.freeview_fill is None
    T.check_freeview_fill_args(a)
    a = T.parser.parse_args(["--freeview", "2", "--freeview-fill"])
    assert a.freeview_fill == 4.0
    T.check_freeview_fill_args(a)
    a = T.parser.parse_args(["--freeview-fill", "2.5", "--freeview", "2", "--synthetic"])
    assert a.freeview_fill == 2.5 and a.freeview == 2
    T.check_freeview_fill_args(a)
    T.check_freeview_fill_args(T.parser.parse_args(["--freeview", "1", "--freeview-fill", "0"]))
    with pytest.raises(SystemExit):
        T.parser.parse_args(["--freeview", "2", "--freeview-fill", "much"])
    for bad in (["--freeview-fill"], ["--freeview-fill", "3"], ["--freeview", "2", "--freeview-fill", "8.5"], ["--freeview", "2", "--freeview-fill", "-1"],
                ["--freeview", "2", "--freeview-fill", "nan"]):
        with pytest.raises(SystemExit):  # stops at the command line
            T.check_freeview_fill_args(T.parser.parse_args(bad))
    with pytest.raises(SystemExit):  # the -save* switches stay refused
        T.refuse_out_of_scope(T.parser.parse_args(["-save", "True", "--freeview", "3", "--freeview-fill"]))


def test_settings_hide_the_argument_when_unused():
    """The filter Test_KITTI.py applies to settings.txt, on parsed arguments: no line for the switch without it, one with it."""
    import Test_KITTI as T
    assert T.FREEVIEW_FILL_ARGS == ("freeview_fill",) and "freeview_fill" not in T.FREEVIEW_ARGS
    off, on = T.parser.parse_args(["--freeview", "2"]), T.parser.parse_args(["--freeview", "2", "--freeview-fill"])
    assert set(T.FREEVIEW_FILL_ARGS) <= set(T.hidden_settings(off)) and not set(T.FREEVIEW_FILL_ARGS) & set(T.hidden_settings(on))
    assert not set(T.FREEVIEW_ARGS) & set(T.hidden_settings(off)) and set(T.FREEVIEW_ARGS) <= set(T.hidden_settings(T.parser.parse_args([])))
    assert set(vars(on)) - set(T.FREEVIEW_FILL_ARGS) == set(vars(off)) - set(T.FREEVIEW_FILL_ARGS)


def test_signature():
    from fal_net_amd import _build, _lib, ops
    P, I, F, L64 = _lib._P, _lib._I, _lib._F, _lib._L
    assert _lib.SIGNATURES["falnet_inpaint_fwd"] == [P, P, P, P, F, F, P, P, L64, I, I, I, I, P]
    assert _lib.SIGNATURES["falnet_inpaint_levels"] == [I, I] and _lib.SIGNATURES["falnet_inpaint_workspace_bytes"] == [I, I, I, I]
    assert _lib._RESTYPES["falnet_inpaint_workspace_bytes"] is _lib.C.c_int64
    assert _lib.EXPECTED_VERSION == 600  # added entry points, no changed one: falnet_version() stays
    assert "inpaint.hip" in _build.SOURCES and os.path.isfile(os.path.join(_build.CSRC, "inpaint.hip"))
    assert "inpaint.hip" not in ops._TUNE_SOURCES  # the packaged autotune cache stays valid
    header = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    for name in ("falnet_inpaint_levels", "falnet_inpaint_workspace_bytes", "falnet_inpaint_fwd"):
        assert name + "(" in header, name
