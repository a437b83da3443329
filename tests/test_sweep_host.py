"""CPU: the float64 reference of the baseline sweep (tests/_sweep_ref.py) held to account, the scaled integer margin of every listed
(case, baseline set), the --sweep command line and the binding's signature.  No GPU."""
import os

import pytest
import torch

import _head_ref as R
import _sweep_ref as S
from oracle import falnet_oracle as O

f64 = torch.float64
CASE = (2, 7, 3, 40, 30.0)


def _oracle_head(inp):
    B = inp["dlog0"].shape[0]
    return O.med_head(inp["dlog0"].to(f64), inp["left"].to(f64), inp["mn"].to(f64).view(B, 1, 1), inp["mx"].to(f64).view(B, 1, 1), True, False, True)


@pytest.mark.parametrize("case", [CASE, (2, 49, 2, 128, 300.0)])
def test_t1_is_the_oracles_right_view_and_t0_the_left_image(case):
    inp = R.make_inputs(case, "a")
    ref = S.reference(inp, (1.0, 0.0))
    head = _oracle_head(inp)
    assert float((ref["view"][:, 0] - head["p_im0"]).abs().max()) == 0.0
    assert float((ref["view"][:, 1] - inp["left"].to(f64)).abs().max()) <= 1e-15
    assert torch.equal(ref["disp"][:, 1], head["disp"])
    assert torch.equal(S.forward_disp(inp), head["disp"])


@pytest.mark.parametrize("case,set_name", [(CASE, "B"), (CASE, "C"), ((1, 128, 2, 64, 300.0), "B")])
def test_magnitude_bounds_the_reference(case, set_name):
    ref = S.reference(R.make_inputs(case, "b"), S.SETS[set_name])
    assert bool((ref["mag_view"] >= ref["view"].abs()).all())
    assert bool((ref["mag_disp"] >= ref["disp"].abs()).all()) and bool((ref["disp"] > 0).all())


def test_negative_t_reads_from_the_left():
    """One bright image column at x = 20, equal logits except one dominant plane whose shift is 3.9 (W - 1) / W pixels: at t = +1 the column
    appears LEFT of 20 (pixel x reads x + s), at t = -1 RIGHT of it."""
    B, N, H, W = 1, 4, 1, 40
    inp = {"dlog0": torch.zeros(B, N, H, W), "left": torch.zeros(B, 3, H, W), "mn": torch.tensor([2.0]), "mx": torch.tensor([3.9])}
    inp["dlog0"][:, N - 1] = 50.0  # plane N - 1: d = mx
    inp["left"][:, :, :, 20] = 1.0
    ref = S.reference(inp, (1.0, -1.0), check_margin=False)
    s = float(inp["mx"][0]) * (W - 1) / W  # 3.8025 (of the stored float32 3.9): taps x + 3 and x + 4
    right, other = ref["view"][0, 0, 0, 0], ref["view"][0, 1, 0, 0]
    assert right[16] > 0.5 and right[17] > 0.1 and float(right[18:].abs().max()) < 1e-12 and float(right[:16].abs().max()) < 1e-12
    assert other[24] > 0.5 and other[23] > 0.1 and float(other[:23].abs().max()) < 1e-12 and float(other[25:].abs().max()) < 1e-12
    assert abs(float(right[16]) - (s - 3)) < 1e-9 and abs(float(other[24]) - (s - 3)) < 1e-9


def test_scaled_margin_of_every_listed_case():
    for case, sets in S.CASES.items():
        inp = R.make_inputs(case, "a")
        for name in sets:
            S.assert_sweep_margin(inp["mn"], inp["mx"], case[1], case[3], S.SETS[name])
    inp = R.make_inputs((1, 7, 1, 2100, 300.0), "a")  # ... and why this pair is not listed
    assert S.sweep_margin(inp["mn"], inp["mx"], 7, 2100, S.SETS["B"]) < S.MARGIN
    with pytest.raises(AssertionError):
        S.assert_sweep_margin(inp["mn"], inp["mx"], 7, 2100, S.SETS["B"])
    # the issue's cases and sets are all there
    want = {(1, 2, 2, 40, 30.0): "ABCZ", (2, 7, 3, 40, 30.0): "ABCZ", (1, 9, 2, 77, 120.0): "ABCZ", (2, 49, 2, 128, 300.0): "ABCZ",
            (1, 128, 2, 64, 300.0): "ABZ", (1, 49, 2, 1242, 300.0): "ABZ", (1, 96, 1, 1280, 300.0): "ABCZ", (1, 7, 1, 2100, 300.0): "ACZ"}
    for case, sets in want.items():
        assert set(sets) <= set(S.CASES[case]), case
    assert S.SETS == {"A": (1.0,), "B": (-1.0, -0.5, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0), "C": (0.37, -1.63, 1.9), "Z": (0.0,)}
    assert set(S.families(CASE)) == set("abcd") and set(S.families((1, 2, 2, 40, 30.0))) == set("abcd") and S.families((1, 9, 2, 77, 120.0)) == ("a", "b")


def test_coefficients_follow_the_rule():
    """Measured, a power of two, and the t = 1 view takes the head's own p_im0 coefficient."""
    import math
    for out in ("view", "disp"):
        for cls in ("d30", "wide"):
            c = S.COEF[out][cls]
            assert c is not None and math.log2(c) == round(math.log2(c)), (out, cls, c)
    assert S.coef("view", CASE, 1.0) == R.COEF["p_im0"]["d30"] and S.coef("view", (1, 9, 2, 77, 120.0), 1.0) == R.COEF["p_im0"]["wide"]
    assert S.coef("view", CASE, 0.5) == S.COEF["view"]["d30"]


def test_command_line():
    import Test_KITTI as T
    a = T.parser.parse_args(["--sweep", "5", "--sweep-range", "-0.5", "1.5"])
    assert a.sweep == 5 and a.sweep_range == [-0.5, 1.5]
    assert T.sweep_fractions(a) == [-0.5, 0.0, 0.5, 1.0, 1.5]
    a = T.parser.parse_args(["--sweep", "5"])
    assert T.sweep_fractions(a) == [-1.0, -0.5, 0.0, 0.5, 1.0]
    assert T.sweep_fractions(T.parser.parse_args(["--sweep", "1", "--sweep-range", "0.25", "1"])) == [0.25]
    a = T.parser.parse_args([])
    assert a.sweep is None and T.sweep_fractions(a) is None
    with pytest.raises(SystemExit):
        T.parser.parse_args(["--sweep", "0"])
    with pytest.raises(SystemExit):
        T.parser.parse_args(["--dump", "disp,depth"])
    with pytest.raises(SystemExit):  # the -save* switches stay refused
        T.refuse_out_of_scope(T.parser.parse_args(["-save", "True", "--sweep", "3"]))


def test_wrapper_checks_need_no_device():
    from fal_net_amd import views as V
    assert V.check_baselines((0.5, -2.0, 2)) == [0.5, -2.0, 2.0]
    for bad in ((3.0,), (float("nan"),), (float("inf"),), (), (0.1, -2.5)):
        with pytest.raises(ValueError):
            V.check_baselines(bad)
    d0, lf, m = torch.zeros(1, 7, 2, 8), torch.zeros(1, 3, 2, 8), torch.ones(1)
    with pytest.raises(ValueError):  # refused before anything touches a device
        V.sweep(d0, lf, m, m, (3.0,))
    with pytest.raises(ValueError):
        V.sweep(torch.zeros(1, 1, 2, 8), lf, m, m, (1.0,))
    with pytest.raises(RuntimeError):  # no CPU fallback
        V.sweep(d0, lf, m, m, (1.0,))


def test_sweep_writer_has_its_own_folders(tmp_path):
    from fal_net_amd import dumps
    w = dumps.SweepWriter(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["Sweep", "r_disp"]
    assert w.file("sweep", 3, 7).endswith(os.path.join("Sweep", "0000000003_v07.png")) and w.file("r_disp", 3).endswith(os.path.join("r_disp", "0000000003.png"))
    assert dumps.DUMP_KINDS == ("disp", "input", "pan", "pc", "feats")
    assert dumps.FrameWriter.folders == {"disp": "l_disp", "input": "Input im", "pan": "Pan", "pc": "Point_cloud", "feats": "feats"}


def test_signature():
    from fal_net_amd import _lib
    sig = _lib.SIGNATURES["falnet_med_sweep_fwd"]
    assert len(sig) == 13
    assert sig == [_lib._P] * 5 + [_lib._I] + [_lib._P] * 2 + [_lib._I] * 4 + [_lib._P]
    assert _lib.EXPECTED_VERSION == 600  # an added entry point, no changed one: falnet_version() stays
    from fal_net_amd import _build
    assert "med_sweep.hip" in _build.SOURCES
