"""CPU: the float64 reference of the distribution statistics (tests/_stats_ref.py) held to account, the float32 restatement of its formulas
against every bound of every listed case, the numpy compaction reference, the command line and the binding's signatures.  No GPU."""
import numpy as np
import pytest
import torch

import _head_ref as R
import _stats_ref as S
from oracle import falnet_oracle as O

f64 = torch.float64


def _oracle_disp(inp):
    B = inp["dlog0"].shape[0]
    return O.med_head(inp["dlog0"].to(f64), inp["left"].to(f64), inp["mn"].to(f64).view(B, 1, 1), inp["mx"].to(f64).view(B, 1, 1), True, False, False)["disp"]


def _planes(inp):
    B, N = inp["dlog0"].shape[:2]
    return O.plane_disparities(inp["mn"].to(f64).view(B, 1, 1), inp["mx"].to(f64).view(B, 1, 1), N)  # (B, N)


@pytest.mark.parametrize("case,family", [(S.CASES[1], "a"), (S.CASES[3], "b"), (S.CASES[1], "e")])
def test_mean_is_the_oracles_disp(case, family):
    inp, ref = S.cached(case, family)
    assert torch.equal(ref["mean"], _oracle_disp(inp))


@pytest.mark.parametrize("case", S.SMALL)
def test_uniform_distribution(case):
    """Family c: entropy 1, the first plane wins the tie, the window holds two of the N planes (both of them at N = 2)."""
    N = case[1]
    _, ref = S.cached(case, "c")
    assert float((ref["entropy"] - 1).abs().max()) <= 1e-15
    assert float((ref["conf"] - min(2, N) / N).abs().max()) <= 1e-15
    assert float(ref["arg"].abs().max()) == 0.0


@pytest.mark.parametrize("case", S.SMALL)
def test_one_hot_distribution(case):
    """Family d (plane N // 3 is 100 above the rest): no spread, and the peak is that plane's disparity."""
    N = case[1]
    inp, ref = S.cached(case, "d")
    d = _planes(inp)[:, N // 3].view(-1, 1, 1, 1)
    assert float(ref["std"].max()) < 1e-15
    assert float((ref["peak"] - d).abs().max()) <= 1e-12
    assert torch.equal(ref["arg"], torch.full_like(ref["arg"], N // 3))


@pytest.mark.parametrize("case,family", S.listed())
def test_peak_lies_between_the_windows_planes_and_arg_is_torchs(case, family):
    inp, ref = S.cached(case, family)
    B, N = inp["dlog0"].shape[:2]
    a = ref["arg"].long()
    assert torch.equal(a, torch.argmax(inp["dlog0"], 1, keepdim=True))
    d = _planes(inp).view(B, N, 1, 1).expand(B, N, *a.shape[2:])
    lo, hi = torch.gather(d, 1, (a - 1).clamp_min(0)), torch.gather(d, 1, (a + 1).clamp_max(N - 1))
    assert bool((ref["peak"] >= lo * (1 - 1e-15)).all()) and bool((ref["peak"] <= hi * (1 + 1e-15)).all())
    assert bool((ref["conf"] > 0).all()) and bool((ref["conf"] <= 1 + 1e-15).all())
    assert bool((ref["entropy"] >= -1e-15).all()) and bool((ref["entropy"] <= 1 + 1e-15).all())
    if family == "e":  # the window is clipped on the low side (the noise moves a few arg-maxes one plane up); family b clips it at N - 1
        assert float(ref["arg"].min()) == 0.0 and float(ref["arg"].float().mean()) < 0.1
    if family == "b":
        assert float(ref["arg"].max()) == N - 1 and float(ref["arg"].float().mean()) > N - 1.1


@pytest.mark.parametrize("case,family", S.listed())
def test_float32_restatement_meets_every_bound(case, family):
    """The bounds are achievable: plain float32 torch on the CPU stays within each of them, seeds 0 - 2."""
    for seed in (0, 1, 2):
        inp = S.make_inputs(case, family, seed)
        ref = S.cached(case, family)[1] if seed == 0 else S.reference(inp)
        res = S.compare_all(case, S.f32_eval(inp), ref)
        for k, r in res.items():
            assert r["bad"] == 0, (case, family, seed, k, r)


def test_the_bounds_reject_the_moment_form_of_std():
    """E[d^2] - mean^2 in float32 loses about u mean^2 / (2 std) where the distribution is nearly one-hot (family e at N = 128: the planes beside
    the arg-max hold e^-3 of its mass; an EXACTLY one-hot pixel, family d, cancels exactly and shows nothing): over the bound."""
    case = (1, 128, 2, 64, 300.0)
    inp, ref = S.cached(case, "e")
    r = S.compare_all(case, S.f32_eval(inp, std_form="moments"), ref, kinds=("std",))["std"]
    assert r["bad"] > 0, r


def test_compaction_reference():
    rec = np.arange(12, dtype=np.float32)
    score = np.array([0.5, 0.1, np.nan, 0.9, 0.5, 0.49999, np.inf, -np.inf, np.nan, 1.0, 0.0, 0.7], dtype=np.float32)
    assert S.compact_ref(rec, score, 0.5).tolist() == [0.0, 3.0, 4.0, 6.0, 9.0, 11.0]
    assert S.compact_ref(rec, score, np.nan).size == 0
    for n in (1, 255, 257):
        for rb in (4, 15):
            r = S.make_records(n, rb)
            assert r.nbytes == n * rb
            assert len(S.compact_ref(r, S.make_scores(n, "none"), 0.5)) == 0
            assert np.array_equal(S.compact_ref(r, S.make_scores(n, "all"), 0.5), r)
            if n > 1:
                k = len(S.compact_ref(r, S.make_scores(n, "half"), 0.5))
                assert 0.25 * n < k < 0.65 * n
                assert np.isnan(S.make_scores(n, "half")).any()


def test_command_line():
    import Test_KITTI as T
    a = T.parser.parse_args([])
    assert a.stats is None and a.pc_min_conf is None and a.disparity == "mean"
    T.check_confidence_args(a)  # nothing asked, nothing refused
    a = T.parser.parse_args(["--stats", "std,entropy,arg,conf,peak", "--dump", "pc", "--pc-min-conf", "0.5", "-mspp", "False", "--disparity", "peak"])
    assert a.stats == ["std", "entropy", "arg", "conf", "peak"] and a.pc_min_conf == 0.5 and a.disparity == "peak"
    T.check_confidence_args(a)
    with pytest.raises(SystemExit):  # --pc-min-conf without --dump pc
        T.check_confidence_args(T.parser.parse_args(["--pc-min-conf", "0.5"]))
    with pytest.raises(SystemExit):
        T.check_confidence_args(T.parser.parse_args(["--pc-min-conf", "0.5", "--dump", "disp"]))
    with pytest.raises(SystemExit):  # ms_pp is on by default
        T.check_confidence_args(T.parser.parse_args(["--disparity", "peak"]))
    with pytest.raises(SystemExit):
        T.check_confidence_args(T.parser.parse_args(["--disparity", "peak", "-mspp", "False", "-fpp", "True"]))
    for bad in (["--stats", "std,variance"], ["--stats", "mean"], ["--stats", ""], ["--pc-min-conf", "0"], ["--pc-min-conf", "1.5"], ["--disparity", "mode"]):
        with pytest.raises(SystemExit):
            T.parser.parse_args(bad)
    with pytest.raises(SystemExit):  # the -save* switches stay refused
        T.refuse_out_of_scope(T.parser.parse_args(["-save_pc", "True", "--stats", "std"]))
    from fal_net_amd import dumps
    assert dumps.DUMP_KINDS == ("disp", "input", "pan", "pc", "feats")


def test_wrapper_checks_need_no_device(tmp_path):
    from fal_net_amd import confidence as C
    assert C.KINDS == S.KINDS
    assert C.which_bits(("peak", "std", "conf")) == (0b110010, ["std", "conf", "peak"])
    assert C.which_bits("arg") == (8, ["arg"])
    for bad in ((), ("std", "std"), ("variance",)):
        with pytest.raises(ValueError):
            C.which_bits(bad)
    d0, m = torch.zeros(1, 7, 2, 8), torch.ones(1)
    with pytest.raises(ValueError):  # refused before anything touches a device
        C.stats(d0, m, m, ("mode",))
    with pytest.raises(ValueError):
        C.stats(torch.zeros(1, 1, 2, 8), m, m)
    with pytest.raises(ValueError):
        C.stats(d0, torch.ones(2), m)
    with pytest.raises(RuntimeError):  # no CPU fallback
        C.stats(d0, m, m)
    with pytest.raises(RuntimeError):
        C.compact(torch.zeros(4), torch.zeros(4), 0.5)
    w = C.StatsWriter(str(tmp_path / "a"), ("arg",), pc_min_conf=0.25)
    assert w.which == ("std", "entropy", "arg", "conf") and w.file(3, "arg").endswith("0000000003_arg.png")
    assert C.StatsWriter(str(tmp_path / "b"), (), pc_min_conf=0.25).which == ("conf",)
    assert not (tmp_path / "b" / "stats").exists()
    with pytest.raises(ValueError):
        C.StatsWriter(str(tmp_path / "c"), ("mean",))


def test_signatures():
    from fal_net_amd import _build, _lib
    import ctypes
    assert _lib.SIGNATURES["falnet_med_stats_fwd"] == [_lib._P] * 3 + [ctypes.c_uint, _lib._P] + [_lib._I] * 4 + [_lib._P]
    assert _lib.SIGNATURES["falnet_compact_records"] == [_lib._P, _lib._I, _lib._P, _lib._F, _lib._L, _lib._P, _lib._P, _lib._P, _lib._P]
    assert _lib.SIGNATURES["falnet_compact_workspace_bytes"] == [_lib._L] and _lib._RESTYPES["falnet_compact_workspace_bytes"] is ctypes.c_int64
    assert _lib.EXPECTED_VERSION == 600  # added entry points, no changed one: falnet_version() stays
    assert "med_stats.hip" in _build.SOURCES and "compact.hip" in _build.SOURCES
    lib = _lib.lib()
    assert lib.falnet_replay_op_index(b"falnet_med_stats_fwd") == -1 and lib.falnet_replay_op_index(b"falnet_compact_records") == -1
    assert lib.falnet_compact_workspace_bytes(1) == 8 and lib.falnet_compact_workspace_bytes(2049) == 16 and lib.falnet_compact_workspace_bytes(0) == 0
