"""CPU: the host side of the sparsification curves -- properties of the definition (tests/_sparsify_ref.py), the AUSE / AURG arithmetic of
fal_net_amd/sparsification.py on rows the definition makes, the refusals that need no device and the command line.  No GPU."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import _sparsify_ref as SR
from fal_net_amd import sparsification as SP

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
S = 50


def seeded_pairs(n, seed=0, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(1, 81, n).astype(np.float64), rng.integers(1, 81, n).astype(np.float64)
    g = rng.random(n) * 79 + 1
    return g, np.clip(g * (1 + 0.2 * rng.standard_normal(n)), 1.0, 80.0)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------
def test_a_score_equal_to_an_error_has_zero_ause_of_that_metric():
    g, p = seeded_pairs(5000)
    e_abs, e_sq, t = SR.errors(g, p)
    xs = [e.astype(np.float32) for e in (e_abs, e_sq, t)]
    row = SR.curves_from_pairs(g, p, xs, S)
    ause, aurg = SR.areas(row, 3, S)
    assert ause[0, 0] == 0.0 and ause[1, 1] == 0.0 and ause[2, 2] == 0.0  # the score's ordering IS the oracle's: the same curve, bit for bit
    assert (aurg[[0, 1, 2], [0, 1, 2]] > 0).all()
    # and through the module's own arithmetic on the same row
    res = SP.summarize(row[None], ["e_abs", "e_sq", "t"], S)
    assert res["frames"] == 1 and res["n"][0] == 5000
    assert res["ause_mean"]["e_abs"]["abs_rel"] == 0.0 and res["ause_mean"]["e_sq"]["rms"] == 0.0 and res["ause_mean"]["t"]["d1"] == 0.0
    got_ause = np.array([[res["ause_mean"][k][m] for m in SP.METRICS] for k in res["names"]])
    got_aurg = np.array([[res["aurg_mean"][k][m] for m in SP.METRICS] for k in res["names"]])
    assert np.allclose(got_ause, ause, rtol=0, atol=1e-15) and np.allclose(got_aurg, aurg, rtol=0, atol=1e-15)


def test_the_oracle_is_below_every_score_on_integer_depths():
    """Integer depths: e_sq and the counts are exact integers and the e_abs are ratios of small integers, which f32 keeps apart, so the oracle
    order is the true order and an exactly rounded sum of the smallest kept errors cannot exceed that of any other kept set of the same size."""
    g, p = seeded_pairs(3001, seed=1, integer=True)
    rng = np.random.default_rng(2)
    e_abs, e_sq, t = SR.errors(g, p)
    xs = [rng.random(3001).astype(np.float32), np.zeros(3001, np.float32), (e_abs + rng.standard_normal(3001) * 0.3).astype(np.float32),
          (-e_sq).astype(np.float32)]
    _, sc, orc = SR.split(SR.curves_from_pairs(g, p, xs, S), 4, S)
    assert (orc[None] <= sc).all()
    assert (orc[:, 0][None] == sc[:, :, 0]).all()  # cut 0 keeps everything: every ordering sums the same set
    assert (np.diff(orc, axis=1) <= 0).all()  # an oracle curve never rises


def test_cut_ranks_by_hand():
    assert SR.cut_ranks(1, S) == [0] * 50
    assert SR.cut_ranks(3, S) == [0] * 17 + [1] * 17 + [2] * 16
    assert SR.cut_ranks(49, S) == [0] + list(range(0, 49))
    assert SR.cut_ranks(51, S) == list(range(50))
    for n in (1, 3, 49, 51):
        assert all(n - r >= 1 for r in SR.cut_ranks(n, S))
    # n < S: cuts repeat, and so do the values of the curves
    g, p = seeded_pairs(3, seed=3)
    _, sc, orc = SR.split(SR.curves_from_pairs(g, p, [np.array([1, 2, 3], np.float32)], S), 1, S)
    for c in (sc[0, 0], orc[0]):
        assert len(set(c[:17])) == len(set(c[17:34])) == len(set(c[34:])) == 1
    one = SR.curves_from_pairs(g[:1], p[:1], [np.zeros(1, np.float32)], S)
    assert one[0] == 1 and len(set(one[1:1 + S])) == 1 and np.isfinite(one).all()
    none = SR.curves_from_pairs(g[:0], p[:0], [np.zeros(0, np.float32)], S)
    assert none[0] == 0 and np.isnan(none[1:]).all() and len(none) == SP.row_length(1, S)


def test_key_image_orders_nan_zeros_and_infinities():
    x = np.array([1.0, np.nan, -0.0, 0.0, np.inf, -np.inf, -1.0, -np.nan, 1e-45, -1e-45], np.float32)
    k = SR.key_image(x)
    assert k[1] == k[7] == 0xFFFFFFFF and k[3] == 0x80000000 and k[2] == 0x7FFFFFFF and k[4] == 0xFF800000 and k[5] == 0x007FFFFF
    assert SR.order(x).tolist() == [1, 7, 4, 0, 8, 3, 2, 9, 6, 5]  # NaN (in index order), inf, 1, denormal, +0, -0, -denormal, -1, -inf
    finite = np.random.default_rng(4).standard_normal(1000).astype(np.float32)
    assert np.array_equal(SR.order(finite), np.argsort(-finite.astype(np.float64), kind="stable"))
    assert int((~k).max()) < 0xFFFFFFFF  # the sort key of no value reaches the pad key of the device path


def test_a_constant_score_removes_in_pixel_number_order():
    assert SR.order(np.full(777, 0.25, np.float32)).tolist() == list(range(777))
    assert SR.order(np.full(5, np.nan, np.float32)).tolist() == list(range(5))


def test_pairs_number_the_counted_pixels_in_region_order():
    rng = np.random.default_rng(5)
    H, W = 375, 1242
    pred = (rng.random((H, W)) * 80 + 1).astype(np.float32)
    gt = np.zeros((H, W), np.float32)
    gt[0, 0], gt[H - 219, 44], gt[H - 219, 43], gt[H - 5, 1179], gt[H - 4, 100], gt[H - 100, 600] = 5, 6, 7, 8, 9, 10
    assert SR.pairs("eigen", pred, gt)[2].tolist() == [(H - 219) * W + 44, (H - 100) * W + 600, (H - 5) * W + 1179]
    assert SR.pairs("kitti2015", pred, gt)[2].tolist() == sorted([0, (H - 219) * W + 44, (H - 219) * W + 43, (H - 5) * W + 1179, (H - 4) * W + 100, (H - 100) * W + 600])
    g, p, idx = SR.pairs("make3d", pred, np.where(gt > 8, np.float32(75), gt))
    assert len(idx) == 4 and (g <= 70).all()  # 0 < gt < 70 only


# ---- the module's host arithmetic -------------------------------------------------------------------------------------------------------------------
def test_summarize_skips_frames_without_pixels_and_unwritten_rows():
    g, p = seeded_pairs(400, seed=6)
    x = np.random.default_rng(7).random(400).astype(np.float32)
    a = SR.curves_from_pairs(g, p, [x], 10)
    b = SR.curves_from_pairs(g[:100], p[:100], [x[:100]], 10)
    empty = SR.curves_from_pairs(g[:0], p[:0], [x[:0]], 10)
    rows = np.stack([a, empty, b, np.full_like(a, np.nan)])
    res = SP.summarize(rows, ["x"], 10)
    assert res["frames"] == 2 and res["steps"] == 10 and res["metrics"] == ["abs_rel", "rms", "d1"]
    ause = [SR.areas(r, 1, 10)[0][0] for r in (a, b)]
    aurg = [SR.areas(r, 1, 10)[1][0] for r in (a, b)]
    for j, m in enumerate(SP.METRICS):
        assert np.allclose(res["ause"]["x"][m], [ause[0][j], ause[1][j]], rtol=0, atol=1e-15)
        assert abs(res["ause_mean"]["x"][m] - (ause[0][j] + ause[1][j]) / 2) < 1e-15 and abs(res["aurg_mean"]["x"][m] - (aurg[0][j] + aurg[1][j]) / 2) < 1e-15
        assert np.allclose(res["curves_mean"]["x"][m], (SR.split(a, 1, 10)[1][0, j] + SR.split(b, 1, 10)[1][0, j]) / 2, rtol=0, atol=1e-15)
        assert np.allclose(res["oracle_mean"][m], (SR.split(a, 1, 10)[2][j] + SR.split(b, 1, 10)[2][j]) / 2, rtol=0, atol=1e-15)
    nothing = SP.summarize(np.stack([empty]), ["x"], 10)
    assert nothing["frames"] == 0 and np.isnan(nothing["ause_mean"]["x"]["rms"]) and np.isnan(nothing["oracle_mean"]["d1"]).all()
    assert SP.area(np.array([3.0, 3.0, 3.0, 3.0])) == 0.25 * (12.0 - 3.0) and SP.row_length(4, 50) == 751


def test_names_steps_and_the_statistics_a_score_needs():
    assert SP.SCORES == {"std": 1, "entropy": 1, "conf": -1, "relstd": 1}
    assert SP.stats_needed(["conf"]) == ("conf",) and SP.stats_needed(["relstd", "entropy"]) == ("mean", "std", "entropy")
    st = {"std": torch.tensor([[2.0, 3.0]]), "mean": torch.tensor([[4.0, 2.0]]), "conf": torch.tensor([[0.5, 0.25]])}
    maps = SP.score_maps(st, ["relstd", "conf"])
    assert list(maps) == ["relstd", "conf"] and maps["relstd"][1] == 1 and maps["conf"][1] == -1
    assert maps["relstd"][0].dtype == torch.float32 and maps["relstd"][0].tolist() == [[0.5, 1.5]] and maps["conf"][0] is st["conf"]
    for bad in ([], ["std", "std"], ["peak"], "arg"):
        with pytest.raises(ValueError):
            SP.check_names(bad)
    for bad in (1, 101, 0):
        with pytest.raises(ValueError):
            SP.check_steps(bad)
    assert SP.check_steps(2) == 2 and SP.check_steps(100) == 100


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SP.argsort_u32(torch.zeros(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SP.curves(torch.ones(3, 4), torch.ones(3, 4), "kitti2015", {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SP.SparsificationTable(1, ["std"], device="cpu")
    with pytest.raises(ValueError):
        SP.curves(torch.ones(3, 4), torch.ones(3, 4), "stereo", {})


# ---- command line -----------------------------------------------------------------------------------------------------------------------------------
def test_parser_refusals_and_what_settings_hide(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    mod = importlib.import_module("Test_KITTI")
    a = mod.parser.parse_args([])
    assert a.sparsification is None and a.sparsification_steps is None
    mod.check_sparsification_args(a, True)
    mod.check_sparsification_args(a, False)
    assert set(mod.SPARSIFICATION_ARGS) == {"sparsification", "sparsification_steps"} <= set(vars(a))
    assert tuple(mod.SPARSIFICATION_SCORES) == tuple(SP.SCORES)
    assert set(mod.SPARSIFICATION_ARGS) <= set(mod.hidden_settings(a))  # settings.txt keeps its lines without the switch
    assert not set(mod.SPARSIFICATION_ARGS) & set(mod.hidden_settings(mod.parser.parse_args(["--sparsification", "std"])))
    a = mod.parser.parse_args(["--sparsification", "std,entropy,conf,relstd", "--sparsification-steps", "20"])
    assert a.sparsification == ["std", "entropy", "conf", "relstd"] and a.sparsification_steps == 20
    mod.check_sparsification_args(a, True)
    with pytest.raises(SystemExit, match="no ground truth"):
        mod.check_sparsification_args(a, False)  # synthetic mode
    with pytest.raises(SystemExit, match="-eval True"):
        mod.check_sparsification_args(mod.parser.parse_args(["--sparsification", "std", "-eval", "False"]), True)
    with pytest.raises(SystemExit, match="add --sparsification"):
        mod.check_family_args(mod.parser.parse_args(["--sparsification-steps", "20"]))
    for bad in (["--sparsification", "peak"], ["--sparsification", "std,std"], ["--sparsification", ""], ["--sparsification", "std", "--sparsification-steps", "1"],
                ["--sparsification", "std", "--sparsification-steps", "101"]):
        with pytest.raises(SystemExit):
            mod.parser.parse_args(bad)


def test_sparsification_txt(tmp_path, monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    mod = importlib.import_module("Test_KITTI")
    g, p = seeded_pairs(300, seed=8)
    x = np.random.default_rng(9).random(300).astype(np.float32)
    res = SP.summarize(SR.curves_from_pairs(g, p, [x, -x], 10)[None], ["std", "conf"], 10)
    path = tmp_path / "sparsification.txt"
    mod.write_sparsification(str(path), res)
    lines = path.read_text().splitlines()
    assert "1 frames, 10 cuts" in lines[0] and lines[1].split(":")[0].strip() == "std" and lines[2].split(":")[0].strip() == "conf"
    assert "ause_abs_rel {:.6f}".format(res["ause_mean"]["std"]["abs_rel"]) in lines[1] and "aurg_d1 {:.6f}".format(res["aurg_mean"]["conf"]["d1"]) in lines[2]
    assert lines[3] == "" and lines[4].startswith("Mean curves")
    curve_lines = lines[5:]
    assert len(curve_lines) == 9 and all(len(ln.split(":")[1].split()) == 10 for ln in curve_lines)


# ---- header, binding, build ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_in_header_binding_and_build():
    from fal_net_amd import _build, _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "falnet_hip.h")).read(), flags=re.S)
    for name in ("falnet_sort_u32", "falnet_sort_u32_workspace_bytes", "falnet_sparsify", "falnet_sparsify_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["falnet_sort_u32"] == [_lib._P, _lib._L, _lib._I, _lib._P, _lib._P, _lib._P]
    assert _lib.SIGNATURES["falnet_sparsify"][9] is _lib.Scores and len(_lib.SIGNATURES["falnet_sparsify"]) == 14
    assert [f[0] for f in _lib.Scores._fields_] == ["map", "sign", "n"] and _lib.C.sizeof(_lib.Scores) == 56
    assert _lib._RESTYPES["falnet_sort_u32_workspace_bytes"] is _lib.C.c_int64 and _lib._RESTYPES["falnet_sparsify_workspace_bytes"] is _lib.C.c_int64
    assert "sort.hip" in _build.SOURCES and "sparsify.hip" in _build.SOURCES
    assert _build.FILE_FLAGS["sparsify.hip"] == ["-ffp-contract=off"] and "sort.hip" not in _build.FILE_FLAGS
    assert "sort.hip" not in ops._TUNE_SOURCES and "sparsify.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600
    sort_src = open(os.path.join(_build.CSRC, "sort.hip")).read()
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", sort_src))  # no floating point in the sort
    # the depth chain is written once, in depth_pair.h, and every file that includes it is compiled without contraction
    text = {f: open(os.path.join(_build.CSRC, f)).read() for f in sorted(os.listdir(_build.CSRC)) if f.endswith((".hip", ".h", ".cpp"))}
    users = [f for f in _build.SOURCES if '#include "depth_pair.h"' in text[f]]
    assert "sparsify.hip" in users and "metrics.hip" in users
    assert [f for f in text if "struct DepthArgs" in text[f]] == ["depth_pair.h"]
    assert all(_build.FILE_FLAGS.get(f) == ["-ffp-contract=off"] for f in users), users
    assert "ordered.h" not in ops._TUNE_SOURCES and "depth_pair.h" not in ops._TUNE_SOURCES


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "fal_net_amd", "libfalnet_hip.so")), reason="library not built")
def test_workspace_bytes_and_refusals_without_a_device():
    """The size functions and every argument check run before anything touches the device."""
    from fal_net_amd import _lib as L
    lib = L.lib()
    tiles = lambda n: (n + 2047) // 2048  # noqa: E731
    assert lib.falnet_sort_u32_workspace_bytes(1, 1) == 2 * 8 + 256 * 4
    assert lib.falnet_sort_u32_workspace_bytes(465750, 7) == 2 * 7 * 465750 * 8 + 7 * 256 * tiles(465750) * 4
    assert lib.falnet_sort_u32_workspace_bytes(1 << 24, 8) == 2 * 8 * (1 << 24) * 8 + 8 * 256 * 8192 * 4
    for bad in ((0, 1), (-1, 1), ((1 << 24) + 1, 1), (5, 0), (5, 9)):
        assert lib.falnet_sort_u32_workspace_bytes(*bad) == 0, bad
    fake, odd = L.C.c_void_p(1 << 20), L.C.c_void_p((1 << 20) + 4)
    for tag, args, word in (("n > 2^24", (fake, (1 << 24) + 1, 1, fake, fake), "2\\^24"), ("n < 0", (fake, -1, 1, fake, fake), "2\\^24"),
                            ("0 segments", (fake, 5, 0, fake, fake), "segments"), ("9 segments", (fake, 5, 9, fake, fake), "segments"),
                            ("null keys", (None, 5, 1, fake, fake), "null"), ("null perm", (fake, 5, 1, None, fake), "null"),
                            ("null workspace", (fake, 5, 1, fake, None), "null"), ("misaligned perm", (fake, 5, 1, odd, fake), "8-byte"),
                            ("misaligned workspace", (fake, 5, 1, fake, odd), "8-byte")):
        assert lib.falnet_sort_u32(*args, None) != 0, tag
        assert re.search(word, lib.falnet_last_error().decode()), (tag, lib.falnet_last_error().decode())
    assert lib.falnet_sort_u32(fake, 0, 3, fake, fake, None) == 0  # n = 0: nothing to do, nothing launched
    assert lib.falnet_sparsify_workspace_bytes(375, 1242, 4) > lib.falnet_sort_u32_workspace_bytes(375 * 1242, 7) > 0
    assert lib.falnet_sparsify_workspace_bytes(375, 1242, 4) % 8 == 0
    for bad in ((0, 5, 0), (5, -1, 0), (4097, 4096, 0), (5, 5, -1), (5, 5, 5)):
        assert lib.falnet_sparsify_workspace_bytes(*bad) == 0, bad
    assert lib.falnet_sparsify_workspace_bytes(4096, 4096, 4) > 0

    def scores(n=1, sign=1, null=False):
        sc = L.Scores()
        sc.n = n
        for i in range(max(min(n, 4), 0)):
            sc.map[i], sc.sign[i] = (None if null else 1 << 20), sign
        return sc

    base = dict(pred=fake, gt=fake, H=5, W=7, mode=0, fb=100.0, scale=None, min_d=1.0, max_d=80.0, scores=scores(), steps=50, row=fake, ws=fake)
    cases = [("null pred", dict(pred=None), "null map"), ("null gt", dict(gt=None), "null map"), ("mode 3", dict(mode=3), "mode"), ("H = 0", dict(H=0), "pixels"),
             ("H W > 2^24", dict(H=4097, W=4096), "2\\^24"), ("fb = 0", dict(fb=0.0), "focal"), ("steps 1", dict(steps=1), "steps"), ("steps 101", dict(steps=101), "steps"),
             ("5 scores", dict(scores=scores(5)), "scores"), ("-1 scores", dict(scores=scores(-1)), "scores"), ("sign 0", dict(scores=scores(2, 0)), "sign"),
             ("sign 2", dict(scores=scores(1, 2)), "sign"), ("null score", dict(scores=scores(3, 1, True)), "null map"), ("null row", dict(row=None), "null row"),
             ("null workspace", dict(ws=None), "null row or workspace"), ("misaligned row", dict(row=odd), "8-byte"), ("misaligned scale", dict(scale=odd), "8-byte"),
             ("min_d = 0", dict(min_d=0.0), "min_d"), ("max_d < min_d", dict(max_d=0.5), "min_d"), ("make3d without scale", dict(mode=2), "median-scaled"),
             ("eigen too small", dict(mode=1), "Eigen crop")]
    for tag, change, word in cases:
        k = dict(base, **change)
        rc = lib.falnet_sparsify(k["pred"], k["gt"], k["H"], k["W"], k["mode"], k["fb"], k["scale"], k["min_d"], k["max_d"], k["scores"], k["steps"], k["row"],
                                 k["ws"], None)
        assert rc != 0, tag
        assert re.search(word, lib.falnet_last_error().decode()), (tag, lib.falnet_last_error().decode())
