"""CPU: the host side of the cloud metrics -- the definition (tests/_cloud_ref.py) against a float64 brute force and on hand-written cases, the
means and ratios of fal_net_amd/cloud_metrics.py on rows the definition makes, the refusals that need no device and the command line.  No GPU."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import _cloud_ref as CR
from fal_net_amd import cloud_metrics as CM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "fal_net_amd", "libfalnet_hip.so")


def cloud(n, seed, extent=(40.0, 10.0, 2.0)):
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 4)) * np.array([*extent, 1.0]) - np.array([0.0, extent[1] / 2, extent[2] / 2, 0.0])).astype(np.float32)
    return pts


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------------
def test_reference_against_float64_brute_force():
    """With |coordinates| <= M = 40 every difference is at most 2 M and carries half an ulp (2^-24 relative); a square then carries 2 (2^-24) + 2^-24,
    and each of the two additions 2^-24 more of a partial sum that is at most d2: the f32 chain is within 6 2^-24 d2 + (the absolute part of the
    differences' roundings, 2^-24 times the coordinates' magnitude, through 2 |d| per axis) of the exact value.  Bound used: 8 2^-24 (d2 + M sqrt(d2))
    -- loose by design; it only has to show that the chain computes the squared distance."""
    q, r = cloud(700, 0), cloud(900, 1)
    d2, idx = CR.nearest_ref(q, r)
    best, j, second = CR.nearest_f64(q, r)
    assert d2.dtype == np.float32 and idx.dtype == np.int32
    tol = 8 * 2.0 ** -24 * (best + 40.0 * np.sqrt(best))
    assert (np.abs(d2.astype(np.float64) - best) <= tol).all()
    # the index is the brute force's wherever best and second best are further apart than both roundings
    clear = second - best > 2 * 8 * 2.0 ** -24 * (second + 40.0 * np.sqrt(second))
    assert clear.sum() > 600 and (idx[clear] == j[clear]).all()
    # and everywhere the index names a reference at the stated distance
    dd = q[:, :3] - r[idx][:, :3]
    assert np.array_equal(((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).view(np.uint32), d2.view(np.uint32))
    # chunking does not enter
    d2b, idxb = CR.nearest_ref(q, r, chunk=37)
    assert np.array_equal(d2b.view(np.uint32), d2.view(np.uint32)) and np.array_equal(idxb, idx)


def test_hand_written_cases():
    nan, inf = np.float32("nan"), np.float32("inf")
    r = np.array([[1, 0, 0, 9], [0, 1, 0, 9], [1, 0, 0, 7], [0, 0, 2, 9], [nan, 0, 0, 9], [inf, 0, 0, 0]], np.float32)
    q = np.array([[0, 0, 0, 5],      # ties between references 0, 1 (d2 = 1) and 2: the smallest index
                  [1, 0, 0, 5],      # a duplicated reference: index 0, not 2
                  [0, 0, 3, 5],      # reference 3
                  [nan, 0, 0, 5],    # a NaN query: no pair takes part
                  [inf, 0, 0, 5],    # inf - inf with reference 5 is NaN, every other pair is +inf and takes part: +inf at index 0
                  [0, 0, 1e30, 5]],  # an overflow to +inf is a value like any other: the first reference whose pair is not NaN
                 np.float32)
    d2, idx = CR.nearest_ref(q, r)
    assert idx.tolist() == [0, 0, 3, -1, 0, 0]
    assert d2[:3].tolist() == [1.0, 0.0, 1.0] and np.isposinf(d2[3:]).all()
    # the fourth column is ignored
    assert np.array_equal(CR.nearest_ref(q[:, :3], r[:, :3])[1], idx)
    # only a NaN pair is left: nothing takes part
    d2, idx = CR.nearest_ref(q[4:5], r[5:6])
    assert np.isposinf(d2[0]) and idx[0] == -1
    # nr = 0 and nq = 0
    d2, idx = CR.nearest_ref(q, r[:0])
    assert np.isposinf(d2).all() and (idx == -1).all() and len(d2) == 6
    d2, idx = CR.nearest_ref(q[:0], r)
    assert d2.shape == (0,) and idx.shape == (0,)


def test_cloud_errors_ref_and_the_host_arithmetic():
    # lattice distances: d2 in {0, 1, 4, 9, inf, nan}; a threshold met exactly (tau = 2: d2 = 4 counts)
    d_p = np.array([0, 1, 4, 9, np.inf, np.nan, 4], np.float32)
    d_g = np.array([1, 1, 9], np.float32)
    row = CR.cloud_errors_ref(d_p, d_g, (1.0, 2.0, 2.5))
    assert row[[CR.N_PRED, CR.SUM_PRED, CR.SUMSQ_PRED, CR.N_GT, CR.SUM_GT, CR.SUMSQ_GT]].tolist() == [5, 8, 18, 3, 5, 11]
    assert row[CR.HIT_PRED:CR.HIT_PRED + 8].tolist() == [2, 4, 4, 0, 0, 0, 0, 0] and row[CR.HIT_GT:CR.HIT_GT + 8].tolist() == [2, 2, 2, 0, 0, 0, 0, 0]
    assert CM.ROW == CR.ROW == 22 and CM.COL == {"n_pred": 0, "sum_pred": 1, "sumsq_pred": 2, "n_gt": 3, "sum_gt": 4, "sumsq_gt": 5, "hit_pred": 6, "hit_gt": 14}
    empty = CR.cloud_errors_ref(d_p, d_g[:0], (1.0, 2.0, 2.5))
    res = CM.summarize(np.stack([row, empty, np.full(CR.ROW, np.nan)]), (1.0, 2.0, 2.5))
    assert res["frames"] == 1 and res["counted"].tolist() == [True, False, False]
    want = CR.derived(row, (1.0, 2.0, 2.5))
    assert CR.derived(empty, (1.0, 2.0, 2.5)) is None
    assert want["accuracy"] == 8 / 5 and want["completeness"] == 5 / 3 and want["chamfer_l2"] == 18 / 5 + 11 / 3
    for k in ("accuracy", "completeness", "chamfer", "chamfer_l2"):
        assert res[k][0] == want[k] == res[k + "_mean"] and np.isnan(res[k][2])
        assert np.isnan(res[k][1]) == (k != "accuracy")  # the empty direction's means are NaN, and what is formed from them; the other's are not
    assert res["accuracy"][1] == 8 / 5 and np.isnan(res["recall"][1]).all() and res["precision"][1].tolist() == want["precision"]
    for k in ("precision", "recall", "f"):
        assert res[k][0].tolist() == want[k] == res[k + "_mean"]
    assert want["precision"] == [2 / 5, 4 / 5, 4 / 5] and want["recall"] == [2 / 3, 2 / 3, 2 / 3]
    # no counted frame: NaN means; P = R = 0: F = 0, not 0 / 0
    none = CM.summarize(np.stack([empty]), (1.0,))
    assert none["frames"] == 0 and np.isnan(none["chamfer_mean"]) and np.isnan(none["f_mean"]).all()
    far = CM.summarize(CR.cloud_errors_ref(np.array([9], np.float32), np.array([9], np.float32), (1.0,))[None], (1.0,))
    assert far["f"][0].tolist() == [0.0] and far["chamfer"][0] == 6.0
    b = CR.sum_bounds(row)
    assert b[CR.SUM_PRED] == 10 * 2.0 ** -53 * 8 and b[CR.SUMSQ_GT] == 5 * 2.0 ** -53 * 11


# ---- the module without a device ------------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_kernel_source():
    from fal_net_amd import _build
    src = open(os.path.join(_build.CSRC, "nearest.hip")).read()
    define = lambda name: re.search(r"#define " + name + r" (.+?)\s*(//.*)?$", src, re.M).group(1)  # noqa: E731
    assert define("NN_BLOCK") == "(NN_THREADS * NN_QPT)" and int(define("NN_THREADS")) * int(define("NN_QPT")) == CM.QUERY_BLOCK
    assert int(define("NN_TILE")) == CM.REF_TILE and int(define("NN_TARGET_WGS")) == CM.TARGET_WORKGROUPS and int(define("NN_MAX_SPLITS")) == CM.MAX_SPLITS
    hdr = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    assert int(re.search(r"#define FALNET_CLOUD_ROW (\d+)", hdr).group(1)) == CM.ROW
    assert int(re.search(r"#define FALNET_CLOUD_MAX_THRESHOLDS (\d+)", hdr).group(1)) == CM.MAX_THRESHOLDS
    for name, col in (("N_PRED", "n_pred"), ("SUM_PRED", "sum_pred"), ("SUMSQ_PRED", "sumsq_pred"), ("N_GT", "n_gt"), ("SUM_GT", "sum_gt"),
                      ("SUMSQ_GT", "sumsq_gt"), ("HIT_PRED", "hit_pred"), ("HIT_GT", "hit_gt")):
        assert int(re.search(r"#define FALNET_CLOUD_" + name + r" (\d+)", hdr).group(1)) == CM.COL[col]
    assert CM.THRESHOLDS == (0.1, 0.25, 0.5, 1.0) and CM.CloudMetrics.key == "cloud"
    B, T = CM.QUERY_BLOCK, CM.REF_TILE
    assert CM.default_splits(0, 5) == CM.default_splits(5, 0) == 1 and CM.default_splits(1, 1) == 1 and CM.default_splits(1, T) == 1
    assert CM.default_splits(B + 1, 2 * T + 3) == 3 and CM.default_splits(1, T + 1) == 2
    assert CM.default_splits(75000, 75000) == -(-CM.TARGET_WORKGROUPS // 74) and CM.default_splits(1, 1 << 30) == CM.TARGET_WORKGROUPS <= CM.MAX_SPLITS


def test_entry_points_in_header_binding_and_build():
    from fal_net_amd import _build, _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "falnet_hip.h")).read(), flags=re.S)
    for name in ("falnet_nearest", "falnet_nearest_splits", "falnet_nearest_workspace_bytes", "falnet_cloud_errors", "falnet_cloud_errors_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["falnet_nearest"] == [_lib._P, _lib._L, _lib._P, _lib._L, _lib._I, _lib._P, _lib._P, _lib._P, _lib._P]
    assert _lib._RESTYPES["falnet_nearest_workspace_bytes"] is _lib.C.c_int64 and _lib._RESTYPES["falnet_cloud_errors_workspace_bytes"] is _lib.C.c_int64
    assert "nearest.hip" in _build.SOURCES and _build.FILE_FLAGS["nearest.hip"] == ["-ffp-contract=off"] and "nearest.hip" not in ops._TUNE_SOURCES
    src = open(os.path.join(_build.CSRC, "nearest.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert '#include "ordered.h"' in src and "wave_sum_f64(" in code and "atomicMin" in code
    assert len(re.findall(r"atomic\w*\s*\(", code)) == 1 and "cooperative" not in code and "fmaf" not in code  # one integer minimum, nothing else


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_sizes_and_refusals_without_a_device():
    """The size functions and every argument check run before anything touches the device."""
    from fal_net_amd import _lib as L
    lib = L.lib()
    B, T = CM.QUERY_BLOCK, CM.REF_TILE
    for nq, nr in ((0, 0), (1, 1), (1, T), (1, T + 1), (B + 1, 2 * T + 3), (75000, 75000), (16000, 90000), (1, (1 << 31) - 1), (3 * B, 5)):
        assert lib.falnet_nearest_splits(nq, nr) == CM.default_splits(nq, nr), (nq, nr)
    assert lib.falnet_nearest_splits(-1, 5) == 0 and lib.falnet_nearest_splits(5, 1 << 31) == 0
    assert lib.falnet_nearest_workspace_bytes(100, 100, 1) == 0 and lib.falnet_nearest_workspace_bytes(100, 100, 3) == 800
    assert lib.falnet_nearest_workspace_bytes(100, 100, 0) == 0 and lib.falnet_nearest_workspace_bytes(100, 5 * T, 0) == 800
    for bad in ((-1, 1, 1), (1, 1 << 31, 1), (1, 1, -1), (1, 1, 1025)):
        assert lib.falnet_nearest_workspace_bytes(*bad) == 0, bad
    assert lib.falnet_cloud_errors_workspace_bytes() == 2 * 64 * 11 * 8
    fake, odd = L.C.c_void_p(1 << 20), L.C.c_void_p((1 << 20) + 4)
    base = dict(q=fake, nq=5, r=fake, nr=7, s=0, d2=fake, idx=fake, ws=fake)
    for tag, change, word in (("nq < 0", dict(nq=-1), "2\\^31"), ("nr = 2^31", dict(nr=1 << 31), "2\\^31"), ("splits -1", dict(s=-1), "splits"),
                              ("splits 1025", dict(s=1025), "splits"), ("null query", dict(q=None), "null"), ("null d2", dict(d2=None), "null"),
                              ("null idx", dict(idx=None), "null"), ("null ref", dict(r=None), "null ref"), ("misaligned query", dict(q=odd), "16-byte"),
                              ("misaligned ref", dict(r=odd), "16-byte"), ("misaligned d2", dict(d2=L.C.c_void_p((1 << 20) + 2)), "4-byte"),
                              ("no workspace", dict(s=2, ws=None), "workspace"), ("misaligned workspace", dict(s=2, ws=odd), "workspace")):
        k = dict(base, **change)
        assert lib.falnet_nearest(k["q"], k["nq"], k["r"], k["nr"], k["s"], k["d2"], k["idx"], k["ws"], None) != 0, tag
        assert re.search(word, lib.falnet_last_error().decode()), (tag, lib.falnet_last_error().decode())
    assert lib.falnet_nearest(None, 0, fake, 7, 0, None, None, None, None) == 0  # nq = 0: nothing to do, nothing launched
    tau = (L.C.c_double * 8)(*[0.01 * (i + 1) for i in range(8)])
    base = dict(a=fake, na=5, b=fake, nb=7, tau=tau, K=4, row=fake, ws=fake)
    bad_tau, nan_tau = (L.C.c_double * 8)(0.1, -1.0), (L.C.c_double * 8)(float("nan"))
    for tag, change, word in (("9 thresholds", dict(K=9), "thresholds"), ("K < 0", dict(K=-1), "thresholds"), ("null thresholds", dict(tau=None), "null"),
                              ("null d2", dict(a=None), "null d2"), ("null row", dict(row=None), "null row"), ("null workspace", dict(ws=None), "null row"),
                              ("misaligned row", dict(row=odd), "8-byte"), ("n < 0", dict(na=-1), "2\\^31"), ("negative tau2", dict(tau=bad_tau), "tau2"),
                              ("NaN tau2", dict(tau=nan_tau, K=1), "tau2")):
        k = dict(base, **change)
        assert lib.falnet_cloud_errors(k["a"], k["na"], k["b"], k["nb"], k["tau"], k["K"], k["row"], k["ws"], None) != 0, tag
        assert re.search(word, lib.falnet_last_error().decode()), (tag, lib.falnet_last_error().decode())


def test_python_checks_without_a_device():
    pts = torch.zeros(5, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CM.nearest(pts, pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CM.nearest(np.zeros((5, 4), np.float32), pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CM.cloud_errors(pts, pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CM.CloudTable(1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CM.CloudMetrics(1, lambda i, H, W: (None, 1.0), device="cpu")
    assert CM.check_thresholds([0.5, 1]) == (0.5, 1.0) and CM.check_thresholds(()) == () and CM.check_thresholds([0.0]) == (0.0,)
    for bad in ([1.0, 0.5], [0.5, 0.5], [-1.0], [float("nan")], [float("inf")], list(range(1, 10))):
        with pytest.raises(ValueError):
            CM.check_thresholds(bad)
    for bad in (dict(on="pred"), dict(calibration=None), dict(beams=-1), dict(beams=200), dict(max_depth=0.0), dict(max_depth=float("inf")),
                dict(thresholds=[2.0, 1.0])):
        with pytest.raises(ValueError):
            CM.CloudMetrics(**dict(dict(n_frames=1, calibration=lambda i, H, W: (None, 1.0), device="cpu"), **bad))
    assert CM.target_fb("eigen", 80) is None and CM.target_fb("kitti2015", 1242) == 721.5377 * 0.54
    with pytest.raises(ValueError):
        CM.target_fb("make3d", 1242)
    assert "Nobody has tuned" in open(CM.__file__).read()  # the default thresholds say what they are

    class F:  # a frame without ground truth is passed over before anything is touched
        target = None
    CM.CloudMetrics.frame(object.__new__(CM.CloudMetrics), F())


# ---- command line -------------------------------------------------------------------------------------------------------------------------------------
def test_parser_refusals_and_what_settings_hide(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    T = importlib.import_module("Test_KITTI")
    parse = T.parser.parse_args
    a = parse([])
    assert a.cloud_metrics is False and a.cm_thresholds is None and a.cm_on == "gt" and a.cm_beams == 0 and a.cm_max_depth == 80.0
    assert T.CLOUD_ARGS == ("cloud_metrics", "cm_thresholds", "cm_on", "cm_beams", "cm_max_depth") and set(T.CLOUD_ARGS) <= set(vars(a))
    T.check_cloud_args(a, True), T.check_cloud_args(a, False), T.check_family_args(a)
    on = parse(["--cloud-metrics", "--cm-thresholds", "0.2,0.4", "--cm-on", "all", "--cm-beams", "64", "--cm-max-depth", "60"])
    assert (on.cloud_metrics, on.cm_thresholds, on.cm_on, on.cm_beams, on.cm_max_depth) == (True, [0.2, 0.4], "all", 64, 60.0)
    T.check_family_args(on), T.check_cloud_args(on, True)
    with pytest.raises(SystemExit, match="no ground truth"):
        T.check_cloud_args(on, False)  # synthetic mode
    with pytest.raises(SystemExit, match="-eval True"):
        T.check_cloud_args(parse(["--cloud-metrics", "-eval", "False"]), True)
    # the parameters are refused without the switch
    for alone in (["--cm-thresholds", "0.5"], ["--cm-on", "all"], ["--cm-beams", "8"], ["--cm-max-depth", "60"]):
        with pytest.raises(SystemExit) as e:
            T.check_family_args(parse(alone))
        assert str(e.value) == "{} set(s) a parameter of --cloud-metrics: add --cloud-metrics".format(alone[0])
        T.check_family_args(parse(["--cloud-metrics"] + alone))
    for bad in (["--cm-thresholds", "1,0.5"], ["--cm-thresholds", "-1"], ["--cm-thresholds", "x"], ["--cm-thresholds", "1,2,3,4,5,6,7,8,9"],
                ["--cm-on", "pred"], ["--cm-beams", "129"], ["--cm-beams", "-1"], ["--cm-max-depth", "0"], ["--cm-max-depth", "inf"]):
        with pytest.raises(SystemExit):
            parse(["--cloud-metrics"] + bad)
    # the pinned tables are untouched, the new family has a table of its own with the same four-tuples
    assert [f[0] for f in T.FAMILIES] == ["--sweep", "--stats", "--pseudo-lidar", "--mesh", "--sparsification", "--freeview", "--freeview-fill"]
    assert [(f[0], f[1], f[3]) for f in T.LATER_FAMILIES] == [("--min-component", T.COMPONENT_ARGS, True)]
    assert [(f[0], f[1], f[3]) for f in T.NEWER_FAMILIES] == [("--cloud-metrics", T.CLOUD_ARGS, True)] and all(len(f) == 4 and callable(f[2]) for f in T.NEWER_FAMILIES)
    assert T.LINE_ORDER == ("view", "sparsification", "pseudo_lidar", "mesh", "sweep", "freeview", "stats", "components") and T.LATER_LINE_ORDER == ("cloud",)
    # hidden_settings and settings_hidden are what they were: they do not know the new names, with or without the switch
    off = parse(["--mesh"])
    on = parse(["--mesh", "--cloud-metrics"])
    assert not set(T.CLOUD_ARGS) & set(T.settings_hidden(off)) and T.settings_hidden(off) == T.settings_hidden(on) and T.hidden_settings(off) == T.hidden_settings(on)
    assert T.settings_left_out(off) == T.settings_hidden(off) + T.CLOUD_ARGS and T.settings_left_out(on) == T.settings_hidden(on)
    # settings.txt: the names of a run without the switch are the names it had before the switch existed
    names = lambda a: [k for k in vars(a) if k not in T.settings_left_out(a)]  # noqa: E731
    before = [k for k in vars(off) if k not in T.settings_hidden(off) and k not in T.CLOUD_ARGS]
    assert names(off) == before and set(names(on)) - set(names(off)) == set(T.CLOUD_ARGS)
    src = open(os.path.join(ROOT, "Test_KITTI.py")).read()
    assert src[src.index("def main():"):].count("CloudMetrics") == 1 and src.count("CloudMetrics") == 1 and "settings_left_out(args)" in src


def test_cloud_errors_txt_and_the_json_line(tmp_path, monkeypatch, capsys):
    monkeypatch.syspath_prepend(ROOT)
    T = importlib.import_module("Test_KITTI")
    th = (0.5, 1.0)
    rows = np.stack([CR.cloud_errors_ref(np.array([0, 1, 4], np.float32), np.array([1, 0.25], np.float32), th),
                     CR.cloud_errors_ref(np.array([1], np.float32), np.zeros(0, np.float32), th)])
    res = CM.summarize(rows, th)
    path = tmp_path / "cloud_errors.txt"
    T.write_cloud_errors(str(path), res)
    lines = path.read_text().splitlines()
    assert "over 1 frames" in lines[0] and lines[1].split()[:7] == ["frame", "n_pred", "n_gt", "accuracy", "completeness", "chamfer", "chamfer_l2"]
    assert lines[1].split()[7:] == ["P@0.5", "R@0.5", "F@0.5", "P@1", "R@1", "F@1"] and len(lines) == 5
    assert lines[2].split()[0] == "mean" and lines[3].split()[0] == "0" and lines[4].split()[0] == "1" and "nan" in lines[4]
    assert lines[2].split()[3:] == lines[3].split()[3:] and float(lines[3].split()[5]) == pytest.approx(1.0 + 0.75, abs=1e-6)
    assert len(lines[3].split()) == 3 + 4 + 6

    class P:
        key = "cloud"
        beside = {"file": "f"}

        def summary(self):
            return {"frames": 1}

    class Q(P):
        key = "mesh"
    T.extra_lines([P(), Q()])
    out = capsys.readouterr().out.splitlines()
    assert out == ['{"mesh": {"frames": 1}, "file": "f"}', '{"cloud": {"frames": 1}, "file": "f"}']  # after LINE_ORDER's
