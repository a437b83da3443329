"""GPU: the sparsification curves (fal_net_amd/sparsification.py: curves, csrc/sparsify.hip) against their numpy definition
(tests/_sparsify_ref.py).  n and every d1 value compare with == (integer counts and one division); abs_rel and rms stay within the DERIVED bound
|got - ref| <= (n_j + 2) 2^-53 |ref|: any-order summation of n_j non-negative terms against the exactly rounded fsum, plus the division and the
square root -- no measured coefficient.  The order inside the call is pinned where S = n: every cut removes exactly one more pixel.  Every row
sits in a NaN-filled buffer with a guard region behind it."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _sparsify_ref as SR  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import metrics as M  # noqa: E402
from fal_net_amd import myUtils as utils  # noqa: E402
from fal_net_amd import sparsification as SP  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GUARD = 64


@pytest.fixture(autouse=True)
def small_widths(monkeypatch):
    """The camera tables of myUtils know KITTI widths only; the small frames take the 1242-pixel camera scaled to their width -- on both sides,
    which read the same dictionaries."""
    for w in (7, 124, 1025):
        monkeypatch.setitem(utils.width_to_focal, w, 721.5377 * w / 1242)
        monkeypatch.setitem(utils.width_to_baseline, w, 0.9982 * 0.54)


def fb_of(mode, W):
    if W in utils.width_to_focal:
        return M.focal_baseline(mode, W)
    return 721 * 0.22 if mode == "make3d" else 721.5377 * W / 1242 * (0.54 if mode == "kitti2015" else 0.9982 * 0.54)


@functools.lru_cache(maxsize=None)
def frame(mode, H, W, valid, seed=0):
    """Prediction: a disparity map; ground truth: pred * (1 + noise) in the unit the mode reads, a fraction `valid` of it non-zero.  Four score
    maps: a noisy copy of the relative error, a constant, a map with NaN, +-0 and +-inf in it, and a confidence (larger is better, sign -1)."""
    rng = np.random.default_rng(seed)
    fb = fb_of(mode, W)
    pred = (rng.random((H, W)) ** 2 * 0.07 * W + 0.5).astype(np.float32)
    noise = 0.15 * rng.standard_normal((H, W))
    noisy = np.maximum(pred.astype(np.float64) * (1 + noise), 0.05)
    gt = (noisy if mode == "kitti2015" else fb / noisy).astype(np.float32)
    gt[rng.random((H, W)) >= valid] = 0
    noisy_err = (np.abs(noise) + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
    special = rng.standard_normal((H, W)).astype(np.float32)
    flat = special.reshape(-1)
    flat[rng.choice(H * W, max(H * W // 6, 5), replace=False)] = np.resize(np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], np.float32), max(H * W // 6, 5))
    conf = (1 / (1 + 8 * np.abs(noise)) + 0.05 * rng.random((H, W))).astype(np.float32)
    scores = (("noisy", noisy_err, 1), ("const", np.full((H, W), 0.25, np.float32), 1), ("special", special, 1), ("conf", conf, -1))
    for a in (pred, gt, noisy_err, special, conf):
        a.setflags(write=False)
    return pred, gt, scores


def one_pixel(mode, H, W):
    pred, gt, scores = frame(mode, H, W, 0.3)
    g1 = np.zeros_like(gt)
    g1[H - 100 if H > 219 else H // 2, 600 if W > 1180 else W // 2] = np.float32(17.5)
    return pred, g1, scores


@functools.lru_cache(maxsize=None)
def reference(mode, H, W, valid, which, use_median, steps, kind="seeded"):
    pred, gt, scores = frame(mode, H, W, valid) if kind == "seeded" else one_pixel(mode, H, W)
    if kind == "empty":
        gt = np.zeros_like(gt)
    return SR.sparsify_ref(mode, pred, gt, [(m, s) for k, m, s in scores if k in which], use_median=use_median, steps=steps)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached frames are read-only


def guarded_table(names, steps):
    """A one-row table whose row is the head of a NaN-filled buffer with GUARD doubles behind it -> (table, buffer)."""
    t = SP.SparsificationTable(1, names, steps, DEV)
    buf = torch.full((t.width + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    t.table = buf[:t.width].view(1, t.width)
    return t, buf


def run(mode, pred, gt, scores, which, use_median, steps):
    t, buf = guarded_table(list(which), steps)
    sc = {k: (dev(m), s) for k, m, s in scores if k in which}
    row = SP.curves(dev(pred), dev(gt), mode, sc, use_median=use_median, steps=steps, out=t.row(0))
    torch.cuda.synchronize()
    assert row.data_ptr() == buf.data_ptr() and bool(torch.isnan(buf[t.width:]).all()), "written behind the row"
    return row.cpu().numpy(), t


def compare(got, want, n_scores, steps, tag):
    """n and d1 exactly; abs_rel and rms within the derived bound.  Prints the worst figure before it asserts."""
    assert got.shape == want.shape == (SP.row_length(n_scores, steps),), tag
    n = int(want[0])
    _, gs, go = SR.split(got, n_scores, steps)
    _, ws, wo = SR.split(want, n_scores, steps)
    g = np.concatenate([gs.reshape(-1, 3, steps), go[None]])  # (n_scores + 1, 3, S)
    w = np.concatenate([ws.reshape(-1, 3, steps), wo[None]])
    if n == 0:
        print(f"{tag}: n 0, every curve NaN: {bool(np.isnan(got[1:]).all())}")
        assert got[0] == 0 and np.isnan(got[1:]).all(), tag
        return
    bound = SR.curve_bound(n, steps, w[:, :2])
    err = np.abs(g[:, :2] - w[:, :2])
    worst = float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))))
    d1_wrong = int((g[:, 2] != w[:, 2]).sum())
    print(f"{tag}: n {int(got[0])} (reference {n}), d1 values that differ {d1_wrong}, worst abs_rel / rms error {worst:.3f} of the bound")
    assert got[0] == n, tag
    assert d1_wrong == 0, tag
    assert (err <= bound).all(), tag


ALL = ("noisy", "const", "special", "conf")
CASES = {  # mode, H, W, valid fraction, scores, median, steps
    "13x7-kitti2015-dense": ("kitti2015", 13, 7, 1.0, ALL, False, 50),
    "13x7-kitti2015-dense-S=n": ("kitti2015", 13, 7, 1.0, ALL, False, 91),  # every cut removes one more pixel: the curves pin the whole order
    "13x7-kitti2015-half-median": ("kitti2015", 13, 7, 0.5, ALL, True, 50),  # n < S: cuts repeat
    "37x124-kitti2015-sparse-median": ("kitti2015", 37, 124, 0.05, ALL, True, 50),
    "37x124-kitti2015-dense-oracles-only": ("kitti2015", 37, 124, 1.0, (), False, 50),  # 4588 pixels: three tiles, the last one partial
    "37x124-make3d": ("make3d", 37, 124, 0.6, ("noisy", "conf"), True, 50),
    "37x124-make3d-steps-100": ("make3d", 37, 124, 0.02, ALL, True, 100),  # about 90 pixels: S = 100 > n
    "375x1242-eigen-sparse": ("eigen", 375, 1242, 0.05, ALL, False, 50),
    "375x1242-eigen-dense-median": ("eigen", 375, 1242, 1.0, ("special",), True, 20),
    "375x1242-kitti2015-sparse-median": ("kitti2015", 375, 1242, 0.05, ALL, True, 50),
    "375x1242-kitti2015-third": ("kitti2015", 375, 1242, 0.3, ("noisy", "conf"), False, 50),
    # 525 825 pixels: 257 tiles, one more than the offset scan takes at a time -- the last tile's pixels are numbered from the carried base
    "513x1025-kitti2015-half": ("kitti2015", 513, 1025, 0.5, ("noisy", "conf"), False, 50),
}


@pytest.mark.parametrize("case", list(CASES))
def test_curves_equal_the_definition(case):
    mode, H, W, valid, which, use_median, steps = CASES[case]
    pred, gt, scores = frame(mode, H, W, valid)
    want = reference(mode, H, W, valid, which, use_median, steps)
    if "S=n" in case:
        assert int(want[0]) == steps == H * W
    got, _ = run(mode, pred, gt, scores, which, use_median, steps)
    compare(got, want, len(which), steps, case)
    if which == ALL and int(want[0]) > 200:  # the scores do what they were made to do: the informative ones beat the constant one
        ause = SR.areas(got, 4, steps)[0]
        assert ause[0, 0] < ause[1, 0] and ause[3, 0] < ause[1, 0]


def test_a_constant_score_keeps_pixel_number_order_on_the_device():
    """S = n with a constant score: cut j keeps the pixels j .. n - 1 of the region's row-major numbering."""
    mode, H, W = "kitti2015", 13, 7
    pred, gt, scores = frame(mode, H, W, 1.0)
    got, _ = run(mode, pred, gt, scores, ("const",), False, 91)
    g, p, idx = SR.pairs(mode, pred, gt)
    e_abs = SR.errors(g, p)[0]
    want = np.array([np.sum(e_abs[j:]) / (91 - j) for j in range(91)])
    assert idx.tolist() == list(range(91)) and np.allclose(SR.split(got, 1, 91)[1][0, 0], want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("mode,H,W", [("kitti2015", 37, 124), ("eigen", 375, 1242), ("make3d", 37, 124)])
def test_no_valid_pixel_and_a_single_one(mode, H, W):
    pred, gt, scores = frame(mode, H, W, 0.3)
    for use_median in (False, True) if mode != "make3d" else (True,):
        got, _ = run(mode, pred, np.zeros_like(gt), scores, ALL, use_median, 50)
        compare(got, reference(mode, H, W, 0.3, ALL, use_median, 50, "empty"), 4, 50, f"{mode} no valid pixel, median={use_median}")
        _, g1, _ = one_pixel(mode, H, W)
        got, _ = run(mode, pred, g1, scores, ALL, use_median, 50)
        want = reference(mode, H, W, 0.3, ALL, use_median, 50, "one")
        compare(got, want, 4, 50, f"{mode} one valid pixel, median={use_median}")
        assert want[0] == 1 and all(len(set(c)) == 1 for c in got[1:].reshape(-1, 50))  # every cut keeps that pixel


def test_two_calls_give_bit_identical_rows_and_a_table_collects_them():
    mode, H, W, valid, which, use_median, steps = CASES["375x1242-kitti2015-sparse-median"]
    pred, gt, scores = frame(mode, H, W, valid)
    a, _ = run(mode, pred, gt, scores, which, use_median, steps)
    b, _ = run(mode, pred, gt, scores, which, use_median, steps)
    assert a.tobytes() == b.tobytes()
    # a table of one row that grows: rows 0 and 2 written (two frame sizes, one workspace), row 1 left NaN
    t = SP.SparsificationTable(1, list(which), steps, DEV)
    sc = {k: (dev(m), s) for k, m, s in scores}
    SP.curves(dev(pred), dev(gt), mode, sc, use_median=use_median, steps=steps, out=t.row(0))
    small = frame("kitti2015", 37, 124, 0.05)
    SP.curves(dev(small[0]), dev(small[1]), "kitti2015", {k: (dev(m), s) for k, m, s in small[2]}, use_median=True, steps=steps, out=t.row(2))
    res = t.result()
    assert res["rows"].shape == (3, SP.row_length(4, steps)) and res["rows"][0].tobytes() == a.tobytes() and np.isnan(res["rows"][1]).all()
    assert res["frames"] == 2 and res["names"] == list(which)
    want = [SR.areas(r, 4, steps) for r in (a, reference("kitti2015", 37, 124, 0.05, ALL, True, 50))]
    for i, k in enumerate(which):
        for j, m in enumerate(SP.METRICS):
            assert abs(res["ause_mean"][k][m] - (want[0][0][i, j] + want[1][0][i, j]) / 2) <= 1e-12, (k, m)
            assert abs(res["aurg_mean"][k][m] - (want[0][1][i, j] + want[1][1][i, j]) / 2) <= 1e-12, (k, m)
    with pytest.raises(ValueError, match="doubles"):
        SP.curves(dev(pred), dev(gt), mode, {"noisy": sc["noisy"]}, out=t.row(0))  # one score into rows made for four


def test_every_refusal_returns_nonzero_and_writes_nothing():
    lib = L.lib()
    H, W = 37, 124
    pred, gt, scores = frame("kitti2015", H, W, 0.3)
    p_t, g_t, m_t = dev(pred), dev(gt), dev(scores[0][1])
    row = torch.full((SP.row_length(1, 50) + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.full((int(lib.falnet_sparsify_workspace_bytes(H, W, 4)) // 8,), -1, dtype=torch.int64, device=DEV)

    def sc(n=1, sign=1, null=False):
        s = L.Scores()
        s.n = n
        for i in range(max(min(n, 4), 0)):
            s.map[i], s.sign[i] = (None if null else m_t.data_ptr()), sign
        return s

    base = dict(pred=L.ptr(p_t), gt=L.ptr(g_t), H=H, W=W, mode=0, fb=100.0, scale=None, min_d=1.0, max_d=80.0, scores=sc(), steps=50, row=L.ptr(row), ws=L.ptr(ws))
    odd = L.C.c_void_p(row.data_ptr() + 4)
    cases = [("null pred", dict(pred=None), "null map"), ("null gt", dict(gt=None), "null map"), ("mode 3", dict(mode=3), "mode"), ("mode -1", dict(mode=-1), "mode"),
             ("H = 0", dict(H=0), "pixels"), ("W < 0", dict(W=-4), "pixels"), ("H W > 2^24", dict(H=4097, W=4096), r"2\^24"), ("fb = 0", dict(fb=0.0), "focal"),
             ("steps 1", dict(steps=1), "steps"), ("steps 101", dict(steps=101), "steps"), ("5 scores", dict(scores=sc(5)), "scores"),
             ("-1 scores", dict(scores=sc(-1)), "scores"), ("sign 0", dict(scores=sc(2, 0)), "sign"), ("sign -2", dict(scores=sc(1, -2)), "sign"),
             ("null score map", dict(scores=sc(2, 1, True)), "null map"), ("null row", dict(row=None), "null row"), ("null workspace", dict(ws=None), "workspace"),
             ("misaligned row", dict(row=odd), "8-byte"), ("min_d = 0", dict(min_d=0.0), "min_d"), ("max_d < min_d", dict(max_d=0.5), "min_d"),
             ("make3d without scale", dict(mode=2), "median-scaled"), ("eigen on a small frame", dict(mode=1), "Eigen crop")]
    for tag, change, word in cases:
        k = dict(base, **change)
        rc = lib.falnet_sparsify(k["pred"], k["gt"], k["H"], k["W"], k["mode"], k["fb"], k["scale"], k["min_d"], k["max_d"], k["scores"], k["steps"], k["row"],
                                 k["ws"], L.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0, tag
        with pytest.raises(RuntimeError, match=word):
            L.check(rc, "sparsify")
        assert bool(torch.isnan(row).all()) and bool((ws == -1).all()), tag  # nothing ran
    k = base
    assert lib.falnet_sparsify(k["pred"], k["gt"], H, W, 0, fb_of("kitti2015", W), None, 1.0, 80.0, k["scores"], 50, k["row"], k["ws"], L.stream_ptr()) == 0
    torch.cuda.synchronize()
    compare(row[:SP.row_length(1, 50)].cpu().numpy(), reference("kitti2015", H, W, 0.3, ("noisy",), False, 50), 1, 50, "the next valid call")
    assert bool(torch.isnan(row[SP.row_length(1, 50):]).all())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SP.curves(p_t.cpu(), g_t, "kitti2015", {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SP.curves(p_t, g_t, "kitti2015", {"x": (m_t.cpu(), 1)})
    for bad in (dict(scores={"x": (m_t, 0)}), dict(scores={"x": (m_t[:5], 1)}), dict(scores={str(i): (m_t, 1) for i in range(5)}), dict(steps=1), dict(steps=101)):
        with pytest.raises(ValueError):
            SP.curves(p_t, g_t, "kitti2015", **dict(dict(scores={}), **bad))
    with pytest.raises(ValueError):
        SP.curves(p_t, g_t[:5], "kitti2015", {})
    with pytest.raises(TypeError):
        SP.curves(p_t, g_t, "kitti2015", {}, out=row)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------
def _write_kitti2015(tmp_path, n_val=1, size=(375, 1242)):
    """<root>/Kitti2015/training/{image_2,image_3,disp_occ_0}: generated KITTI-2015-shaped pairs, as tests/test_gpu_metrics.py builds them."""
    from PIL import Image
    rng = np.random.default_rng(7)
    root = tmp_path / "data"
    for i in range(n_val):
        for sub in ("image_2", "image_3"):
            d = root / "Kitti2015" / "training" / sub
            d.mkdir(parents=True, exist_ok=True)
            Image.fromarray(rng.integers(0, 256, (*size, 3), dtype=np.uint8)).save(d / f"{i:06d}_10.png")
        d = root / "Kitti2015" / "training" / "disp_occ_0"
        d.mkdir(parents=True, exist_ok=True)
        disp = (rng.random(size) * 80 * 256).astype(np.uint16)
        disp[rng.random(size) < 0.8] = 0  # sparse ground truth
        Image.fromarray(disp).save(d / f"{i:06d}_10.png")
    return root


def _child(script, argv, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, cwd=ROOT, env=dict(os.environ, FALNET_DETERMINISTIC="1"), capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


@pytest.mark.parametrize("extra", [[], ["--device-metrics", "-median", "True"]], ids=["host-metrics", "device-metrics-median"])
def test_cli_end_to_end(tmp_path, extra):
    root = _write_kitti2015(tmp_path)
    argv = ["-d", str(root), "-tn", "Kitti2015", "--allow-seeded-weights", "-w", "0", "-mspp", "False"] + extra
    out = _child(os.path.join("tests", "_sparsify_cli.py"), [str(tmp_path / "rec")] + argv + ["--save-path", str(tmp_path / "sp"), "--sparsification", "std,conf",
                                                                                            "--sparsification-steps", "25"])
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and list(lines[0]) == ["sparsification"], out
    s = lines[0]["sparsification"]
    rec = np.load(tmp_path / "rec" / "frame_0.npz")
    assert s["scores"] == ["std", "conf"] == rec["names"].tolist() and s["steps"] == 25 == int(rec["steps"]) and s["frames"] == 1
    assert rec["signs"].tolist() == [1, -1] and str(rec["mode"]) == "kitti2015" and bool(rec["use_median"]) == bool(extra)
    want = SR.sparsify_ref("kitti2015", rec["disp"], rec["gt"], list(zip(rec["maps"], rec["signs"].tolist())), use_median=bool(extra), steps=25)
    ause, aurg = SR.areas(want, 2, 25)
    # the bound of a curve value, carried through the trapezoid: dx times the sum of the bounds of the S differences (each difference carries
    # the bounds of its two values), plus the roundings of the S additions themselves
    n = int(want[0])
    _, sc, orc = SR.split(want, 2, 25)
    b_sc, b_or = SR.curve_bound(n, 25, sc), SR.curve_bound(n, 25, orc)
    b_sc[:, 2], b_or[2] = 0, 0  # d1 is exact
    for i, k in enumerate(("std", "conf")):
        for j, m in enumerate(SP.METRICS):
            tol_ause = (b_sc[i, j] + b_or[j]).sum() / 25 + 30 * 2.0 ** -53 * np.abs(sc[i, j]).max()
            tol_aurg = (b_sc[i, j] + b_sc[i, j, :1]).sum() / 25 + 30 * 2.0 ** -53 * np.abs(sc[i, j]).max()
            print(f"{k} {m}: ause {s['ause'][k][m]!r} (reference {ause[i, j]!r}, tolerance {tol_ause:.2e}), aurg {s['aurg'][k][m]!r} (reference {aurg[i, j]!r})")
            assert abs(s["ause"][k][m] - ause[i, j]) <= tol_ause and abs(s["aurg"][k][m] - aurg[i, j]) <= tol_aurg, (k, m)
    txt = open(tmp_path / "sp" / "sparsification.txt").read().splitlines()
    assert s["file"].endswith("sparsification.txt") and "1 frames, 25 cuts" in txt[0] and txt[1].split(":")[0].strip() == "std" and txt[2].split(":")[0].strip() == "conf"
    assert "ause_rms {:.6f}".format(s["ause"]["std"]["rms"]) in txt[1] and len(txt) == 5 + 9
    # the same command without the switch: no file, no extra line, the same errors.txt, and a settings.txt without the two names
    out = _child("Test_KITTI.py", argv + ["--save-path", str(tmp_path / "plain")])
    assert len([ln for ln in out.splitlines() if ln.startswith("{")]) == 1 and not os.path.exists(tmp_path / "plain" / "sparsification.txt")
    assert open(tmp_path / "plain" / "errors.txt").read() == open(tmp_path / "sp" / "errors.txt").read()
    with_sp = dict(ln.split(":", 1) for ln in open(tmp_path / "sp" / "settings.txt").read().splitlines())
    plain = dict(ln.split(":", 1) for ln in open(tmp_path / "plain" / "settings.txt").read().splitlines())
    assert {k.strip() for k in with_sp} - {k.strip() for k in plain} == {"sparsification", "sparsification_steps"}
    assert all(plain[k] == with_sp[k] for k in plain if k.strip() != "save_path")
