"""GPU: the cloud metrics (fal_net_amd/cloud_metrics.py, csrc/nearest.hip) against their definition on the host (tests/_cloud_ref.py).

nearest: every comparison is == on the bits of d2 and on idx.  Both sides do the same correctly rounded f32 operations in the same order, a minimum
has no order, and the 64-bit key (bits(d2) << 32) | r decides value and tie together, so there is no tolerance.  The shapes come from the module's
exported decomposition: B = QUERY_BLOCK queries per workgroup, T = REF_TILE references per LDS tile, and the default split rule.
cloud_errors: the counts are equal as integers; the sums lie within the derived bound of math.fsum (_cloud_ref.sum_bounds: (n + 2) 2^-53 relative for
an ordered f64 sum of n non-negative terms against a correctly rounded one, three more units for the device's square roots, held to one ulp).
FALNET_CLOUD_REPORT=<file> also writes the observed worst case there (profiles/cloud_metrics_vs_ref.txt is such a file).
The device path is never compared with itself, except where the property IS self-agreement (two runs, a permutation)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _cloud_ref as CR  # noqa: E402
import _lidar_ref as LR  # noqa: E402
import _velo_ref as VR  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import cloud_metrics as CM  # noqa: E402
from fal_net_amd import inference, metrics, velodyne  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
B, T = CM.QUERY_BLOCK, CM.REF_TILE
NQ = (1, B - 1, B, B + 1)                 # (the fifth value of the list is B + 1 again: two blocks x three tiles is (B + 1, 2 T + 3))
NR = (1, T - 1, T, T + 1, 2 * T + 3)
SPLITS = (1, 2, 3, 0)                     # plain store, the atomic path (with an empty split where nr <= T), the library's own choice
GUARD = 64
GUARD_WORD = 0x5A5AA5A5
WORST = {}  # tag -> (ratio of the bound reached, n): the figures of profiles/cloud_metrics_vs_ref.txt


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def clouds(kind):
    """Two seeded clouds of B + 1 and 2 T + 3 records, computed once and left unchanged.  'road': metres in front of a car, f32 noise in every bit;
    'lattice': integer coordinates in [0, 12)^3 -- more records than two thirds of the sites -- so every d2 is an exact small integer and ties and
    duplicates abound."""
    rng = np.random.default_rng({"road": 5, "lattice": 6}[kind])
    if kind == "road":
        make = lambda n: (rng.random((n, 4)) * np.array([60.0, 30.0, 3.0, 1.0]) - np.array([0.0, 15.0, 1.5, 0.0])).astype(np.float32)  # noqa: E731
    else:
        make = lambda n: np.concatenate([rng.integers(0, 12, (n, 3)), rng.integers(0, 100, (n, 1))], 1).astype(np.float32)  # noqa: E731
    return make(B + 1), make(2 * T + 3)


@functools.lru_cache(maxsize=None)
def reference(kind, nq, nr):
    q, r = clouds(kind)
    return CR.nearest_ref(q[:nq], r[:nr])


@functools.lru_cache(maxsize=None)
def both_directions(kind):
    """(d2 of the first cloud against the second, d2 of the second against the first) by the reference."""
    q, r = clouds(kind)
    return reference(kind, B + 1, 2 * T + 3)[0], CR.nearest_ref(r, q)[0]


def run_nearest(q, r, splits, tag):
    """nearest() into NaN / -2 pre-filled outputs with guard zones behind them and a garbage-filled workspace with one too; the guards come back
    untouched.  -> (d2, idx) on the host."""
    nq = len(q)
    d2 = torch.full((nq + GUARD,), GUARD_WORD, dtype=torch.int32, device=DEV).view(torch.float32)
    idx = torch.full((nq + GUARD,), GUARD_WORD, dtype=torch.int32, device=DEV)
    d2[:nq] = float("nan")
    idx[:nq] = -2
    ws = torch.zeros(nq + GUARD, dtype=torch.int64, device=DEV)  # all zeros is the smallest key there is: unless the library fills it, it wins
    ws[1::2] = 0x123456789
    ws[nq:] = GUARD_WORD
    got_d2, got_idx = CM.nearest(dev(q), dev(r), splits=splits, out=(d2[:nq], idx[:nq]), workspace=ws)
    assert nq == 0 or (got_d2.data_ptr() == d2.data_ptr() and got_idx.data_ptr() == idx.data_ptr())  # (an empty view has no address)
    assert bool((d2[nq:].view(torch.int32) == GUARD_WORD).all()) and bool((idx[nq:] == GUARD_WORD).all()), tag + ": written behind an output"
    assert bool((ws[nq:] == GUARD_WORD).all()), tag + ": written behind the workspace"
    return d2[:nq].cpu().numpy(), idx[:nq].cpu().numpy()


def assert_same(got, want, tag):
    d2, idx = got
    bad_d = int((d2.view(np.uint32) != want[0].view(np.uint32)).sum())
    bad_i = int((idx != want[1]).sum())
    print(f"{tag}: {len(idx)} queries, {bad_d} d2 and {bad_i} idx differ from the reference")
    assert d2.dtype == np.float32 and idx.dtype == np.int32 and bad_d == 0 and bad_i == 0, tag


# ---- 1. nearest against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr", NR)
@pytest.mark.parametrize("nq", NQ)
def test_nearest_equals_the_reference(nq, nr):
    q, r = clouds("road")
    want = reference("road", nq, nr)
    assert (want[1] >= 0).all() and np.isfinite(want[0]).all()
    for s in SPLITS:
        assert_same(run_nearest(q[:nq], r[:nr], s, f"nq={nq} nr={nr} splits={s}"), want, f"nq={nq} nr={nr} splits={s}")
    chosen = L.lib().falnet_nearest_splits(nq, nr)
    assert chosen == CM.default_splits(nq, nr) and (chosen > 1) == (nr > T)  # the library's choice takes both paths over these shapes


def test_three_column_input_is_padded():
    q, r = clouds("road")
    d2, idx = CM.nearest(dev(q[:100, :3]), dev(r[:300, :3]))
    want = CR.nearest_ref(q[:100], r[:300])
    assert_same((d2.cpu().numpy(), idx.cpu().numpy()), want, "three columns")


# ---- 2. ties ------------------------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smallest_index():
    q, r = clouds("lattice")
    r = r.copy()
    r[T + 5:T + 40] = r[3:38]            # duplicated records across a tile border ...
    r[2 * T:2 * T + 3] = r[0:3]          # ... and in the last, partial tile
    # the definition in integers, independent of the f32 chain: exact squared distances, np.argmin takes the first minimum
    d = ((q[:, None, :3].astype(np.int64) - r[None, :, :3].astype(np.int64)) ** 2).sum(-1)
    first = d.argmin(1)
    assert ((d == d.min(1)[:, None]).sum(1) > 1).mean() > 0.4  # every other query has a tie to decide
    want = (d.min(1).astype(np.float32), first.astype(np.int32))
    ref = CR.nearest_ref(q, r)
    assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[1], want[1])
    for s in SPLITS:
        assert_same(run_nearest(q, r, s, f"lattice splits={s}"), want, f"lattice splits={s}")


# ---- 3. order freedom ------------------------------------------------------------------------------------------------------------------------------------
def test_a_permutation_of_ref_and_a_second_call_change_nothing():
    q, r = clouds("road")
    want = reference("road", B + 1, 2 * T + 3)
    perm = np.random.default_rng(9).permutation(len(r))
    unique = CR.attained(q, r, want[0]) == 1
    assert unique.sum() > B // 2
    for s in (1, 3, 0):
        d2, idx = run_nearest(q, r[perm], s, f"permuted splits={s}")
        assert np.array_equal(d2.view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(perm[idx][unique], want[1][unique])  # where the minimum is unique the index maps through the permutation
        again = run_nearest(q, r[perm], s, f"permuted again splits={s}")
        assert np.array_equal(again[0].view(np.uint32), d2.view(np.uint32)) and np.array_equal(again[1], idx)


# ---- 4. non-finite records ---------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_records():
    nan, inf = np.float32("nan"), np.float32("inf")
    q, r = (a.copy() for a in clouds("road"))
    q, r = q[:B + 1], r[:T + 7]
    rng = np.random.default_rng(10)
    for a in (q, r):
        for val in (nan, inf, -inf):
            rows = rng.choice(len(a), 40, replace=False)
            a[rows, rng.integers(0, 3, 40)] = val
    r[0] = (nan, 1, 1, 1)                      # the first reference takes no part anywhere
    r[5] = (inf, 2.0, -1.0, 0)
    q[7] = r[5]                                # inf - inf: this pair is NaN, the others of the query are +inf and take part
    q[8], r[9] = (3e-20, 0, 0, 0), (1e-20, 0, 0, 0)  # a denormal d2 = 4e-40 is a value like any other
    q[:, 3], r[:, 3] = nan, inf                # the fourth value is ignored
    want = CR.nearest_ref(q, r)
    assert want[1][7] >= 0 and np.isposinf(want[0][7]) and (want[1] == -1).sum() >= 30 and 0 < want[0][8] < 1.2e-38 and want[1][8] == 9
    for s in SPLITS:
        assert_same(run_nearest(q, r, s, f"non-finite splits={s}"), want, f"non-finite splits={s}")
    # an all-NaN reference set, an empty one and no query at all
    nothing = (np.full(50, inf, np.float32), np.full(50, -1, np.int32))
    for s in SPLITS:
        assert_same(run_nearest(q[:50], np.full((T + 3, 4), nan, np.float32), s, f"all-NaN ref splits={s}"), nothing, f"all-NaN ref splits={s}")
        assert_same(run_nearest(q[:50], r[:0], s, f"nr=0 splits={s}"), nothing, f"nr=0 splits={s}")
        d2, idx = run_nearest(q[:0], r, s, f"nq=0 splits={s}")
        assert d2.shape == (0,) and idx.shape == (0,)


# ---- 5. the sums ---------------------------------------------------------------------------------------------------------------------------------------------
def check_row(got, want, thresholds, tag):
    """Counts equal as integers; sums within _cloud_ref.sum_bounds of math.fsum.  Prints each figure before it asserts."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    counts = [CR.N_PRED, CR.N_GT] + list(range(CR.HIT_PRED, CR.HIT_PRED + 8)) + list(range(CR.HIT_GT, CR.HIT_GT + 8))
    print(f"{tag}: n {got[CR.N_PRED]:.0f} / {got[CR.N_GT]:.0f} (reference {want[CR.N_PRED]:.0f} / {want[CR.N_GT]:.0f}), hits "
          f"{got[CR.HIT_PRED:CR.HIT_PRED + len(thresholds)].tolist()} {got[CR.HIT_GT:CR.HIT_GT + len(thresholds)].tolist()}")
    worst = 0.0
    for col, bound in CR.sum_bounds(want).items():
        err = abs(got[col] - want[col])
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"{tag}: column {col}: {got[col]!r} (reference {want[col]!r}), |difference| {err:.3e}, bound {bound:.3e}")
    WORST[tag] = (worst, int(want[CR.N_PRED]), int(want[CR.N_GT]))
    assert np.array_equal(got[counts], want[counts]), tag
    for col, bound in CR.sum_bounds(want).items():
        assert abs(got[col] - want[col]) <= bound, (tag, col)


def test_cloud_errors_equals_the_reference():
    for kind, th in (("road", CM.THRESHOLDS), ("lattice", (1.0, 2.0, 3.0)), ("road", ()), ("lattice", tuple(0.5 * (k + 1) for k in range(8)))):
        p, g = clouds(kind)
        d_p, d_g = both_directions(kind)
        want = CR.cloud_errors_ref(d_p, d_g, th)
        if kind == "lattice":  # tau = 1 is a threshold that distances of both directions meet exactly: (double)d2 == tau tau
            assert 1.0 in th and (d_p == 1).any() and (d_g == 1).any()
        row = CM.cloud_errors(dev(p), dev(g), thresholds=th)
        assert row.dtype == torch.float64 and tuple(row.shape) == (CM.ROW,)
        check_row(row.cpu().numpy(), want, th, f"{kind} K={len(th)}")
    # two calls give the same bits
    a, b = CM.cloud_errors(dev(p), dev(g), thresholds=th), CM.cloud_errors(dev(p), dev(g), thresholds=th)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_the_reduction_over_its_whole_grid():
    """falnet_cloud_errors on d2 arrays longer than one pass of its fixed grid (64 workgroups x 256 threads), with non-finite entries sprinkled in:
    every thread strides, and the entries left out are left out of everything."""
    rng = np.random.default_rng(11)
    n_p, n_g = 2 * 64 * 256 + 77, 64 * 256 + 1
    d_p, d_g = (rng.random(n_p) * 30).astype(np.float32) ** 2, (rng.random(n_g) * 3).astype(np.float32) ** 2
    d_p[rng.choice(n_p, 500, replace=False)] = np.float32("inf")
    d_p[rng.choice(n_p, 300, replace=False)] = np.float32("nan")
    d_g[::7] = np.float32("inf")
    d_p[:64], d_g[:64] = 4.0, 0.0  # entries that meet tau = 2 and tau = 0 exactly
    th = (0.0, 0.1, 2.0, 29.0, 31.0)
    want = CR.cloud_errors_ref(d_p, d_g, th)
    table = CM.CloudTable(2, th, DEV)
    tau2 = (L.C.c_double * 8)(*[t * t for t in th])
    tp, tg = dev(d_p), dev(d_g)
    rows = []
    for i in (0, 1):
        L.check(L.lib().falnet_cloud_errors(L.ptr(tp), n_p, L.ptr(tg), n_g, tau2, len(th), L.ptr(table.row(i).tensor), L.ptr(table.workspace), L.stream_ptr()))
        rows.append(table.row(i).tensor.cpu().numpy())
    check_row(rows[0], want, th, "whole grid")
    assert rows[0].tobytes() == rows[1].tobytes()


def test_a_cloud_against_itself_and_against_nothing():
    p, _ = clouds("road")
    table = CM.CloudTable(3, (0.0, 0.5), DEV)
    CM.cloud_errors(dev(p), dev(p), out=table.row(0))
    CM.cloud_errors(dev(p), dev(p[:0]), out=table.row(1))
    CM.cloud_errors(dev(p[:0]), dev(p), out=table.row(2))
    res = table.result()
    n = float(len(p))
    assert res["rows"][0].tolist() == [n, 0.0, 0.0, n, 0.0, 0.0] + [n, n] + [0.0] * 6 + [n, n] + [0.0] * 6
    assert res["chamfer"][0] == 0.0 and res["precision"][0].tolist() == [1.0, 1.0] and res["recall"][0].tolist() == [1.0, 1.0] and res["f"][0].tolist() == [1.0, 1.0]
    # against an empty cloud no distance is finite in either direction: the rows are written, and not counted
    assert res["rows"][1].tolist() == [0.0] * CM.ROW and res["rows"][2].tolist() == [0.0] * CM.ROW
    assert res["counted"].tolist() == [True, False, False] and res["frames"] == 1 and res["chamfer_mean"] == 0.0 and np.isnan(res["chamfer"][1:]).all()
    with pytest.raises(ValueError):
        CM.cloud_errors(dev(p), dev(p), thresholds=(1.0,), out=table.row(0))
    with pytest.raises(TypeError):
        CM.cloud_errors(dev(p), dev(p), out=table.table[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CM.cloud_errors(dev(p), torch.from_numpy(p))
    with pytest.raises(ValueError):
        CM.nearest(dev(p), dev(p).double())
    with pytest.raises(ValueError):
        CM.nearest(dev(p), dev(p), out=(torch.empty(5, device=DEV), torch.empty(5, dtype=torch.int32, device=DEV)))


# ---- 6. the product ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(mode):
    """A small frame, computed once: a road-like depth, a prediction 3 % off it with flying pixels at the depth edges left in, a sparse target.
    eigen: 24 x 80, the target is a depth.  kitti2015: 6 x 1242 (the mode's focal length is looked up by the KITTI width), the target is a disparity."""
    H, W, scale = (24, 80, 0.065) if mode == "eigen" else (6, 1242, 1.0)
    rng = np.random.default_rng(12)
    depth = LR.road_depth(4, H, W, holes=0.0)
    fb = 721.5377 * scale * 0.54
    disp = (fb / (depth.astype(np.float64) * rng.uniform(0.97, 1.03, (H, W)))).astype(np.float32)
    target = depth.copy()
    target[rng.random((H, W)) < 0.8] = 0  # a sparse scan
    if mode == "kitti2015":
        t_fb = CM.target_fb(mode, W)
        target = np.where(target > 0, t_fb / np.maximum(target, 1e-6).astype(np.float64), 0.0).astype(np.float32)
    # (the 6-row strip takes the nominal camera: its principal point lies in the strip, so the simulated scanner's elevation range sees it)
    P = VR.kitti_like_P(scale) if mode == "eigen" else velodyne.nominal_matrix(H, W, 721.5377)
    return dict(H=H, W=W, P=P, fb=fb, disp=disp, target=target)


def make_frame(s, mode, index=0, target=True, use_median=False):
    return inference.Frame(index, None, None, dev(s["disp"]).view(1, 1, s["H"], s["W"]), None, None,
                           target=dev(s["target"]).view(1, 1, s["H"], s["W"]) if target else None, mode=mode, use_median=use_median)


@pytest.mark.parametrize("mode,on,beams,median", [("eigen", "gt", 0, False), ("eigen", "all", 0, False), ("eigen", "all", 8, False),
                                                  ("kitti2015", "gt", 0, False), ("kitti2015", "all", 16, False), ("kitti2015", "gt", 0, True)])
def test_the_product_on_a_small_frame(mode, on, beams, median):
    s = scene(mode)
    th = (0.1, 0.5, 2.0)
    asked = []

    def calibration(i, H, W):
        asked.append((i, H, W))
        return s["P"], s["fb"]

    prod = CM.CloudMetrics(3, calibration, thresholds=th, on=on, beams=beams, az_bins=256, max_depth=70.0, device=DEV, beside={"file": "x"})
    prod.frame(make_frame(s, mode, index=0, target=False))  # no ground truth: passed over, nothing asked, no row
    assert asked == [] and prod.table.n == 0
    prod.frame(make_frame(s, mode, index=4, use_median=median))
    assert asked == [(4, s["H"], s["W"])] and prod.table.n == 1
    fb = s["fb"]
    if median:  # the factor is the metric chain's own (tests/test_gpu_metrics.py holds it to numpy's); here it is read, as the product reads it
        fb = float(fb) * float(metrics.median_scale(dev(s["disp"]), dev(s["target"]), mode)[0].item())
    want, pred, gt = CR.product_ref(s["disp"], s["target"], s["P"], fb, CM.target_fb(mode, s["W"]), th, on=on, beams=beams, az_bins=256, max_depth=70.0)
    assert len(gt) > 50 and len(pred) > 50 and (on == "all" or beams or len(pred) <= int((s["target"] > 0).sum()))
    res = prod.result()
    tag = f"product {mode} on={on} beams={beams} median={median}"
    check_row(res["rows"][0], want, th, tag)
    assert res["frames"] == 1 and res["n_pred"][0] == len(pred) and res["n_gt"][0] == len(gt)
    d = CR.derived(res["rows"][0], th)
    assert res["chamfer"][0] == d["chamfer"] and res["f"][0].tolist() == d["f"] and 0 < res["chamfer_mean"] < 50
    summ = prod.summary()
    assert summ["frames"] == 1 and summ["on"] == on and summ["beams"] == beams and summ["chamfer"] == d["chamfer"] and summ["thresholds"] == list(th)
    json.dumps(summ)


# ---- 7. the command line ---------------------------------------------------------------------------------------------------------------------------------------
def _write_kitti2015(tmp_path, size=(375, 1242)):
    """<root>/Kitti2015/training/{image_2,image_3,disp_occ_0}: one generated KITTI-2015-shaped pair, as tests/test_gpu_sparsify.py builds them, with a
    ground truth on 2 % of the pixels."""
    from PIL import Image
    rng = np.random.default_rng(7)
    root = tmp_path / "data"
    for sub in ("image_2", "image_3"):
        d = root / "Kitti2015" / "training" / sub
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (*size, 3), dtype=np.uint8)).save(d / "000000_10.png")
    d = root / "Kitti2015" / "training" / "disp_occ_0"
    d.mkdir(parents=True, exist_ok=True)
    disp = ((rng.random(size) * 70 + 5) * 256).astype(np.uint16)
    disp[rng.random(size) < 0.98] = 0
    Image.fromarray(disp).save(d / "000000_10.png")
    return root


def _child(argv, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "Test_KITTI.py")] + argv, cwd=ROOT, env=dict(os.environ, FALNET_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_cli_end_to_end(tmp_path):
    root = _write_kitti2015(tmp_path)
    argv = ["-d", str(root), "-tn", "Kitti2015", "--allow-seeded-weights", "-w", "0", "-mspp", "False"]
    out = _child(argv + ["--save-path", str(tmp_path / "cm"), "--cloud-metrics", "--cm-thresholds", "0.5,2"])
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and list(lines[0]) == ["cloud", "file", "calibration"] and "=> cloud metrics: no calibration files" in out, out
    c = lines[0]["cloud"]
    assert c["frames"] == 1 and c["thresholds"] == [0.5, 2.0] and c["on"] == "gt" and c["beams"] == 0 and lines[0]["calibration"] == "nominal"
    assert c["n_gt"] > 1000 and 0 < c["n_pred"] <= c["n_gt"] * 1.5 and c["chamfer"] == c["accuracy"] + c["completeness"] and c["chamfer"] > 0
    assert all(0.0 <= v <= 1.0 for k in ("precision", "recall", "f") for v in c[k]) and c["precision"][0] <= c["precision"][1]
    txt = open(tmp_path / "cm" / "cloud_errors.txt").read().splitlines()
    assert lines[0]["file"].endswith("cloud_errors.txt") and "over 1 frames" in txt[0] and len(txt) == 4
    assert txt[2].split()[0] == "mean" and txt[3].split()[0] == "0" and "{:.6f}".format(c["chamfer"]) in txt[2] and txt[2].split()[3:] == txt[3].split()[3:]
    # the same command without the switch: no file, no extra line, the same errors.txt, and a settings.txt without the family's names
    out = _child(argv + ["--save-path", str(tmp_path / "plain")])
    assert len([ln for ln in out.splitlines() if ln.startswith("{")]) == 1 and '{"cloud"' not in out and "cloud metrics" not in out and not os.path.exists(tmp_path / "plain" / "cloud_errors.txt")
    assert open(tmp_path / "plain" / "errors.txt").read() == open(tmp_path / "cm" / "errors.txt").read()
    with_cm = dict(ln.split(":", 1) for ln in open(tmp_path / "cm" / "settings.txt").read().splitlines())
    plain = dict(ln.split(":", 1) for ln in open(tmp_path / "plain" / "settings.txt").read().splitlines())
    assert {k.strip() for k in with_cm} - {k.strip() for k in plain} == {"cloud_metrics", "cm_thresholds", "cm_on", "cm_beams", "cm_max_depth"}
    assert all(plain[k] == with_cm[k] for k in plain if k.strip() != "save_path")


# ---- the figures ------------------------------------------------------------------------------------------------------------------------------------------------
def test_zz_report_the_worst_case():
    """Prints the largest fraction of its bound that any sum reached in this session; FALNET_CLOUD_REPORT=<file> also writes the figures there."""
    lines = ["# sums of falnet_cloud_errors against math.fsum: the largest |difference| / bound per case (bound: tests/_cloud_ref.py: sum_bounds)",
             "# case | n_pred | n_gt | worst fraction of the bound"]
    lines += [f"{tag} | {n_p} | {n_g} | {ratio:.4f}" for tag, (ratio, n_p, n_g) in sorted(WORST.items())]
    print("\n".join(lines))
    path = os.environ.get("FALNET_CLOUD_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert all(ratio <= 1.0 for ratio, _, _ in WORST.values())
