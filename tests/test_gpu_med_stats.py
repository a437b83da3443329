"""The statistics of the MED distribution and the ordered compaction (csrc/med_stats.hip, csrc/compact.hip through the C-ABI,
fal_net_amd/confidence.py, Test_KITTI.py --stats / --pc-min-conf / --disparity) on the MI355X, element by element against the float64
reference of tests/_stats_ref.py:  |got - ref| <= u |ref| + c mag + eta with the derived coefficients recorded there; arg is exact.

Every output buffer is NaN before its launch and has a NaN guard region behind it that must stay NaN: an element the kernel never writes, or
one it writes out of bounds, is a violation.  Observed worst coefficients: profiles/med_stats_vs_f64.txt."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import confidence as C  # noqa: E402

import _head_ref as R  # noqa: E402
import _stats_ref as S  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 1024  # floats of NaN behind the output
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def raw_stats(dlog0, mn, mx, which, shape=None, null_out=False):
    """One falnet_med_stats_fwd call on device tensors into a NaN-pre-filled buffer of SIX planes per sample with a NaN guard behind it.
    shape overrides what the call is told (the refusals).  -> (return code, buffer as (B, 6, H, W) of which the launch may write the first
    K planes of each sample's K -- the view below is of a dense (B, K) launch only when K = 6 --, the flat buffer, guard intact)."""
    B, N, H, W = dlog0.shape if shape is None else shape
    flat = torch.full((dlog0.shape[0] * 6 * dlog0.shape[2] * dlog0.shape[3] + GUARD,), NAN, dtype=torch.float32, device=DEV)
    rc = L.lib().falnet_med_stats_fwd(L.ptr(dlog0), L.ptr(mn), L.ptr(mx), which, L.ptr(None if null_out else flat), B, N, H, W, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, flat, bool(torch.isnan(flat[-GUARD:]).all())


def launch(inp, which=S.ALL):
    """-> ({name: (B, 1, H, W) on the host} of the K outputs of a dense (B, K, H, W) launch, the floats behind them all NaN, guard intact)"""
    d0, mn, mx = inp["dlog0"].contiguous().to(DEV), inp["mn"].to(DEV), inp["mx"].to(DEV)
    B, N, H, W = d0.shape
    rc, flat, guard = raw_stats(d0, mn, mx, which)
    assert rc == 0, L.lib().falnet_last_error()
    names = [k for i, k in enumerate(S.KINDS) if which >> i & 1]
    K = len(names)
    out = flat[:B * K * H * W].view(B, K, H, W).cpu()
    rest_nan = bool(torch.isnan(flat[B * K * H * W:]).all())
    return {k: out[:, i:i + 1] for i, k in enumerate(names)}, rest_nan, guard


@pytest.mark.parametrize("case,family", S.listed())
def test_stats_against_float64(case, family):
    """All six outputs of every listed (case, logit family): every element within its bound, arg exact."""
    inp, ref = S.cached(case, family)
    got, rest_nan, guard = launch(inp)
    assert guard, "the NaN guard behind the output was written"
    res = S.compare_all(case, got, ref)
    for k, r in res.items():
        print(f"{case} {family} {k}: coef {r['coef']:.3g} (bound {S.coef(k, case):.3g}) worst ratio {r['worst_ratio']:.3g} max-norm {r['maxnorm']:.3g}")
    bad = {k: r for k, r in res.items() if r["bad"]}
    assert not bad, bad
    assert torch.equal(got["arg"].long(), S.first_argmax(inp["dlog0"]))
    if family == "c":
        assert float(got["arg"].abs().max()) == 0.0


def test_the_bound_can_fail():
    """Four mutations, each with elements over the bound, beside the unmutated comparison of the same launch, which has none."""
    case = (2, 49, 2, 128, 300.0)
    inp, ref = S.cached(case, "a")
    got, _, _ = launch(inp)
    assert not any(r["bad"] for r in S.compare_all(case, got, ref).values())
    # 1: a reference built from N - 1 planes
    res = S.compare_all(case, got, S.reference(inp, n_planes=case[1] - 1))
    print("N - 1 planes:", {k: r["bad"] for k, r in res.items()})
    assert all(res[k]["bad"] > 0 for k in ("mean", "std", "entropy"))
    # 3: a window of +-2 planes
    res = S.compare_all(case, got, S.reference(inp, window=2), kinds=("conf", "peak"))
    print("window of 2:", {k: r["bad"] for k, r in res.items()})
    assert res["conf"]["bad"] > 0 and res["peak"]["bad"] > 0
    # 2: std from E[d^2] - mean^2 in float32 at nearly one-hot pixels (an exactly one-hot one cancels exactly) -- and the kernel's centred std
    # of the same pixels within the bound
    case = (1, 128, 2, 64, 300.0)
    inp, ref = S.cached(case, "e")
    r = S.compare_all(case, S.f32_eval(inp, std_form="moments"), ref, kinds=("std",))["std"]
    print("moment form of std:", r["bad"], "of", r["n"], "max-norm", r["maxnorm"])
    assert r["bad"] > 0
    got, _, _ = launch(inp)
    assert S.compare_all(case, got, ref, kinds=("std",))["std"]["bad"] == 0
    # 4: last-index tie-breaking where every plane ties
    case = (2, 7, 3, 40, 30.0)
    inp, ref = S.cached(case, "c")
    got, _, _ = launch(inp)
    res = S.compare_all(case, got, S.reference(inp, last_tie=True), kinds=("arg", "peak"))
    print("last-index ties:", {k: r["bad"] for k, r in res.items()})
    assert res["arg"]["bad"] == res["arg"]["n"] and res["peak"]["bad"] > 0


@pytest.mark.parametrize("case", [(2, 7, 3, 40, 30.0), (2, 49, 2, 128, 300.0), (1, 128, 2, 64, 300.0)])
def test_subsets_are_the_planes_of_the_full_launch(case):
    """Each single bit and which = 0b101010: bit-identical to the same outputs of the all-six launch; K planes written, nothing beyond them."""
    inp, _ = S.cached(case, "a")
    full, _, _ = launch(inp)
    for which in [1 << b for b in range(6)] + [0b101010]:
        got, rest_nan, guard = launch(inp, which)
        assert guard and rest_nan, f"which={which:#b}: something beyond the K planes was written"
        assert list(got) == [k for i, k in enumerate(S.KINDS) if which >> i & 1]
        for k, v in got.items():
            assert torch.equal(v, full[k]), (which, k)
    st = C.stats(inp["dlog0"].to(DEV), inp["mn"].to(DEV), inp["mx"].to(DEV), ("peak", "std", "conf"))  # the wrapper, any order of names
    assert list(st) == ["std", "conf", "peak"]
    for k, v in st.items():
        assert v.shape == full[k].shape and torch.equal(v.cpu(), full[k])


def test_refusals():
    """Non-zero return with the whole buffer still NaN."""
    case = (2, 7, 3, 40, 30.0)
    inp, _ = S.cached(case, "a")
    d0, mn, mx = inp["dlog0"].to(DEV), inp["mn"].to(DEV), inp["mx"].to(DEV)
    B, N, H, W = d0.shape
    big = torch.zeros(B, 129, H, W, device=DEV)  # the call is told 129 planes: give it the memory for them (it must not touch any of it)
    trials = {
        "which = 0": dict(which=0),
        "which = 64": dict(which=64),
        "N = 1": dict(which=S.ALL, shape=(B, 1, H, W)),
        "N = 129": dict(which=S.ALL, shape=(B, 129, H, W), logits=big),
        "out = NULL": dict(which=S.ALL, null_out=True),
        "H = 0": dict(which=S.ALL, shape=(B, N, 0, W)),
    }
    for name, kw in trials.items():
        rc, flat, guard = raw_stats(kw.pop("logits", d0), mn, mx, **kw)
        assert rc != 0, name
        assert guard and bool(torch.isnan(flat).all()), name
    rc, flat, _ = raw_stats(d0, None, mx, S.ALL)
    assert rc != 0 and bool(torch.isnan(flat).all())
    assert L.lib().falnet_replay_op_index(b"falnet_med_stats_fwd") == -1 and L.lib().falnet_replay_op_index(b"falnet_compact_records") == -1


@pytest.mark.parametrize("case", [(2, 49, 2, 128, 300.0), (1, 49, 2, 1242, 300.0)])
def test_stats_are_deterministic(case):
    inp, _ = S.cached(case, "b")
    g1, _, _ = launch(inp)
    g2, _, _ = launch(inp)
    for k in S.KINDS:
        assert torch.equal(g1[k], g2[k]), k


def _model(arch, n, dtype=torch.float32):
    from fal_net_amd import models, synthetic
    sd = synthetic.seeded_state_dict(arch, n)
    return models.__dict__["FAL_net" + arch]({"state_dict": sd}, no_levels=n, compute_dtype=dtype).to(DEV).eval()


@pytest.mark.parametrize("arch,n,dtype", [("B", 49, torch.float32), ("B", 49, torch.bfloat16), ("A", 33, torch.float32)])
def test_from_model_reads_the_plans_own_logits(arch, n, dtype):
    """confidence.from_model on a seeded model: every statistic held to the float64 reference of the plan's own dlog0 (copied after the call) --
    `mean` and the forward's `disp` both to the head's own disp coefficient --, and bit for bit what stats() gives on those logits."""
    from fal_net_amd import synthetic
    B, H, W = 1, 64, 128
    model = _model(arch, n, dtype)
    left, _, _, _ = synthetic.synthetic_pair(B, H, W, seed=11)
    left = left.to(DEV)
    mx = torch.tensor([300.0], device=DEV).view(B, 1, 1)
    mn = mx * 2 / 300
    names = ("mean", "std", "entropy", "arg", "conf", "peak")
    st, disp = C.from_model(model, left, mn, mx, names)
    buf = model._plan(B, H, W, left.device).buf
    assert buf["dlog0"].dtype == torch.float32 and tuple(buf["dlog0"].shape) == (B, n, H, W)
    inp = {"dlog0": buf["dlog0"].cpu(), "mn": buf["min_disp"].reshape(-1).float().cpu(), "mx": buf["max_disp"].reshape(-1).float().cpu()}
    ref = S.reference(inp)
    case = (B, n, H, W, 300.0)
    res = S.compare_all(case, {k: v.cpu() for k, v in st.items()}, ref)
    for k, r in res.items():
        print(f"FAL_net{arch} {dtype} {k}: coef {r['coef']:.3g} worst ratio {r['worst_ratio']:.3g}")
    assert not {k: r for k, r in res.items() if r["bad"]}
    r = R.compare(disp.float().cpu(), ref["mean"], ref["mean"], torch.float32, R.coef("disp", case))
    assert not r["bad"], r
    again = C.stats(buf["dlog0"], buf["min_disp"], buf["max_disp"], names)
    for k in names:
        assert st[k].shape == (B, 1, H, W) and torch.equal(st[k], again[k]), k


# ------------------------------------------------------------------------------------------------------------------- compaction
FILL = 0xA5
PAD = 64  # bytes of pre-fill behind dst


def raw_compact(rec, score, thr):
    """One falnet_compact_records call; dst is pre-filled with FILL and PAD bytes longer than src.  -> (rc, dst bytes on the host, count)"""
    n = len(score)
    rb = rec.nbytes // n
    src = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV)
    dst = torch.full((n * rb + PAD,), FILL, dtype=torch.uint8, device=DEV)
    sc = torch.from_numpy(score).to(DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    lib = L.lib()
    ws = torch.empty(int(lib.falnet_compact_workspace_bytes(n)) // 8, dtype=torch.int64, device=DEV)
    rc = lib.falnet_compact_records(L.ptr(src), rb, L.ptr(sc), float(thr), n, L.ptr(dst), L.ptr(count), L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy(), int(count.item())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048, 2049, 65537, 256 * 2048, 256 * 2048 + 1, 2 * 256 * 2048 + 2049])
@pytest.mark.parametrize("rec_bytes", [4, 15])
def test_compaction_against_numpy(n, rec_bytes):
    """dst[:count] and count equal numpy's boolean indexing byte for byte, the bytes beyond keep their pre-fill; kept fraction 0, 1 and about
    a half, NaN scores present.  (2048 and 2049: one workgroup's tile of csrc/compact.hip and one record more, beside the issue's sizes.
    The offset scan takes 256 workgroup counts at a time and carries a base: 256 * 2048 records are exactly one such chunk, one record more
    puts a single workgroup with a single record into a second chunk, and the last size needs three.)"""
    rec = S.make_records(n, rec_bytes)
    for kind in ("none", "all", "half"):
        score = S.make_scores(n, kind)
        want = S.compact_ref(rec, score, 0.5)
        rc, dst, count = raw_compact(rec, score, 0.5)
        assert rc == 0, L.lib().falnet_last_error()
        assert count == len(want), (kind, count, len(want))
        assert dst[:count * rec_bytes].tobytes() == want.tobytes(), kind
        assert bool((dst[count * rec_bytes:] == FILL).all()), f"{kind}: bytes beyond the kept records were written"
        assert {"none": count == 0, "all": count == n, "half": n == 1 or 0 < count < n}[kind]


def test_compaction_refusals():
    rec, score = S.make_records(8, 4), S.make_scores(8, "all")
    lib = L.lib()
    src, sc = torch.from_numpy(rec).to(DEV), torch.from_numpy(score).to(DEV)
    dst = torch.full((64,), FILL, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    ws = torch.zeros(4, dtype=torch.int64, device=DEV)
    for rb, n, s, d in ((8, 8, src, dst), (16, 8, src, dst), (4, 0, src, dst), (4, 8, None, dst), (4, 8, src, None)):
        rc = lib.falnet_compact_records(L.ptr(s), rb, L.ptr(sc), 0.5, n, L.ptr(d), L.ptr(count), L.ptr(ws), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0, (rb, n)
        assert bool((dst == FILL).all()) and int(count.item()) == -7 and int(ws.abs().sum()) == 0


@pytest.mark.parametrize("packed", [True, False])
def test_filter_point_cloud_is_the_dump_indexed_by_the_score(packed):
    """A 6 x 10 frame: the kept vertices are dumps.point_cloud's own output indexed by conf >= C -- the existing kernel's bytes, so `==`."""
    from fal_net_amd import dumps
    g = torch.Generator().manual_seed(3)
    B, H, W, thr = 2, 6, 10, 0.4
    img = (torch.rand(B, 3, H, W, generator=g) - 0.43).to(DEV)
    disp = (torch.rand(B, 1, H, W, generator=g) * 40 + 1).to(DEV)
    conf = torch.rand(B, 1, H, W, generator=g)
    conf[0, 0, 2, 3] = NAN
    conf[1, 0, 0, 0] = thr
    conf = conf.to(DEV)
    kept, counts = C.filter_point_cloud(img, disp, conf, thr, packed=packed, focal=721.0, baseline=0.54)
    full = dumps.point_cloud(img, disp, 721.0, 0.54, packed=packed)
    for b in range(B):
        mask = (conf[b].reshape(-1) >= thr)
        want = full[b][mask] if packed else full[b][:, mask]
        assert counts[b] == int(mask.sum()) and 0 < counts[b] < H * W
        assert kept[b].shape == want.shape and torch.equal(kept[b], want)


# ------------------------------------------------------------------------------------------------------------------- command line
def _run_cli(tmp, *extra):
    env = dict(os.environ, FALNET_DETERMINISTIC="1")
    cmd = [sys.executable, os.path.join(ROOT, "Test_KITTI.py"), "--synthetic", "--height", "128", "--width", "416", "--iters", "1",
           "-mspp", "False", "-fpp", "False", "--save-path", str(tmp)] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]


def _ply_vertices(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    n = int([ln for ln in raw[:end].decode("ascii").splitlines() if ln.startswith("element vertex")][0].split()[-1])
    assert len(raw) - end == 15 * n, "the PLY body does not hold the header's vertex count"
    return n


def test_cli_stats_end_to_end(tmp_path):
    from PIL import Image
    H, W = 128, 416
    out = tmp_path / "stats"
    lines = _run_cli(out, "--stats", "std,entropy,arg,conf,peak", "--dump", "pc", "--pc-min-conf", "0.5")
    assert len(lines) == 2 and list(lines[0]) == ["stats"], lines
    st = lines[0]["stats"]
    assert st["kinds"] == ["std", "entropy", "arg", "conf", "peak"] and st["files"] == 5 and st["frames"] == 1
    assert all(math.isfinite(st[k]) for k in ("mean_std", "mean_entropy", "mean_conf"))
    assert st["mean_std"] >= 0 and 0 <= st["mean_entropy"] <= 1 + 1e-6 and 0 < st["mean_conf"] <= 1 + 1e-6
    for k in st["kinds"]:
        assert Image.open(out / "stats" / "{:010d}_{}.png".format(0, k)).size == (W, H), k
    n = _ply_vertices(out / "Point_cloud" / "{:010d}.ply".format(0))
    assert n == st["pc_kept"] and n < H * W and st["pc_vertices"] == H * W and st["pc_min_conf"] == 0.5
    assert st["pc_kept_fraction"] == pytest.approx(n / (H * W))
    # the same command on the same seed without the new switches: no stats folder, one line, the whole cloud -- and the same numbers
    plain = tmp_path / "plain"
    plain_lines = _run_cli(plain, "--dump", "pc")
    assert len(plain_lines) == 1 and not os.path.exists(plain / "stats")
    assert _ply_vertices(plain / "Point_cloud" / "{:010d}.ply".format(0)) == H * W
    drop = lambda d: {k: v for k, v in d.items() if k != "sec_per_image_median"}  # noqa: E731
    assert drop(plain_lines[0]) == drop(lines[1])


def test_cli_peak_disparity(tmp_path):
    lines = _run_cli(tmp_path / "peak", "--disparity", "peak", "--device-metrics")
    assert len(lines) == 1
    assert math.isfinite(lines[0]["disp_mean"]) and math.isfinite(lines[0]["disp_max"]) and lines[0]["disp_mean"] > 0
    assert lines[0]["post"] == "none"
