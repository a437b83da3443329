"""The background-biased pull-push (csrc/inpaint.hip through the C-ABI, fal_net_amd/inpaint.py, freeview.fill_views, Test_KITTI.py --freeview-fill)
on the MI355X, element by element against the float64 reference of tests/_inpaint_ref.py:  |got - ref| <= K (L + 1) 2^-24 M  with the derived K
of that module (the ratios reached: profiles/inpaint_vs_f64.txt).

`out` and the workspace are NaN before every launch and sit between NaN guard zones that must stay NaN; `out` must be finite everywhere after
it: an element the kernels never write, or one they write out of bounds, is a violation."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import freeview as FV  # noqa: E402
from fal_net_amd import inpaint as IP  # noqa: E402

import _inpaint_ref as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 1024  # floats of NaN before and behind `out` and the workspace
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def raw_fill(values, weight, guide, scale, beta, floor=R.FLOOR, shape=None, null=(), ws_bytes=None, alias=False, shift=0):
    """One falnet_inpaint_fwd call on device tensors; `out` and the workspace NaN-pre-filled between NaN guard zones.  shape / null / ws_bytes /
    alias override what the call is told (the refusals); shift moves `out` and the workspace by that many floats (off 16-byte alignment).
    -> (return code, out (I, C, H, W), the workspace's body, guards intact)."""
    I, C, H, W = values.shape
    need = 4 * R.workspace_floats(C, H, W, I)
    full_o = torch.full((values.numel() + 2 * GUARD + shift,), NAN, dtype=torch.float32, device=DEV)
    full_w = torch.full((need // 4 + 2 * GUARD + shift,), NAN, dtype=torch.float32, device=DEV)
    out, ws = full_o[GUARD + shift:GUARD + shift + values.numel()], full_w[GUARD + shift:GUARD + shift + need // 4]
    args = {"values": values, "weight": weight, "guide": guide, "scale": scale, "out": values if alias else out, "ws": ws}
    p = {k: L.ptr(None if k in null else t) for k, t in args.items()}
    rc = L.lib().falnet_inpaint_fwd(p["values"], p["weight"], p["guide"], p["scale"], beta, floor, p["out"], p["ws"], need if ws_bytes is None else ws_bytes,
                                    *((I, C, H, W) if shape is None else shape), L.stream_ptr())
    torch.cuda.synchronize()
    guards = all(bool(torch.isnan(f[:GUARD + shift]).all()) and bool(torch.isnan(f[f.numel() - GUARD:]).all()) for f in (full_o, full_w))
    return rc, out.view(I, C, H, W), ws, guards


def on_device(inp):
    return tuple(torch.from_numpy(inp[k]).to(DEV) for k in ("values", "weight", "guide", "guide_scale"))


def check(got, ref, M, H, W, label):
    """Every element of every image within the bound; prints the largest ratio (the figure of profiles/inpaint_vs_f64.txt)."""
    assert bool(torch.isfinite(got).all()), f"{label}: a non-finite element in out"
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    worst = 0.0
    for i, m in enumerate(M):
        b = R.bound(H, W, m)
        ratio = float(err[i].max() / b) if b > 0 else (0.0 if err[i].max() == 0 else float("inf"))
        worst = max(worst, ratio)
    print(f"{label}: largest |got - ref| / bound {worst:.3g}")
    assert worst <= 1.0, (label, worst)
    return worst


# every (shape, family) with three parameter sets that between them take every C, every I and every beta of the list
COMBOS = [(4, 1, 4.0), (3, 3, 0.0), (1, 1, 8.0)]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_inpaint_against_float64(H, W, family):
    for C, I, beta in COMBOS:
        inp, ref, M = R.cached(H, W, C, I, family, 0, beta)
        rc, got, _, guards = raw_fill(*on_device(inp), beta)
        assert rc == 0 and guards, L.lib().falnet_last_error()
        check(got, ref, M, H, W, f"{H}x{W} {family} C={C} I={I} beta={beta:g}")
        if family == "zero":
            assert not bool(got.any())
        if family == "ones":
            assert torch.equal(got.cpu(), torch.from_numpy(inp["values"]))


def test_inpaint_full_size_once():
    H, W = R.FULL
    inp, ref, M = R.cached(H, W, 4, 1, "wedge", 0, 4.0)
    rc, got, _, guards = raw_fill(*on_device(inp), 4.0)
    assert rc == 0 and guards, L.lib().falnet_last_error()
    check(got, ref, M, H, W, f"{H}x{W} wedge C=4 I=1 beta=4")


@pytest.mark.parametrize("H,W,family", [(256, 384, "sparse"), (1030, 1344, "wedge")])
def test_inpaint_other_hand_over_levels(H, W, family):
    """With C = 4 the listed shapes hand over to the apex workgroup at levels 0, 1, 2 and 4.  256 x 384 hands over at level 3 (level 2 is the
    last that does not fit its LDS); 1030 x 1344 at level 5, the smallest kind of image whose pull and push take two tile launches each, the
    second on stored levels (level 4 is 65 x 84: 16-byte rows there too)."""
    inp, ref, M = R.cached(H, W, 4, 1, family, 0, 4.0)
    rc, got, _, guards = raw_fill(*on_device(inp), 4.0)
    assert rc == 0 and guards, L.lib().falnet_last_error()
    check(got, ref, M, H, W, f"{H}x{W} {family} C=4 I=1 beta=4")


def test_the_bound_can_fail():
    """The comparator bites: the device's output of beta = 4 against the reference of beta = 2."""
    H, W = 37, 124
    inp, _, M = R.cached(H, W, 3, 1, "sparse", 0, 4.0)
    _, other, _ = R.cached(H, W, 3, 1, "sparse", 0, 2.0)
    rc, got, _, guards = raw_fill(*on_device(inp), 4.0)
    assert rc == 0 and guards
    err = np.abs(got.cpu().numpy().astype(np.float64) - other)
    assert err.max() > 100 * R.bound(H, W, M[0])


@pytest.mark.parametrize("H,W", [(65, 63), (37, 124), (129, 200)])
def test_exact_properties(H, W):
    inp = R.inputs(H, W, 4, 3, "dense", 1)
    v, w, g, s = on_device(inp)
    rc, got, _, guards = raw_fill(v, w, g, s, 4.0)
    assert rc == 0 and guards
    full = (w == 1.0).expand_as(v)
    assert int(full.sum()) > 0 and torch.equal(got[full], v[full])  # weight == 1: bit for bit
    rc, again, _, guards = raw_fill(v, w, g, s, 4.0)
    assert rc == 0 and guards and torch.equal(got, again)  # two calls, the same bits
    for i in range(3):  # image i of the batch equals its own call
        rc, single, _, guards = raw_fill(v[i:i + 1].contiguous(), w[i:i + 1].contiguous(), g[i:i + 1].contiguous(), s[i:i + 1].contiguous(), 4.0)
        assert rc == 0 and guards and torch.equal(single[0], got[i]), i
    rc, off, _, guards = raw_fill(v, w, g, s, 4.0, shift=1)  # out and the workspace off 16-byte alignment: the scalar paths, the same bits
    assert rc == 0 and guards and torch.equal(off, got)
    rc, plain, _, guards = raw_fill(v, w, g, s, 0.0, null=("guide", "scale"))
    assert rc == 0 and guards
    rc, nan_guide, _, guards = raw_fill(v, w, torch.full_like(g, NAN), torch.full_like(s, NAN), 0.0)
    assert rc == 0 and guards and torch.equal(plain, nan_guide)  # beta = 0 never reads the guide


def test_dropped_pixels_do_not_leak():
    """NaN in values (and in the guide) under weight < floor does not reach out, which equals the run with zeros there."""
    H, W = 65, 63
    inp = R.inputs(H, W, 3, 1, "floor", 2)
    v, w, g, s = on_device(inp)
    rc, clean, _, guards = raw_fill(v, w, g, s, 4.0)
    assert rc == 0 and guards
    dropped = w < R.FLOOR
    assert 0 < int(dropped.sum()) < w.numel()
    rc, dirty, _, guards = raw_fill(torch.where(dropped.expand_as(v), torch.full_like(v, NAN), v), w, torch.where(dropped, torch.full_like(g, NAN), g), s, 4.0)
    assert rc == 0 and guards and bool(torch.isfinite(dirty).all()) and torch.equal(dirty, clean)


def test_refusals():
    """Non-zero return with `out` and the workspace still NaN and every guard intact."""
    H, W = 37, 124
    inp = R.inputs(H, W, 3, 2, "dense", 3)
    v, w, g, s = on_device(inp)
    need = 4 * R.workspace_floats(3, H, W, 2)
    trials = {
        "null values": dict(null=("values",)), "null weight": dict(null=("weight",)), "null out": dict(null=("out",)), "null workspace": dict(null=("ws",)),
        "no guide": dict(null=("guide",)), "no guide_scale": dict(null=("scale",)), "out is values": dict(alias=True),
        "C = 0": dict(shape=(2, 0, H, W)), "C = 5": dict(shape=(1, 5, H, W)), "I = 0": dict(shape=(0, 3, H, W)), "H = 0": dict(shape=(2, 3, 0, W)),
        "W = -1": dict(shape=(2, 3, H, -1)), "plane above 2^30": dict(shape=(1, 1, 1 << 16, (1 << 14) + 1)),
        "beta < 0": dict(beta=-0.5), "beta > 8": dict(beta=8.5), "beta nan": dict(beta=NAN), "beta inf": dict(beta=float("inf")),
        "floor 0": dict(floor=0.0), "floor > 1": dict(floor=1.5), "floor nan": dict(floor=NAN), "workspace too small": dict(ws_bytes=need - 4),
    }
    for name, kw in trials.items():
        beta = kw.pop("beta", 4.0)
        rc, out, ws, guards = raw_fill(v, w, g, s, beta, **kw)
        assert rc != 0, name
        assert guards and bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()), name
        if name == "out is values":
            assert torch.equal(v.cpu(), torch.from_numpy(inp["values"])), name
    assert L.lib().falnet_replay_op_index(b"falnet_inpaint_fwd") == -1


def test_wrapper(monkeypatch):
    """fill folds leading dimensions into one call, expands guide_scale, takes (..., H, W) planes and a caller's workspace; refusals launch nothing."""
    H, W = 37, 124
    inp = R.inputs(H, W, 3, 6, "wedge", 4)
    v, w, g, s = on_device(inp)
    calls = []
    real = L.lib().falnet_inpaint_fwd
    monkeypatch.setattr(L.lib(), "falnet_inpaint_fwd", lambda *a: calls.append(a) or real(*a))
    rc, want, _, guards = raw_fill(v, w, g, s, 4.0)
    assert rc == 0 and guards and len(calls) == 1
    got = IP.fill(v.view(2, 3, 3, H, W), w.view(2, 3, H, W), guide=g.view(2, 3, 1, H, W), guide_scale=s, beta=4.0)
    assert len(calls) == 2 and calls[-1][9] == 6 and got.shape == (2, 3, 3, H, W) and torch.equal(got.view(6, 3, H, W), want)
    ws = torch.full((IP.workspace_bytes(3, H, W, 6) // 4,), NAN, device=DEV)
    same_scale = IP.fill(v, w, g, 100.0, beta=4.0, workspace=ws)
    rc, want, _, _ = raw_fill(v, w, g, torch.full((6,), 100.0, device=DEV), 4.0)
    assert torch.equal(same_scale, want)
    assert torch.equal(IP.fill(v, w), raw_fill(v, w, None, None, 0.0, null=("guide", "scale"))[1])
    n = len(calls)
    for kw in (dict(beta=9.0), dict(beta=2.0), dict(floor=0.0), dict(workspace=ws[:100]), dict(beta=2.0, guide=g, guide_scale=[1.0, 2.0])):
        with pytest.raises(ValueError):
            IP.fill(v, w, **kw)
    assert len(calls) == n


def seeded_warp():
    """freeview.warp on seeded logits, 37 x 124, N = 8, one pose at centre (0.5, 0.25, 0) baselines with 3 degrees of yaw."""
    B, N, H, W = 1, 8, 37, 124
    gen = torch.Generator().manual_seed(5)
    dlog0 = (torch.randn(B, N, H, W, generator=gen) * 3.0).to(DEV)
    left = torch.rand(B, 3, H, W, generator=gen).to(DEV)
    mx = torch.tensor([40.0], device=DEV)
    mn = torch.tensor([2.0], device=DEV)
    pose = FV.pose(FV.camera(H, W), centre=(0.5, 0.25, 0.0), yaw=3.0)
    return FV.warp(dlog0, left, mn, mx, [pose]), mx


def test_fill_views_is_one_four_channel_call():
    out, mx = seeded_warp()
    assert float(out["cover"].min()) < R.FLOOR and float(out["cover"].max()) > 0.99  # there are holes to fill
    filled = FV.fill_views(out, mx, beta=4.0)
    assert sorted(filled) == ["disp", "view"] and filled["view"].shape == out["view"].shape and filled["disp"].shape == out["disp"].shape
    by_hand = IP.fill(torch.cat([out["view"], out["disp"] * out["cover"]], 2), out["cover"], guide=out["disp"], guide_scale=mx.view(1, 1), beta=4.0)
    assert torch.equal(filled["view"], by_hand[:, :, :3]) and torch.equal(filled["disp"], by_hand[:, :, 3:])
    assert bool(torch.isfinite(by_hand).all())
    assert float(filled["view"].min()) >= -1e-5 and float(filled["view"].max()) <= 1.0 + 1e-5  # inside the range of the left image's colours
    assert torch.equal(FV.fill_views(out, mx)["view"], filled["view"])  # 4.0 is the default


def test_render_fill_none_is_what_it_was():
    from fal_net_amd import models, synthetic
    B, H, W = 1, 64, 128
    sd = synthetic.seeded_state_dict("B", 49)
    model = models.__dict__["FAL_netB"]({"state_dict": sd}, no_levels=49, compute_dtype=torch.float32).to(DEV).eval()
    left = synthetic.synthetic_pair(B, H, W, seed=11)[0].to(DEV)
    mx = torch.tensor([300.0], device=DEV).view(B, 1, 1)
    mn = mx * 2 / 300
    poses = [FV.pose(FV.camera(H, W), **kw) for kw in FV.paths.orbit(2, 0.5, 0.25, yaw=3.0)]
    out, disp = FV.render(model, left, mn, mx, poses, want=("view", "cover"))
    buf = model._plan(B, H, W, left.device).buf
    direct = FV.warp(buf["dlog0"], buf["left"], buf["min_disp"], buf["max_disp"], poses, ("view", "cover"))
    assert list(out) == ["view", "cover"] and all(torch.equal(out[k], direct[k]) for k in out) and torch.equal(disp, buf["disp"])
    both, disp2 = FV.render(model, left, mn, mx, poses, want=("view", "cover"), fill=4.0)
    # a second forward (its convolutions need not repeat the first one's bits): held to the plan's buffers as they are now
    assert list(both) == ["view", "cover", "view_filled", "disp_filled"] and torch.equal(disp2, buf["disp"])
    full = FV.warp(buf["dlog0"], buf["left"], buf["min_disp"], buf["max_disp"], poses)
    assert all(torch.equal(both[k], full[k]) for k in out)
    full = FV.warp(buf["dlog0"], buf["left"], buf["min_disp"], buf["max_disp"], poses)
    filled = FV.fill_views(full, buf["max_disp"], beta=4.0)
    assert torch.equal(both["view_filled"], filled["view"]) and torch.equal(both["disp_filled"], filled["disp"])
    with pytest.raises(ValueError):
        FV.render(model, left, mn, mx, poses, fill=9.0)


def run_cli(tmp, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "Test_KITTI.py"), "--synthetic", "--height", "75", "--width", "250", "--freeview", "2", "--iters", "1",
           "--save-path", str(tmp)] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    return [l["freeview"] for l in lines if "freeview" in l], sorted(os.path.basename(f) for f in glob.glob(str(tmp / "Freeview" / "*.png")))


def test_cli_freeview_fill_end_to_end(tmp_path):
    from PIL import Image
    fv, names = run_cli(tmp_path / "on", "--freeview-fill")
    assert len(fv) == 1 and fv[0]["fill"] == {"beta": 4.0, "floor": 2.0 ** -10, "levels": 8}, fv
    assert fv[0]["files"] == 6 and fv[0]["filled"] == 2 and fv[0]["poses"] == 2, fv
    assert names == sorted("{:010d}_p{:02d}{}.png".format(0, j, s) for j in range(2) for s in ("", "_cover", "_filled")), names
    for n in names:
        im = Image.open(tmp_path / "on" / "Freeview" / n)
        assert im.size == (250, 75) and im.mode == ("L" if n.endswith("_cover.png") else "RGB"), (n, im.size, im.mode)
    fv, names = run_cli(tmp_path / "off")
    assert len(fv) == 1 and "fill" not in fv[0] and "filled" not in fv[0] and fv[0]["files"] == 4, fv
    assert not [n for n in names if "_filled" in n] and len(names) == 4, names
