"""The baseline sweep (csrc/med_sweep.hip through the C-ABI, fal_net_amd/views.py, dumps.SweepWriter, Test_KITTI.py --sweep) on the MI355X,
element by element against the float64 reference of tests/_sweep_ref.py:  |got - ref| <= u |ref| + c mag + eta.

Every output buffer is NaN before its launch and has a NaN guard region behind it that must stay NaN: an element the kernel never writes,
or one it writes out of bounds, is a violation.  The t = 1 view is held to the head's own p_im0 coefficient, the other views and the
disparities to the measured coefficients of _sweep_ref.COEF (raw figures: profiles/sweep_vs_f64.txt)."""
import ctypes
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
from fal_net_amd import views as V  # noqa: E402

import _head_ref as R  # noqa: E402
import _sweep_ref as S  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 1024  # floats of NaN behind each output
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def raw_sweep(dlog0, left, mn, mx, ts, want_views=True, want_disps=True, n_views=None, shape=None):
    """One falnet_med_sweep_fwd call on device tensors from NaN-pre-filled outputs with a NaN guard behind each.  n_views / shape override
    what the call is told (the refusals).  -> (return code, views or None, disps or None, guards_intact) with BOTH buffers returned even
    when one of them is not passed to the library (its NaNs must then be intact)."""
    B, N, H, W = dlog0.shape if shape is None else shape
    nv = len(ts) if n_views is None else n_views
    rows = max(len(ts), 1)
    fv = torch.full((B * rows * 3 * H * W + GUARD,), NAN, dtype=torch.float32, device=DEV)
    fd = torch.full((B * rows * H * W + GUARD,), NAN, dtype=torch.float32, device=DEV)
    t_host = (ctypes.c_float * max(len(ts), 1))(*ts)
    rc = L.lib().falnet_med_sweep_fwd(L.ptr(dlog0), L.ptr(left), L.ptr(mn), L.ptr(mx), ctypes.cast(t_host, ctypes.c_void_p), nv,
                                      L.ptr(fv if want_views else None), L.ptr(fd if want_disps else None), B, N, H, W, L.stream_ptr())
    torch.cuda.synchronize()
    guards = bool(torch.isnan(fv[-GUARD:]).all()) and bool(torch.isnan(fd[-GUARD:]).all())
    return rc, fv[:-GUARD].view(B, rows, 3, H, W), fd[:-GUARD].view(B, rows, 1, H, W), guards


def on_device(inp):
    return inp["dlog0"].contiguous().to(DEV), inp["left"].to(DEV), inp["mn"].to(DEV), inp["mx"].to(DEV)


@pytest.mark.parametrize("case,set_name,family", S.listed())
def test_sweep_against_float64(case, set_name, family):
    """Views and disparities of every listed (case, baseline set, logit family): every element within the bound.  At set Z (t = 0) the views
    are also held to `left` itself and the disparity to the forward's float64 `disp`."""
    ts = S.SETS[set_name]
    inp, ref = S.cached(case, set_name, family)
    rc, views, disps, guards = raw_sweep(*on_device(inp), ts)
    assert rc == 0, L.lib().falnet_last_error()
    assert guards, "the NaN guard behind an output was written"
    res = S.compare_views(case, ts, views.cpu(), disps.cpu(), ref)
    if set_name == "Z":
        left64, disp64 = inp["left"].to(torch.float64), S.cached_inputs(case, family)[1]
        res.append(("view=left", 0, 0.0, R.compare(views[:, 0].cpu(), left64, ref["mag_view"][:, 0], torch.float32, S.coef("view", case, 0.0))))
        res.append(("disp=forward", 0, 0.0, R.compare(disps[:, 0].cpu(), disp64, disp64, torch.float32, S.coef("disp", case))))
    for what, v, t, r in res:
        print(f"{case} {set_name} {family} {what}[{v}] t={t}: coef {r['coef']:.3g} worst ratio {r['worst_ratio']:.3g} max-norm {r['maxnorm']:.3g}")
    bad = [(what, v, t, r) for what, v, t, r in res if r["bad"]]
    assert not bad, bad


def test_sweep_bound_can_fail():
    """The comparator bites: the reference of t = 0.5 against the kernel's output at t = 0.75."""
    case = (2, 49, 2, 128, 300.0)
    inp, _ = S.cached_inputs(case, "a")
    ref = S.reference(inp, (0.5,))
    rc, views, disps, _ = raw_sweep(*on_device(inp), (0.75,))
    assert rc == 0
    res = S.compare_views(case, (0.5,), views.cpu(), disps.cpu(), ref)
    for what, v, t, r in res:
        print(f"mutation {what}: {r['bad']} of {r['n']} over the bound, worst ratio {r['worst_ratio']:.3g}")
        assert r["bad"] > 0, (what, r)


@pytest.mark.parametrize("case", [(2, 7, 3, 40, 30.0), (1, 49, 2, 1242, 300.0), (1, 7, 1, 2100, 300.0)])
def test_sweep_partial_outputs(case):
    """views NULL: only disps is written (and equals the full launch's bit for bit), and the reverse; the other buffer's NaNs are intact."""
    inp, _ = S.cached_inputs(case, "a")
    dev = on_device(inp)
    ts = S.SETS["C"]
    rc, views, disps, guards = raw_sweep(*dev, ts)
    assert rc == 0 and guards
    rc, v1, d1, guards = raw_sweep(*dev, ts, want_views=False)
    assert rc == 0 and guards
    assert bool(torch.isnan(v1).all()) and torch.equal(d1, disps)
    rc, v2, d2, guards = raw_sweep(*dev, ts, want_disps=False)
    assert rc == 0 and guards
    assert bool(torch.isnan(d2).all()) and torch.equal(v2, views)


def test_sweep_refusals():
    """Non-zero return with every output still NaN."""
    case = (2, 7, 3, 40, 30.0)
    inp, _ = S.cached_inputs(case, "a")
    d0, lf, mn, mx = on_device(inp)
    B, N, H, W = d0.shape
    one, nine = (1.0,), (0.1,) * 9
    trials = {
        "V = 0": dict(ts=one, n_views=0),
        "V = 9": dict(ts=nine, n_views=9),
        "both outputs null": dict(ts=one, want_views=False, want_disps=False),
        "N = 1": dict(ts=one, shape=(B, 1, H, W)),
        "N = 129": dict(ts=one, shape=(B, 129, H, W)),
        "t = nan": dict(ts=(0.5, NAN)),
        "t = inf": dict(ts=(float("inf"),)),
        "t = 2.5": dict(ts=(1.0, 2.5, 0.0)),
    }
    for name, kw in trials.items():
        if name == "N = 129":  # the call is told 129 planes: give it the memory for them (it must not touch any of it)
            big = torch.zeros(B, 129, H, W, device=DEV)
            rc, views, disps, guards = raw_sweep(big, lf, mn, mx, **kw)
        else:
            rc, views, disps, guards = raw_sweep(d0, lf, mn, mx, **kw)
        assert rc != 0, name
        assert guards and bool(torch.isnan(views).all()) and bool(torch.isnan(disps).all()), name


@pytest.mark.parametrize("case", [(2, 49, 2, 128, 300.0), (1, 49, 2, 1242, 300.0)])
def test_sweep_is_deterministic(case):
    inp, _ = S.cached_inputs(case, "b")
    dev = on_device(inp)
    _, v1, d1, _ = raw_sweep(*dev, S.SETS["B"])
    _, v2, d2, _ = raw_sweep(*dev, S.SETS["B"])
    assert torch.equal(v1, v2) and torch.equal(d1, d2)


def test_wrapper_splits_into_launches_of_eight():
    case = (2, 49, 2, 128, 300.0)
    inp, _ = S.cached_inputs(case, "a")
    dev = on_device(inp)
    ts = [-1.0 + 0.25 * i for i in range(11)]
    views, disps = V.sweep(*dev, ts)
    assert views.shape == (2, 11, 3, 2, 128) and disps.shape == (2, 11, 1, 2, 128)
    v8, d8 = V.sweep(*dev, ts[:8])
    v3, d3 = V.sweep(*dev, ts[8:])
    assert torch.equal(views, torch.cat((v8, v3), 1)) and torch.equal(disps, torch.cat((d8, d3), 1))
    _, raw_v, raw_d, _ = raw_sweep(*dev, ts[8:])
    assert torch.equal(v3, raw_v) and torch.equal(d3, raw_d)
    only_d = V.sweep(*dev, ts, want_views=False)
    assert only_d[0] is None and torch.equal(only_d[1], disps)


def test_wrapper_refuses_before_any_launch(monkeypatch):
    inp, _ = S.cached_inputs((2, 7, 3, 40, 30.0), "a")
    dev = on_device(inp)
    calls = []
    real = L.lib().falnet_med_sweep_fwd
    monkeypatch.setattr(L.lib(), "falnet_med_sweep_fwd", lambda *a: calls.append(a) or real(*a))
    V.sweep(*dev, (0.5,))
    assert len(calls) == 1  # the spy sees launches
    for bad in ([0.1] * 8 + [3.0], [float("nan")], []):  # the refused fraction sits in the SECOND launch: the first must not run either
        with pytest.raises(ValueError):
            V.sweep(*dev, bad)
    with pytest.raises(ValueError):
        V.sweep(*dev, (0.5,), want_views=False, want_disps=False)
    assert len(calls) == 1


def _model(arch, n, dtype=torch.float32):
    from fal_net_amd import models, synthetic
    sd = synthetic.seeded_state_dict(arch, n)
    return models.__dict__["FAL_net" + arch]({"state_dict": sd}, no_levels=n, compute_dtype=dtype).to(DEV).eval()


@pytest.mark.parametrize("arch,n", [("B", 49), ("A", 33)])
def test_render_from_the_models_own_logits(arch, n):
    """views.render on a seeded model: held to the float64 reference of the plan's own dlog0 (copied after the call) with the caller's
    min_disp / max_disp -- wrong buffers or unprocessed disparity ranges show.  mx = [300, 279], mn = mx 2 / 300: the margins of case
    (2, 49, 2, 128, 300)."""
    lib = L.lib()
    was = lib.falnet_get_deterministic()
    lib.falnet_set_deterministic(1)  # ordered reductions in the backbone: a second forward then gives the same logits bit for bit
    try:
        _render_checks(arch, n)
    finally:
        lib.falnet_set_deterministic(was)


def _render_checks(arch, n):
    from fal_net_amd import synthetic
    B, H, W = 2, 64, 128
    model = _model(arch, n)
    left, _, _, _ = synthetic.synthetic_pair(B, H, W, seed=11)
    left = left.to(DEV)
    mx = torch.tensor([300.0, 279.0], device=DEV).view(B, 1, 1)
    mn = mx * 2 / 300
    ts = S.SETS["B"]
    views, disps, disp = V.render(model, left, mn, mx, ts)
    buf = model._plan(B, H, W, left.device).buf
    inp = {"dlog0": buf["dlog0"].cpu(), "left": left.cpu().float(), "mn": mn.reshape(-1).cpu(), "mx": mx.reshape(-1).cpu()}
    assert torch.equal(buf["left"].cpu(), inp["left"]) and torch.equal(disp, buf["disp"])
    ref = S.reference(inp, ts)
    case = (B, n, H, W, 300.0)
    res = S.compare_views(case, ts, views.cpu(), disps.cpu(), ref)
    for what, v, t, r in res:
        print(f"FAL_net{arch} {what}[{v}] t={t}: coef {r['coef']:.3g} worst ratio {r['worst_ratio']:.3g}")
    assert not [x for x in res if x[3]["bad"]]
    with torch.no_grad():
        fwd = model(left, mn, mx, ret_disp=True, ret_subocc=False, ret_pan=False)
    print(f"FAL_net{arch} returned disp against a second forward: max difference {float((disp - fwd).abs().max()):.3g}")
    assert torch.equal(disp, fwd)
    assert torch.equal(V.right_disparity(model, left, mn, mx), disps[:, ts.index(1.0)])
    if arch == "B":  # the t = 1 view is the forward's own right view, to the head's own bound
        with torch.no_grad():
            pan = model(left, mn, mx, ret_disp=True, ret_subocc=False, ret_pan=True)[0]
        r = R.compare(pan.cpu(), ref["view"][:, ts.index(1.0)], ref["mag_view"][:, ts.index(1.0)], torch.float32, R.coef("p_im0", case))
        assert not r["bad"], r


def _run_cli(tmp, *extra):
    env = dict(os.environ, FALNET_DETERMINISTIC="1")
    cmd = [sys.executable, os.path.join(ROOT, "Test_KITTI.py"), "--synthetic", "--height", "128", "--width", "416", "--iters", "1", "--save-path", str(tmp)] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]


def test_cli_sweep_end_to_end(tmp_path):
    from PIL import Image
    from fal_net_amd import dumps, synthetic
    out = tmp_path / "sweep"
    lines = _run_cli(out, "--sweep", "5")
    assert lines[-2] == {"sweep": {"views": 5, "range": [-1.0, 1.0], "files": 6}}, lines
    assert "sec_per_image_median" in lines[-1]
    files = sorted(glob.glob(str(out / "Sweep" / "*_v0?.png")))
    assert [os.path.basename(f) for f in files] == ["{:010d}_v{:02d}.png".format(0, j) for j in range(5)]
    for f in files:
        assert Image.open(f).size == (416, 128)
    assert [os.path.basename(f) for f in glob.glob(str(out / "r_disp" / "*.png"))] == ["{:010d}.png".format(0)]
    # fraction 0 is view 2 of [-1, -0.5, 0, 0.5, 1]: the left image, up to a rounding tie of the 8-bit conversion
    left, _, _, _ = synthetic.synthetic_pair(1, 128, 416, seed=7)
    want = dumps.image_u8(left.to(DEV))[0].cpu().numpy().astype(np.int16)
    got = np.asarray(Image.open(files[2])).astype(np.int16)
    assert got.shape == want.shape and int(np.abs(got - want).max()) <= 1
    # without --sweep: neither folder, no extra line
    plain = tmp_path / "plain"
    lines = _run_cli(plain)
    assert len(lines) == 1 and "sweep" not in lines[0]
    assert not os.path.exists(plain / "Sweep") and not os.path.exists(plain / "r_disp")
