"""The free-viewpoint plane sweep (csrc/med_pose.hip through the C-ABI, fal_net_amd/freeview.py, Test_KITTI.py --freeview) on the MI355X, element by
element against the float64 reference of tests/_freeview_ref.py:  |got - ref| <= u |ref| + c mag + eta.

Every output buffer is NaN before its launch and sits between two NaN guard zones that must stay NaN: an element the kernel never writes, or
one it writes out of bounds, is a violation.  The coefficients are the measured ones of _freeview_ref.COEF (raw figures:
profiles/freeview_vs_f64.txt)."""
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
from fal_net_amd import freeview as FV  # noqa: E402
from fal_net_amd import views as V  # noqa: E402

import _freeview_ref as F  # noqa: E402
import _head_ref as R  # noqa: E402
import _sweep_ref as S  # noqa: E402

DEV = "cuda"
NAN = float("nan")
GUARD = 1024  # floats of NaN before and behind each output
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHANS = {"view": 3, "disp": 1, "cover": 1}


def raw_pose(dlog0, left, mn, mx, poses, want=("view", "disp", "cover"), n_poses=None, shape=None, null=()):
    """One falnet_med_pose_fwd call on device tensors from NaN-pre-filled outputs, each between two NaN guard zones.  n_poses / shape override
    what the call is told and `null` names inputs passed as NULL (the refusals).  -> (return code, {output: (B, V, C, H, W)} of ALL THREE
    buffers, also those not passed to the library -- their NaNs must then be intact --, guards_intact)."""
    B, _, H, W = dlog0.shape
    rows = max(len(poses), 1)
    nv = len(poses) if n_poses is None else n_poses
    full = {k: torch.full((B * rows * c * H * W + 2 * GUARD,), NAN, dtype=torch.float32, device=DEV) for k, c in CHANS.items()}
    body = {k: full[k][GUARD:-GUARD] for k in CHANS}
    rec = np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64) for p in poses])) if len(poses) else np.zeros((1, 12))
    ins = [L.ptr(None if k in null else t) for k, t in (("dlog0", dlog0), ("left", left), ("mn", mn), ("mx", mx))]
    rc = L.lib().falnet_med_pose_fwd(*ins, rec.ctypes.data_as(ctypes.c_void_p), nv, *[L.ptr(body[k] if k in want else None) for k in ("view", "disp", "cover")],
                                     *(tuple(dlog0.shape) if shape is None else shape), L.stream_ptr())
    torch.cuda.synchronize()
    guards = all(bool(torch.isnan(full[k][:GUARD]).all()) and bool(torch.isnan(full[k][-GUARD:]).all()) for k in CHANS)
    return rc, {k: body[k].view(B, rows, CHANS[k], H, W) for k in CHANS}, guards


def on_device(inp):
    return inp["dlog0"].contiguous().to(DEV), inp["left"].to(DEV), inp["mn"].to(DEV), inp["mx"].to(DEV)


def launches(dev, poses, want=("view", "disp", "cover")):
    """The poses in launches of at most 8 -> ({output: CPU tensor}, every return code 0 and every guard intact)."""
    parts, ok = {k: [] for k in want}, True
    for v0 in range(0, len(poses), 8):
        rc, out, guards = raw_pose(*dev, poses[v0:v0 + 8], want)
        ok = ok and rc == 0 and guards
        for k in want:
            parts[k].append(out[k].cpu())
    return {k: torch.cat(v, 1) for k, v in parts.items()}, ok


def check(case, got, ref, label):
    res = F.compare_outputs(case, got, ref)
    for what, v, r in res:
        print(f"{label} {what}[{v}]: coef {r['coef']:.3g} worst ratio {r['worst_ratio']:.3g} max-norm {r['maxnorm']:.3g}")
    for k, t in got.items():
        assert not bool(torch.isnan(t).any()), f"{label}: NaN left in {k}"
    bad = [(what, v, r) for what, v, r in res if r["bad"]]
    assert not bad, bad


@pytest.mark.parametrize("case,set_name,family", F.listed())
def test_freeview_against_float64(case, set_name, family):
    """View, disparity and cover of every listed (case, pose set, logit family): every element within the bound, no NaN left, guards intact.
    Set N9 goes through two launches (8 + 1)."""
    inp, poses, ref = F.cached(case, set_name, family)
    got, ok = launches(on_device(inp), poses)
    assert ok, L.lib().falnet_last_error()
    check(case, got, ref, f"{case} {set_name} {family}")
    if set_name == "O":  # turned away: nothing is seen
        assert not bool(got["view"].any()) and not bool(got["cover"].any())


def test_freeview_bound_can_fail():
    """The comparator bites on the device's output too: the reference with E_y negated against the kernel's output of pose G."""
    case = F.CASES[1]
    inp, poses, _ = F.cached(case, "G", "a")
    got, ok = launches(on_device(inp), poses)
    assert ok
    for what, v, r in F.compare_outputs(case, got, F.reference(inp, poses, mutate="ey")):
        print(f"mutation {what}: {r['bad']} of {r['n']} over the bound, worst ratio {r['worst_ratio']:.3g}")
        assert r["bad"] > 0, (what, r)


SUBSETS = [("view",), ("disp",), ("cover",), ("view", "disp"), ("view", "cover"), ("disp", "cover"), ("view", "disp", "cover")]


@pytest.mark.parametrize("want", SUBSETS)
def test_freeview_output_subsets(want):
    """Every subset of the outputs: the wanted ones within the bound and bit for bit those of the full launch, the others' NaNs intact."""
    case = F.CASES[1]
    inp, poses, ref = F.cached(case, "F", "a")
    dev = on_device(inp)
    rc, full, guards = raw_pose(*dev, poses)
    assert rc == 0 and guards
    rc, out, guards = raw_pose(*dev, poses, want)
    assert rc == 0 and guards, L.lib().falnet_last_error()
    for k in CHANS:
        if k in want:
            assert torch.equal(out[k], full[k]), k
        else:
            assert bool(torch.isnan(out[k]).all()), k
    check(case, {k: out[k].cpu() for k in want}, ref, f"{case} F {want}")


@pytest.mark.parametrize("case", F.CASES)
def test_identity_gives_left_and_the_forwards_disparity(case):
    inp, poses, ref = F.cached(case, "I", "a")
    got, ok = launches(on_device(inp), poses)
    assert ok
    left64, disp64 = inp["left"].to(torch.float64), S.forward_disp(inp)
    res = [("view=left", R.compare(got["view"][:, 0], left64, ref["mag_view"][:, 0], torch.float32, F.coef("view", case))),
           ("disp=forward", R.compare(got["disp"][:, 0], disp64, disp64, torch.float32, F.coef("disp", case))),
           ("cover=1", R.compare(got["cover"][:, 0], torch.ones_like(disp64), torch.ones_like(disp64), torch.float32, F.coef("cover", case)))]
    for what, r in res:
        print(f"{case} {what}: coef {r['coef']:.3g} worst ratio {r['worst_ratio']:.3g} max-norm {r['maxnorm']:.3g}")
    assert not [x for x in res if x[1]["bad"]], res


@pytest.mark.parametrize("case", [F.CASES[1], F.CASES[4]])
def test_pure_baseline_poses_agree_with_the_sweep(case):
    """Set S against views.sweep with the same fractions on the same buffers: within the SUM of this kernel's bound and the sweep's."""
    ts = (1.0, -0.5, 1.9)
    inp, poses, ref = F.cached(case, "S", "a")
    dev = on_device(inp)
    got, ok = launches(dev, poses, ("view", "disp"))
    assert ok
    sv, sd = V.sweep(*dev, ts)
    sref = S.reference(inp, ts)
    u, eta = R.U[torch.float32], R.ETA[torch.float32]
    for v, t in enumerate(ts):
        for k, mine, theirs in (("view", got["view"][:, v], sv[:, v].cpu()), ("disp", got["disp"][:, v], sd[:, v].cpu())):
            bound = (u * ref[k][:, v].abs() + F.coef(k, case) * ref["mag_" + k][:, v] + eta) + (u * sref[k][:, v].abs() + S.coef(k, case, t) * sref["mag_" + k][:, v] + eta)
            err = (mine.double() - theirs.double()).abs()
            print(f"{case} t={t} {k}: max difference {float(err.max()):.3g}, worst ratio {float((err / bound).max()):.3g}")
            assert bool((err <= bound).all()), (k, t)


def test_wrapper_splits_and_is_deterministic():
    """Nine poses through the wrapper equal the same poses launched singly; two identical calls give the same bits."""
    case = F.CASES[4]
    inp, poses, _ = F.cached(case, "N9", "b")
    dev = on_device(inp)
    out = FV.warp(*dev, poses)
    assert out["view"].shape == (2, 9, 3, 9, 128) and out["disp"].shape == (2, 9, 1, 9, 128) and out["cover"].shape == (2, 9, 1, 9, 128)
    for v, p in enumerate(poses):
        rc, single, guards = raw_pose(*dev, [p])
        assert rc == 0 and guards
        for k in CHANS:
            assert torch.equal(out[k][:, v], single[k][:, 0]), (k, v)
    again = FV.warp(*dev, poses)
    assert all(torch.equal(out[k], again[k]) for k in CHANS)
    only = FV.warp(*dev, poses, want=("cover",))
    assert list(only) == ["cover"] and torch.equal(only["cover"], out["cover"])


def test_freeview_refusals():
    """Non-zero return with every output still NaN and every guard intact."""
    case = F.CASES[1]
    inp, poses, _ = F.cached(case, "G", "a")
    d0, lf, mn, mx = on_device(inp)
    B, N, H, W = d0.shape
    one = [poses[0]]

    def changed(i, val):
        p = poses[0].copy()
        p[i] = val
        return [p]
    flat = poses[0].copy()
    flat[6:9] = 0.0
    trials = {
        "V = 0": dict(poses=one, n_poses=0),
        "V = 9": dict(poses=one * 9, n_poses=9),
        "all outputs null": dict(poses=one, want=()),
        "N = 1": dict(poses=one, shape=(B, 1, H, W)),
        "N = 129": dict(poses=one, shape=(B, 129, H, W)),
        "H = 0": dict(poses=one, shape=(B, N, 0, W)),
        "nan in A": dict(poses=changed(4, NAN)),
        "inf in E": dict(poses=[poses[0]] + changed(10, float("inf"))),
        "third row of A zero": dict(poses=[flat]),
        "null logits": dict(poses=one, null=("dlog0",)),
        "null max_disp": dict(poses=one, null=("mx",)),
        "views without left": dict(poses=one, null=("left",)),
    }
    for name, kw in trials.items():
        # told 129 planes: the call gets the memory for them (it must not touch any of it)
        logits = torch.zeros(B, 129, H, W, device=DEV) if name == "N = 129" else d0
        rc, out, guards = raw_pose(logits, lf, mn, mx, **kw)
        assert rc != 0, name
        assert guards and all(bool(torch.isnan(out[k]).all()) for k in CHANS), name
    assert L.lib().falnet_replay_op_index(b"falnet_med_pose_fwd") == -1


def test_wrapper_refuses_before_any_launch(monkeypatch):
    inp, poses, _ = F.cached(F.CASES[1], "N9", "a")
    dev = on_device(inp)
    calls = []
    real = L.lib().falnet_med_pose_fwd
    monkeypatch.setattr(L.lib(), "falnet_med_pose_fwd", lambda *a: calls.append(a) or real(*a))
    FV.warp(*dev, poses[:1])
    assert len(calls) == 1  # the spy sees launches
    bad = poses[0].copy()
    bad[3] = NAN
    flat = poses[0].copy()
    flat[6:9] = 0.0
    for wrong in (poses[:8] + [bad], poses[:8] + [flat], [], [poses[0][:11]]):  # the refused pose sits in the SECOND launch: the first must not run either
        with pytest.raises(ValueError):
            FV.warp(*dev, wrong)
    with pytest.raises(ValueError):
        FV.warp(*dev, poses, want=())
    with pytest.raises(ValueError):
        FV.warp(*dev, poses, want=("view", "depth"))
    with pytest.raises(ValueError):
        FV.warp(dev[0], dev[1][:, :2], dev[2], dev[3], poses)
    assert len(calls) == 1


def test_render_from_the_models_own_logits():
    """freeview.render on a seeded FAL_netB at (1, 3, 64, 128): equals warp on the plan's own buffers, bit for bit, and returns the forward's disparity."""
    from fal_net_amd import models, synthetic
    B, H, W = 1, 64, 128
    sd = synthetic.seeded_state_dict("B", 49)
    model = models.__dict__["FAL_netB"]({"state_dict": sd}, no_levels=49, compute_dtype=torch.float32).to(DEV).eval()
    left, _, _, _ = synthetic.synthetic_pair(B, H, W, seed=11)
    left = left.to(DEV)
    mx = torch.tensor([300.0], device=DEV).view(B, 1, 1)
    mn = mx * 2 / 300
    K = FV.camera(H, W)
    poses = [FV.pose(K, **kw) for kw in FV.paths.orbit(3, 0.5, 0.25, yaw=3.0)] + [FV.pose(K)]
    out, disp = FV.render(model, left, mn, mx, poses)
    buf = model._plan(B, H, W, left.device).buf  # no second forward: the buffers still hold this one's logits
    assert torch.equal(disp, buf["disp"]) and torch.equal(buf["left"].cpu(), left.cpu().float())
    direct = FV.warp(buf["dlog0"], buf["left"], buf["min_disp"], buf["max_disp"], poses)
    assert all(torch.equal(out[k], direct[k]) for k in CHANS)
    assert out["view"].shape == (B, 4, 3, H, W) and not bool(torch.isnan(out["view"]).any())
    # the identity pose: the left image and the forward's disparity, to the bound of the wide class
    case = (B, 49, H, W, 300.0)
    r = R.compare(out["view"][:, 3].cpu(), left.cpu().double(), left.cpu().double().abs(), torch.float32, F.coef("view", case))
    assert not r["bad"], r
    r = R.compare(out["disp"][:, 3].cpu(), disp.cpu().double(), disp.cpu().double(), torch.float32, F.coef("disp", case))
    assert not r["bad"], r


def test_cli_freeview_end_to_end(tmp_path):
    from PIL import Image
    cmd = [sys.executable, os.path.join(ROOT, "Test_KITTI.py"), "--synthetic", "--freeview", "3", "--height", "64", "--width", "128", "--iters", "1",
           "--save-path", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 2 and "sec_per_image_median" in lines[-1], lines
    fv = lines[0]["freeview"]
    assert fv["frames"] == 1 and fv["poses"] == 3 and fv["files"] == 6 and fv["path"] == "orbit" and fv["camera"] == "nominal", fv
    assert 0.0 < fv["mean_cover"] <= 1.0, fv
    names = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "Freeview" / "*.png")))
    assert names == sorted(["{:010d}_p{:02d}{}.png".format(0, j, s) for j in range(3) for s in ("", "_cover")]), names
    for n in names:
        im = Image.open(tmp_path / "Freeview" / n)
        assert im.size == (128, 64) and im.mode == ("L" if n.endswith("_cover.png") else "RGB"), (n, im.size, im.mode)
