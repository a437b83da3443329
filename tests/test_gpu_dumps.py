"""GPU: the test-time output kernels (csrc/dump.hip through fal_net_amd/dumps.py) against numpy / torch-CPU restatements of the reference
lines they replace (Test_KITTI.py:211-253,303-317, myUtils.py:339-373), at 375 x 1242, 75 x 250 (odd) and B = 2, and Test_KITTI.py --dump end
to end.  Every comparison prints its figure before it asserts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from fal_net_amd import dumps, inference, synthetic  # noqa: E402
from fal_net_amd import myUtils as utils  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MEAN = np.array([0.411, 0.432, 0.45], np.float32)
SIZES = [(1, 375, 1242), (2, 75, 250)]


def seeded_disp(shape):
    return (np.random.default_rng(0).random(shape) ** 3 * 120).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- percentile -------------------------------------------------------------------------------------------------------------------------
def _percentile_cases():
    rng = np.random.default_rng(5)
    return {
        "kitti_375x1242": seeded_disp((1, 375 * 1242)),
        "odd_75x250_b2": np.stack([seeded_disp((75 * 250,)), rng.random(75 * 250).astype(np.float32) * 7 + 1]),
        "constant": np.full((2, 5000), 3.25, np.float32),
        "duplicates": rng.integers(1, 12, (2, 40001)).astype(np.float32),            # few distinct values, n odd
        "negative": (rng.standard_normal((2, 100003)) * 50 - 200).astype(np.float32),  # all order statistics below zero
        "mixed_sign": (rng.standard_normal((1, 70001)) * 50 + 40).astype(np.float32),
        "n_not_a_block_multiple": (rng.random((3, 2049 * 8 + 1)) * 100).astype(np.float32),  # one past a whole number of 8-element threads
        "tiny": np.array([[4.0, -1.0, 2.5]], np.float32),
    }


@pytest.mark.parametrize("name", list(_percentile_cases()))
@pytest.mark.parametrize("q", [0, 50, 95, 100])
def test_percentile_exact(name, q):
    x = _percentile_cases()[name]
    B, n = x.shape
    got, stats = dumps.percentile(torch.from_numpy(x).to(DEV), q, return_order_stats=True)
    again, stats2 = dumps.percentile(torch.from_numpy(x).to(DEV), q, return_order_stats=True)
    got, stats = got.cpu().numpy(), stats.cpu().numpy()
    assert np.array_equal(bits(got), bits(again.cpu().numpy())) and np.array_equal(bits(stats), bits(stats2.cpu().numpy()))  # run to run
    pos = q / 100 * (n - 1)
    lo, hi = int(np.floor(pos)), int(np.ceil(pos))
    for b in range(B):
        part = np.partition(x[b], [lo, hi])
        want = np.percentile(x[b], q)
        err = abs(float(got[b]) - float(want)) / max(abs(float(want)), 1e-30)
        print(f"percentile {name} q={q} b={b}: stats {stats[b]} want [{part[lo]} {part[hi]}]  value {got[b]} want {want} rel {err:.2e}")
        assert bits(stats[b, 0]) == bits(part[lo]) and bits(stats[b, 1]) == bits(part[hi])  # the two order statistics, bit for bit
        assert err <= 1e-6


# ---- plasma -----------------------------------------------------------------------------------------------------------------------------
def plasma_index(disp, p95):
    v = np.float32(256) * np.clip(disp / (np.float32(p95) + np.float32(1e-6)), np.float32(0), np.float32(1))
    return np.minimum(np.rint(v), 255).astype(np.int64)


@pytest.mark.parametrize("tag,shape", [("75x250", (75, 250)), ("375x1242", (375, 1242))])
def test_plasma_vs_matplotlib_golden(tag, shape, golden_dir):
    g = np.load(os.path.join(golden_dir, "dumps_plasma.npz"))
    lut = dumps.plasma_lut()
    disp = seeded_disp(shape)
    d = torch.from_numpy(disp).to(DEV).view(1, 1, *shape)
    p95_dev = dumps.percentile(d, 95)
    out = dumps.disparity_png(d, p95_dev)[0].cpu().numpy()
    # (a) with the device's own p95 fed to the host formula: byte for byte
    p95 = p95_dev.cpu().numpy()[0]
    k_dev = plasma_index(disp, p95)
    assert out.shape == shape + (4,) and np.array_equal(out, lut[k_dev])
    # (b) end to end against the golden (the image plt.imsave wrote; at the large size the table indexed with the golden's p95 -- that the
    # table reproduces imsave is tests/test_dumps_host.py): a pixel may differ by ONE table step, and only where v sits within the percentile
    # margin (1e-6 relative on p95, plus the f32 rounding of the quotient, 2^-23) of a rounding tie; at most 0.1 % of the pixels
    p95_ref = g["p95_" + tag]
    k_ref = plasma_index(disp, p95_ref)
    want = g["rgba_" + tag] if ("rgba_" + tag) in g.files else lut[k_ref]
    differ = (out != want).any(axis=2)
    v = 256 * np.clip(disp.astype(np.float64) / (float(p95_ref) + 1e-6), 0, 1)
    near_tie = np.abs(v - (np.floor(v) + 0.5)) <= v * (1e-6 + 2.0 ** -23)
    print(f"plasma {tag}: p95 device {p95!r} golden {p95_ref!r} rel {abs(float(p95) - float(p95_ref)) / float(p95_ref):.2e}; "
          f"pixels differing {int(differ.sum())} of {differ.size} (host margin count in the golden: {g['margin_' + tag]})")
    assert np.abs(k_dev - k_ref).max() <= 1
    assert not (differ & ~near_tie).any()
    assert differ.mean() <= 1e-3


def test_plasma_batch_uses_each_samples_percentile():
    disp = np.stack([seeded_disp((75, 250)), seeded_disp((75, 250)) * 0.25 + 3])[:, None]
    d = torch.from_numpy(disp).to(DEV)
    out = dumps.disparity_png(d).cpu().numpy()
    p95 = dumps.percentile(d, 95).cpu().numpy()
    lut = dumps.plasma_lut()
    for b in range(2):
        assert np.array_equal(out[b], lut[plasma_index(disp[b, 0], p95[b])])


# ---- 8-bit images -----------------------------------------------------------------------------------------------------------------------
def tie_values():
    """f32 values y with 255 * y == k + 0.5 EXACTLY in f32 (a property of the inputs, found by search): rint must round them half to even."""
    ks = np.arange(0, 255, dtype=np.float32)
    y = ((ks + np.float32(0.5)) / np.float32(255)).astype(np.float32)
    good = y[np.float32(255) * y == ks + np.float32(0.5)]
    assert len(good) >= 16
    return good


@pytest.mark.parametrize("B,H,W", SIZES + [(2, 5, 7)])
def test_image_to_u8_exact(B, H, W):
    rng = np.random.default_rng(21)
    x = (rng.random((B, 3, H, W)) * 3 - 1).astype(np.float32)  # beyond [0, 1]: both saturations act
    for mean in (MEAN, np.zeros(3, np.float32)):
        if not mean.any():
            t = tie_values()[:x.size]
            x.reshape(-1)[:len(t)] = t  # exact .5 ties (mean 0: x + mean is x)
        got = dumps.image_u8(torch.from_numpy(x).to(DEV), mean=tuple(float(m) for m in mean)).cpu().numpy()
        s = np.float32(255) * (x + mean.reshape(1, 3, 1, 1))
        assert s.dtype == np.float32
        want = np.clip(np.rint(s), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)  # saturated where the reference's astype(uint8) wraps
        ties = int((s - np.floor(s) == 0.5).sum())
        print(f"image_to_u8 {B}x{H}x{W} mean {mean}: mismatches {int((got != want).sum())}, ties in the input {ties}, saturated {int((s > 255).sum() + (s < 0).sum())}")
        assert got.shape == (B, H, W, 3) and np.array_equal(got, want)
        assert mean.any() or ties >= 16


@pytest.mark.parametrize("shape", [(1, 1, 375, 1242), (2, 3, 75, 250), (1, 2, 3, 5), (1, 1, 1, 1)])
def test_feature_to_u8_exact(shape):
    rng = np.random.default_rng(22)
    x = (rng.standard_normal(shape) * 0.7).astype(np.float32)  # negative values and |x| > 1
    t = tie_values()[:x.size]
    x.reshape(-1)[:len(t)] = t * np.where(np.arange(len(t)) % 2 == 0, 1, -1).astype(np.float32)
    got = dumps.feature_u8(torch.from_numpy(x).to(DEV)).cpu().numpy()
    feature = np.float32(255) * np.abs(x)
    feature[feature < 0] = 0
    feature[feature > 255] = 255
    want = np.rint(feature).astype(np.uint8)
    print(f"feature_to_u8 {shape}: mismatches {int((got != want).sum())}")
    assert got.shape == shape and np.array_equal(got, want)


# ---- local normalisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SIZES + [(1, 17, 66)])
def test_local_norm_vs_avg_pool(B, H, W):
    g = torch.Generator().manual_seed(31)
    x = torch.rand(B, 3, H, W, generator=g) - 0.43
    out, mu, sigma = dumps.local_normalization(x.to(DEV), return_stats=True)
    out2 = dumps.local_normalization(x.to(DEV))
    assert torch.equal(out, out2)
    out, mu, sigma = out.cpu(), mu.cpu(), sigma.cpu()
    img = x + torch.tensor(MEAN).view(1, 3, 1, 1)  # Test_KITTI.py:303-317 on the CPU
    win_mean = F.avg_pool2d(img, kernel_size=3, stride=1, padding=1)
    win_std = F.avg_pool2d((img - win_mean) ** 2, kernel_size=3, stride=1, padding=1) ** (1 / 2)
    ref = (img - win_mean) / (win_std + 0.0000001)
    e_mu = float(((mu - win_mean).abs() / win_mean.abs()).max())
    e_sigma = float(((sigma - win_std).abs() / win_std.abs()).max())
    # The quotient where sigma > 1e-3.  Its numerator img - mu is a difference of two numbers of size <= 1.1, each carrying up to one f32
    # rounding of its own (2^-24 relative), so it is only known to ~2 * 1.1 * 2^-24 ABSOLUTE; divided by sigma that is the floor under any
    # relative statement about the quotient (the ill-conditioning the two-part comparison exists for).  On top of it: 1e-5 relative.
    ok = win_std > 1e-3
    bound = 1e-5 * ref.abs() + 2 * 1.1 * 2.0 ** -24 / win_std
    excess = float((((out - ref).abs() - bound)[ok]).max())
    print(f"local_norm {B}x{H}x{W}: mu rel {e_mu:.2e} sigma rel {e_sigma:.2e}; quotient: worst (|err| - bound) {excess:.2e} over {int(ok.sum())} of {ok.numel()} pixels, "
          f"max |err| {float((out - ref).abs()[ok].max()):.2e}")
    assert float(win_std.min()) > 1e-3  # a random image has no flat window: every pixel takes part
    assert e_mu <= 1e-5 and e_sigma <= 1e-5
    assert excess <= 0


# ---- point cloud ------------------------------------------------------------------------------------------------------------------------
def point_cloud_numpy(img, disp, focal, baseline):
    """myUtils.py:339-373 restated in f32 numpy, u = j + 0.5 / v = i + 0.5 for the affine_grid (align_corners=False) lines."""
    b, _, h, w = disp.shape
    f32 = np.float32
    z = f32(focal * baseline) / (disp + f32(0.0001))
    u = (np.arange(w, dtype=f32) + f32(0.5)).reshape(1, 1, 1, w)
    v = (np.arange(h, dtype=f32) + f32(0.5)).reshape(1, 1, h, 1)
    x = ((u - f32(w / 2)) / f32(focal)) * z
    y = ((v - f32(h / 2)) / f32(focal)) * z
    z = np.clip(z, 0, 200)
    rgb = (img + MEAN.reshape(1, 3, 1, 1)) * f32(255)
    out = np.concatenate([x, z, -y, rgb], 1).reshape(b, 6, h * w)
    assert out.dtype == f32
    return out


@pytest.mark.parametrize("B,H,W", SIZES)
def test_point_cloud_vs_numpy(B, H, W):
    rng = np.random.default_rng(41)
    img = (rng.random((B, 3, H, W)) * 1.2 - 0.53).astype(np.float32)  # some colours below 0 and above 255
    disp = (rng.random((B, 1, H, W)) * 100).astype(np.float32)
    disp[rng.random(disp.shape) < 0.02] = 0  # z capped at 200 there, x and y from the uncapped z
    focal, baseline = dumps.camera_for_width(W)
    want = point_cloud_numpy(img, disp, focal, baseline)
    ti, td = torch.from_numpy(img).to(DEV), torch.from_numpy(disp).to(DEV)
    got = dumps.point_cloud(ti, td, focal, baseline).cpu().numpy()
    packed = dumps.point_cloud(ti, td, focal, baseline, packed=True).cpu().numpy()
    assert got.shape == (B, 6, H * W) and packed.shape == (B, H * W, 15)
    with np.errstate(divide="ignore", invalid="ignore"):
        relerr = np.where(want[:, :3] == got[:, :3], 0, np.abs(got[:, :3] - want[:, :3]) / np.abs(want[:, :3]))
    zero = disp.reshape(B, -1) == 0
    print(f"point_cloud {B}x{H}x{W}: xyz rel {relerr.max():.2e}, colour mismatches {int((got[:, 3:] != want[:, 3:]).sum())}, disp = 0 vertices {int(zero.sum())}")
    assert relerr.max() <= 1e-6
    assert np.array_equal(got[:, 3:], want[:, 3:])
    assert zero.any() and (got[:, 1][zero] == 200).all() and np.abs(got[:, 0][zero]).max() > 1e4  # capped z, uncapped x
    for b in range(B):
        rec = np.frombuffer(packed[b].tobytes(), dtype=dumps.PLY_VERTEX)
        assert rec.tobytes() == dumps.pack_vertices(got[b]).tobytes()
    assert rec["red"].min() == 0 and rec["red"].max() == 255


def test_get_point_cloud_is_the_kernel():
    g = torch.Generator().manual_seed(43)
    img = (torch.rand(1, 3, 20, 1242, generator=g) - 0.43).to(DEV)
    disp = (torch.rand(1, 1, 20, 1242, generator=g) * 80).to(DEV)
    m = torch.tensor(MEAN, device=DEV).view(1, 3, 1, 1)
    a = utils.get_point_cloud((img + m) * 255, disp)  # how the reference calls it (Test_KITTI.py:224)
    b = dumps.point_cloud(img, disp)
    assert a.is_cuda and a.shape == (1, 6, 20 * 1242) and torch.equal(a, b)
    with pytest.raises(KeyError):
        utils.get_point_cloud(img[..., :320], disp[..., :320])


# ---- ms_pp with the device percentile ---------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def test_ms_pp_device_percentile_vs_host_and_oracle():
    from oracle import falnet_oracle as O
    left, right, mn, mx = synthetic.synthetic_pair(1, 375, 1242, seed=77)
    sd = synthetic.seeded_falnetb_state_dict(49)
    m = FAL_netB({"state_dict": sd}, 49).to(DEV).eval()
    with torch.no_grad():
        disp = m(left.to(DEV), mn.to(DEV), mx.to(DEV))
        host = inference.ms_pp(left.to(DEV), m, disp, mn.to(DEV), mx.to(DEV))
        dev = inference.ms_pp(left.to(DEV), m, disp, mn.to(DEV), mx.to(DEV), device_percentile=True)
        ref_pp = O.ms_pp(sd, left, O.falnet_forward(sd, left, mn, mx), mn, mx)
    print(f"ms_pp device percentile vs host {rel(dev, host):.2e}, vs oracle {rel(dev, ref_pp):.2e} (host vs oracle {rel(host, ref_pp):.2e})")
    assert rel(dev, host) < 2e-4
    assert rel(dev, ref_pp) < 2e-4


# ---- Test_KITTI.py --dump end to end ----------------------------------------------------------------------------------------------------
def _run(argv, cwd, timeout=900):
    env = dict(os.environ, FALNET_DETERMINISTIC="1")  # kernel choices never come from a timing: two runs compute the same numbers
    return subprocess.run([sys.executable, os.path.join(ROOT, "Test_KITTI.py")] + argv, capture_output=True, text=True, timeout=timeout, cwd=cwd, env=env)


def _check_dump_tree(res, H, W, ply_format):
    from PIL import Image
    name = "0000000000"
    for folder, mode, chans in (("l_disp", "RGBA", 4), ("Input im", "RGB", 3), ("Pan", "RGB", 3)):
        im = Image.open(res / folder / (name + ".png"))
        assert im.size == (W, H) and im.mode == mode, (folder, im.size, im.mode)
    feats = sorted(os.listdir(res / "feats"))
    assert feats == [f"{name}_l0_c0.png", f"{name}_l0_c1.png", f"{name}_l0_c2.png", f"{name}_l1_c0.png", f"{name}_l2_c0.png"]
    for f in feats:
        im = Image.open(res / "feats" / f)
        assert im.size == (W, H) and im.mode == "L"
    raw = (res / "Point_cloud" / (name + ".ply")).read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[1] == ("format binary_little_endian 1.0" if ply_format == "binary" else "format ascii 1.0")
    assert lines[2] == f"element vertex {H * W}"
    if ply_format == "binary":
        assert len(body) == 15 * H * W
    else:
        assert body.count(b"\n") == H * W


def test_test_kitti_dump_synthetic(tmp_path):
    base = ["--synthetic", "--height", "96", "--width", "320", "--iters", "1"]
    r = _run(base + ["--dump", "disp,input,pan,pc,feats", "--save-path", str(tmp_path / "res")], ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_dump_tree(tmp_path / "res", 96, 320, "binary")
    r0 = _run(base, str(tmp_path))
    assert r0.returncode == 0, r0.stderr[-3000:]
    a, b = (json.loads([l for l in x.stdout.splitlines() if l.startswith("{")][-1]) for x in (r, r0))
    a.pop("sec_per_image_median"), b.pop("sec_per_image_median")
    assert a == b  # the JSON line of a run without --dump (but for the wall time)
    bad = _run(base + ["--dump", "disp", "-save", "True"], str(tmp_path), timeout=300)
    assert bad.returncode != 0 and "out of scope" in (bad.stderr + bad.stdout)


def test_test_kitti_dump_dataset(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_host_logic import _write_png_fixture
    root, _ = _write_png_fixture(tmp_path, n_train=1, n_val=1)
    base = ["-d", str(root), "-tn", "Kitti2015", "--allow-seeded-weights", "--dtype", "f32", "-w", "1"]
    r = _run(base + ["--save-path", str(tmp_path / "res"), "--dump", "disp,input,pan,pc,feats", "--ply-format", "ascii"], ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_dump_tree(tmp_path / "res", 375, 1242, "ascii")
    r0 = _run(base + ["--save-path", str(tmp_path / "plain")], ROOT)
    assert r0.returncode == 0, r0.stderr[-3000:]
    assert not os.path.exists(tmp_path / "plain" / "l_disp")  # nothing is created without --dump
    assert open(tmp_path / "res" / "errors.txt").read() == open(tmp_path / "plain" / "errors.txt").read()
    a, b = (json.loads([l for l in x.stdout.splitlines() if l.startswith("{")][-1]) for x in (r, r0))
    for o in (a, b):
        o.pop("sec_per_image"), o.pop("errors_txt")
    print("dataset run with --dump:", a)
    assert a == b and a["frames"] == 1 and a["epe"] > 0  # metrics equal to the last digit: dumping does not perturb the evaluation
