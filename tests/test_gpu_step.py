"""GPU parity tests, step level: the Stage-1 / Stage-2 step bodies (model + VGG + losses + backward + fused Adam)
against the golden fixtures recorded from the reference and against the CPU oracle."""
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import synthetic, train  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402
from oracle import falnet_oracle as O  # noqa: E402

from _grad_parity import grad_parity  # noqa: E402

DEV = "cuda"
TOL = 1e-4  # north_star gate (f32 path): loss scalars and disparity maps within 1e-4 relative


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def sample_idx(key, numel, k=16):
    g = np.random.default_rng(zlib.crc32(("idx:" + key).encode()))
    return g.integers(0, numel, size=min(k, numel))


def check_after_adam(after, golden_after, golden_gsamp, gnorm, numel, key, tol=2.5e-5, lr=1e-4):
    """Weights after the FIRST Adam step: the update is lr * g / (|g| + eps) = +-lr for every element whose gradient is not ~0, so
    a sampled element whose gradient lies within run-to-run noise of zero (f32 atomics reorder the split-K sums) can land on the
    other sign: 2*lr away.  Elements with |g| > 1 % of the tensor's RMS gradient are sign-stable and must match tightly; the
    others may differ by at most that flip."""
    d = np.abs(after - golden_after)
    stable = np.abs(golden_gsamp) > 1e-2 * gnorm / np.sqrt(numel)
    assert d[stable].max(initial=0.0) < tol, key
    assert d.max(initial=0.0) < 2 * lr + tol, key


def oracle64(sd, left, right, mn, mx, vsd=None):
    """Float64 leaf parameters, teacher weights, VGG weights and images for an oracle run without f32 summation noise."""
    sd = {k: v.double() for k, v in sd.items()}
    vsd = {k: v.double() for k, v in (vsd or synthetic.seeded_vgg19_state_dict()).items()}
    return O.leaf_params(sd), sd, vsd, left.double(), right.double(), mn.double(), mx.double()


def build(n_levels, dtype=torch.float32):
    LF.set_compute_dtype(dtype)
    m = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(n_levels)}, no_levels=n_levels, compute_dtype=dtype)
    return m.to(DEV)


def test_stage1_step_vs_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g2_stage1_step.npz"))
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=int(g["seed"]), distinct=True)
    m = build(49).train()
    opt = train.FlatAdam(m, lr=1e-4, betas=(0.5, 0.999))
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    out = train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV))
    for k in ("loss", "rec", "sm"):
        assert abs(float(out[k]) - float(g[k])) / abs(float(g[k])) < TOL, (k, float(out[k]), float(g[k]))
    grads = {k: p.grad for k, p in m.named_parameters()}
    for k, p in m.named_parameters():
        if "amask_conv" in k:
            assert ("nograd:" + k) in g.files and p.grad is None
            assert torch.equal(p.detach(), before[k])  # untouched by Adam, like torch's grad-is-None skip
            continue
        gr = grads[k].reshape(-1)
        gn = float(g["gnorm:" + k])
        assert abs(float(gr.norm()) - gn) / gn < 5e-4, k
        idx = sample_idx(k, gr.numel())
        assert np.abs(gr[idx].cpu().numpy() - g["gsamp:" + k]).max() <= 5e-4 * gn + 1e-9, k
        after = p.detach().reshape(-1)[sample_idx(k, p.numel())].cpu().numpy()
        check_after_adam(after, g["after:" + k], g["gsamp:" + k], gn, p.numel(), k)  # first Adam step moves by ~lr=1e-4


def test_stage1_config_shape_vs_golden(golden_dir):
    """256x512, N=49 (BASELINE configs[0]/[1] shape), B=1: disparity map + loss scalars."""
    g = np.load(os.path.join(golden_dir, "g4_config_256x512.npz"))
    left, right, mn, mx = synthetic.synthetic_pair(1, 256, 512, seed=int(g["seed"]))
    m = build(49).train()
    opt = train.FlatAdam(m)
    out = train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV))
    for k in ("loss", "rec", "sm"):
        assert abs(float(out[k]) - float(g[k])) / abs(float(g[k])) < TOL, (k, float(out[k]), float(g[k]))
    assert rel(out["ldisp"][:, :, ::8, ::8], g["disp"]) < TOL
    assert rel(out["rpan"][:, :, ::8, ::8], g["p_im0"]) < 2e-4
    for k, p in m.named_parameters():
        if ("gnorm:" + k) in g.files:
            gn = float(g["gnorm:" + k])
            assert abs(float(p.grad.norm()) - gn) / gn < 2e-3, k
    # the golden stores gradient norms only: every gradient element-wise against the float64 oracle on the same inputs
    p64, _, vsd64, *x64 = oracle64(synthetic.seeded_falnetb_state_dict(49), left, right, mn, mx)
    O.stage1_losses(p64, vsd64, *x64)["loss"].backward()
    grad_parity({k: p.grad for k, p in m.named_parameters() if p.grad is not None}, {k: p.grad for k, p in p64.items() if p.grad is not None},
                norm_tol=2e-3, what="Stage-1 B=1 256x512 (g4 inputs)")
    # abs_rel of depth (myUtils.py:225 style) between HIP and reference disparities
    d_ref, d_hip = 721.5377 * 0.54 / g["disp"], 721.5377 * 0.54 / out["ldisp"].detach()[:, :, ::8, ::8].cpu().numpy()
    assert float(np.mean(np.abs(d_ref - d_hip) / d_ref)) < 1e-5


def test_losses_vs_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g6_losses_metrics.npz"))
    LF.set_compute_dtype(torch.float32)
    img, dsp = torch.from_numpy(g["img"]).to(DEV), torch.from_numpy(g["dsp"]).to(DEV).requires_grad_(True)
    assert abs(float(LF.smoothness(img, dsp, 1)) - float(g["sm_g1"])) < 1e-5 * float(g["sm_g1"])
    sm2 = LF.smoothness(img, dsp, 2)
    assert abs(float(sm2) - float(g["sm_g2"])) < 1e-5 * float(g["sm_g2"])
    sm2.backward()
    assert rel(dsp.grad, g["sm_g2_grad"]) < 1e-5
    synth = torch.from_numpy(g["synth"]).to(DEV).requires_grad_(True)
    label, mask = torch.from_numpy(g["label"]).to(DEV), torch.from_numpy(g["mask"]).to(DEV)
    vl = LF.vgg(label)
    assert np.allclose([float(v.float().mean()) for v in vl], g["vgg_label_means"], rtol=1e-4)
    r = LF.rec_loss_fnc(mask, synth, label, vl, 0.01)
    assert abs(float(r) - float(g["rec_masked"])) < TOL * float(g["rec_masked"])
    r.backward()
    assert rel(synth.grad, g["rec_masked_grad"]) < 2e-4
    assert abs(float(LF.rec_loss_fnc(1, synth.detach(), label, vl, 0.01)) - float(g["rec_one"])) < TOL * float(g["rec_one"])
    assert abs(float(LF.rec_loss_fnc(mask, synth.detach(), label, None, 0.0)) - float(g["rec_l1"])) < TOL * float(g["rec_l1"])


def test_smoothness_column_window():
    """The callers crop columns before the loss (Train_Stage1_K.py:255); the windowed kernel must equal the
    loss on materialised crops, incl. gradients landing in the uncropped parent."""
    gen = torch.Generator().manual_seed(5)
    img = (torch.rand(2, 3, 16, 64, generator=gen) - 0.43).to(DEV)
    dsp = (torch.rand(2, 1, 16, 64, generator=gen) * 40).to(DEV).requires_grad_(True)
    a = LF.smoothness(img[:, :, :, 12:], dsp[:, :, :, 12:], gamma=2)
    a.backward()
    ga = dsp.grad.clone()
    dsp.grad = None
    ref = O.smoothness(img.cpu()[:, :, :, 12:], dsp.detach().cpu().requires_grad_(True)[:, :, :, 12:], gamma=2)
    assert abs(float(a) - float(ref)) < 1e-5 * float(ref)
    assert float(ga[:, :, :, :12].abs().max()) == 0.0
    b = LF.smoothness(img[:, :, :, 12:].contiguous(), dsp[:, :, :, 12:].contiguous(), gamma=2)
    b.backward()
    assert rel(dsp.grad, ga) < 1e-6


def test_stage2_step_vs_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "g3_stage2_step.npz"))
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=int(g["seed"]), distinct=True)
    m, fix = build(7).train(), build(7).eval()
    opt = train.FlatAdam(m, lr=5e-5)
    out = train.stage2_step(m, fix, opt, left.to(DEV), right.to(DEV), mx.to(DEV))
    for k in ("loss", "rec", "sm", "mirror"):
        assert abs(float(out[k]) - float(g[k])) / abs(float(g[k])) < TOL, (k, float(out[k]), float(g[k]))
    for k in ("ldisp", "rdisp"):
        assert rel(out[k], g[k]) < TOL, k
    for k in ("O_L", "O_R"):
        assert rel(out[k], g[k]) < 2e-4, k
    for k, p in m.named_parameters():
        if ("gnorm:" + k) in g.files:
            gn = float(g["gnorm:" + k])
            assert abs(float(p.grad.norm()) - gn) / gn < 1e-3, k
    # the golden stores gradient norms only: every gradient element-wise against the float64 oracle on the same inputs
    p64, sd64, vsd64, *x64 = oracle64(synthetic.seeded_falnetb_state_dict(7), left, right, mn, mx)
    O.stage2_losses(p64, sd64, vsd64, *x64)["loss"].backward()
    grad_parity({k: p.grad for k, p in m.named_parameters() if p.grad is not None}, {k: p.grad for k, p in p64.items() if p.grad is not None},
                norm_tol=1e-3, what="Stage-2 B=2 64x128 (g3 inputs)")


def test_stage1_slow_step_vs_golden(golden_dir):
    """Two-view Stage-1 variant (Train_Stage1_Kslow.py:236-284) against the reference-made golden: losses, both
    disparities, both synthesised views, gradients and the weights after Adam."""
    g = np.load(os.path.join(golden_dir, "g9_stage1_slow_step.npz"))
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=int(g["seed"]), distinct=True)
    m = build(49).train()
    opt = train.FlatAdam(m)
    out = train.stage1_slow_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV))
    for k in ("loss", "rec", "sm"):
        assert abs(float(out[k]) - float(g[k])) / abs(float(g[k])) < TOL, (k, float(out[k]), float(g[k]))
    for k in ("ldisp", "rdisp"):
        assert rel(out[k], g[k]) < TOL, k
    for k in ("rpan", "lpan"):
        assert rel(out[k][:, :, ::2, ::2], g[k]) < 2e-4, k
    for k, p in m.named_parameters():
        if ("gnorm:" + k) not in g.files:
            continue
        gn = float(g["gnorm:" + k])
        gr = p.grad.reshape(-1)
        assert abs(float(gr.norm()) - gn) / gn < 1e-3, k
        assert np.abs(gr[sample_idx(k, gr.numel())].cpu().numpy() - g["gsamp:" + k]).max() <= 1e-3 * gn + 1e-9, k
        after = p.detach().reshape(-1)[sample_idx(k, p.numel())].cpu().numpy()
        check_after_adam(after, g["after:" + k], g["gsamp:" + k], gn, p.numel(), k)


@pytest.mark.parametrize("arch", ["A", "C"])
def test_falnet_variants_vs_golden(golden_dir, arch):
    """FAL_netA (3x1 / 1x3 residual convs, `BackBone.` keys, maskR with align_corners=False) and FAL_netC (wider bottleneck,
    `synth.` keys) on the shared launch plan, against goldens recorded from models/FAL_netA.py / FAL_netC.py: forward with
    masks, then one Stage-1 step (losses, every gradient, weights after Adam)."""
    from fal_net_amd import models as M
    g = np.load(os.path.join(golden_dir, f"g10_falnet{arch}.npz"))
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=int(g["seed"]), distinct=True)
    LF.set_compute_dtype(torch.float32)
    sd = synthetic.seeded_state_dict(arch, 33)
    m = getattr(M, "FAL_net" + arch)({"state_dict": sd}, no_levels=33, compute_dtype=torch.float32).to(DEV)
    assert list(m.state_dict().keys()) == list(sd.keys())  # the reference's checkpoint layout, in its order
    with torch.no_grad():
        pan, disp, maskL, maskR = m.eval()(left.to(DEV), mn.to(DEV), mx.to(DEV), ret_disp=True, ret_subocc=True, ret_pan=True)
    assert rel(disp, g["disp"]) < TOL
    assert rel(pan[:, :, ::2, ::2], g["p_im0"]) < 2e-4
    assert rel(maskL, g["maskL"]) < 2e-4
    assert rel(maskR, g["maskR"]) < 2e-4
    m.train()
    opt = train.FlatAdam(m, lr=1e-4, betas=(0.5, 0.999))
    out = train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV))
    for k in ("loss", "rec", "sm"):
        assert abs(float(out[k]) - float(g[k])) / abs(float(g[k])) < TOL, (k, float(out[k]), float(g[k]))
    for k, p in m.named_parameters():
        if ("nograd:" + k) in g.files:
            assert p.grad is None
            continue
        gr, gn = p.grad.reshape(-1), float(g["gnorm:" + k])
        assert abs(float(gr.norm()) - gn) / gn < 5e-4, k
        assert np.abs(gr[sample_idx(k, gr.numel())].cpu().numpy() - g["gsamp:" + k]).max() <= 5e-4 * gn + 1e-9, k
        after = p.detach().reshape(-1)[sample_idx(k, p.numel())].cpu().numpy()
        check_after_adam(after, g["after:" + k], g["gsamp:" + k], gn, p.numel(), k)


@pytest.mark.parametrize("arch", ["A", "C"])
def test_falnet_variants_bf16_step_runs(arch):
    """bf16 throughput path of the variants: runs, finite, loss close to the f32 path's."""
    from fal_net_amd import models as M
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=7, distinct=True)
    losses = {}
    for dt in (torch.float32, torch.bfloat16):
        LF.set_compute_dtype(dt)
        m = getattr(M, "FAL_net" + arch)({"state_dict": synthetic.seeded_state_dict(arch, 33)}, no_levels=33, compute_dtype=dt).to(DEV).train()
        out = train.stage1_step(m, train.FlatAdam(m), left.to(DEV), right.to(DEV), mx.to(DEV))
        losses[dt] = float(out["loss"])
        assert torch.isfinite(m.flat_gradients()).all()
    LF.set_compute_dtype(torch.float32)
    assert abs(losses[torch.bfloat16] - losses[torch.float32]) / losses[torch.float32] < 3e-2, losses


def test_stage2_step_falnetA_vs_oracle():
    """Stage-2 step with FAL_netA: its right occlusion mask (align_corners=False sampling, FAL_netA.py:264) feeds O_R, the masked
    reconstruction and the mirror loss.  Checked against the oracle (pinned for FAL_netA's masks by g10, for the Stage-2 body by g3)."""
    from fal_net_amd import models as M
    LF.set_compute_dtype(torch.float32)
    sd = synthetic.seeded_state_dict("A", 7)
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=33, distinct=True)
    m = M.FAL_netA({"state_dict": sd}, no_levels=7, compute_dtype=torch.float32).to(DEV).train()
    fix = M.FAL_netA({"state_dict": sd}, no_levels=7, compute_dtype=torch.float32).to(DEV).eval()
    out = train.stage2_step(m, fix, train.FlatAdam(m, lr=5e-5), left.to(DEV), right.to(DEV), mx.to(DEV))
    params = O.leaf_params(sd)
    ref = O.stage2_losses(params, sd, synthetic.seeded_vgg19_state_dict(), left, right, mn, mx)
    for k in ("loss", "rec", "sm", "mirror"):
        assert abs(float(out[k]) - float(ref[k])) / abs(float(ref[k])) < TOL, (k, float(out[k]), float(ref[k]))
    for k in ("O_L", "O_R"):
        assert rel(out[k], ref[k]) < 2e-4, k
    ref["loss"].backward()
    for k, p in m.named_parameters():
        gn = float(params[k].grad.norm())
        assert abs(float(p.grad.norm()) - gn) / gn < 1e-3, k
    # element-wise against the float64 oracle
    p64, sd64, vsd64, *x64 = oracle64(sd, left, right, mn, mx)
    O.stage2_losses(p64, sd64, vsd64, *x64)["loss"].backward()
    grad_parity({k: p.grad for k, p in m.named_parameters() if p.grad is not None}, {k: p.grad for k, p in p64.items() if p.grad is not None},
                norm_tol=1e-3, what="Stage-2 FAL_netA 64x128")


def test_16bit_steps_run_and_track_f32():
    """bf16 / f16 throughput paths: same step, deviation reported (no 1e-4 gate; the reference is f32-only).  f16 carries three
    more significant bits than bf16 and must land correspondingly closer to the f32 step."""
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=21, distinct=True)
    res = {}
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        m = build(49, dt).train()
        opt = train.FlatAdam(m)
        out = train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV))
        res[dt] = (float(out["loss"]), out["ldisp"].clone(), m.flat_gradients().clone())
    LF.set_compute_dtype(torch.float32)
    l32, d32, g32 = res[torch.float32]
    dev = {}
    for dt in (torch.bfloat16, torch.float16):
        l16, d16, g16 = res[dt]
        dev[dt] = (abs(l16 - l32) / l32, rel(d16, d32), float(torch.nn.functional.cosine_similarity(g16, g32, dim=0)))
        print(dt, "vs f32: loss rel", dev[dt][0], "disp rel", dev[dt][1], "grad cos", dev[dt][2])
        assert dev[dt][0] < 2e-2 and dev[dt][2] > 0.98
    assert dev[torch.float16][1] < dev[torch.bfloat16][1] and dev[torch.float16][1] < 1e-2


def test_collective_path_world1(tmp_path):
    """The N>1 code path on one GPU: RCCL process group of size 1, bucketed asynchronous all-reduce behind backward,
    1/world folded into Adam -- the step must reproduce the single-process result.  bench.py's last timed step starts from the seeded
    state in both runs, so what it computes THROUGH the collective is compared (its --dump-outputs): the all-reduced gradients and the
    weights after Adam, besides the losses and forward outputs -- to the reordering of f32 atomics, and Adam's +-lr on sign-unstable
    near-zero gradients (the tolerances of test_overlapped_allreduce_equals_single_allreduce_world1)."""
    import subprocess, sys, json
    env = dict(os.environ, FALNET_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29517", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    outs, dumps = [], []
    for name, e in (("dist", env), ("single", dict(os.environ))):
        d = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "2", "--height", "64",
                            "--width", "128", "--no-cpu-baseline", "--no-roofline", "--dtype", "f32", "--dump-outputs", str(d)],
                           capture_output=True, text=True, env=e, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
        assert r.stdout.strip().splitlines()[-1] == line  # the JSON is the last line even with RCCL's banner
        outs.append(json.loads(line)["config"]["final_loss"])
        dumps.append({f.name: np.load(f).astype(np.float64) for f in sorted(d.iterdir())})
    assert abs(outs[0] - outs[1]) < 1e-5 * abs(outs[1]), outs
    a, b = dumps
    assert a.keys() == b.keys() and {"gradients.npy", "parameters.npy"} <= set(a)
    for k in ("loss.npy", "rec.npy", "sm.npy"):
        assert rel(a[k], b[k]) < 1e-5, k
    for k in ("ldisp.npy", "rpan.npy"):
        assert rel(a[k], b[k]) < TOL, k
    assert rel(a["gradients.npy"], b["gradients.npy"]) < 2e-3
    dp = np.abs(a["parameters.npy"] - b["parameters.npy"])
    assert dp.max() <= 2.1e-4 and np.mean(dp > 1e-6) < 0.05  # one Adam step of lr = 1e-4: at most a flipped +-lr, on few elements


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain `bench.py` run (no --full) times exactly --steps steps and reports them without any leg of --full; `--dump-outputs` writes what
    the last timed step computed as float32 .npy files within 64 MB, its loss the line's final_loss.  Same arguments, same inputs: two runs in
    deterministic mode dump identical arrays."""
    import subprocess, sys, json
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = dict(os.environ, FALNET_DETERMINISTIC="1")
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"dump{i}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                            "--height", "64", "--width", "128", "--dtype", "f32", "--dump-outputs", str(d)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
        dumps.append({f.name: np.load(f) for f in sorted(d.iterdir())})
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64e6
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    for leg in ("roofline", "cpu_baseline", "abs_rel_vs_ref", "abs_rel_vs_gt", "allreduce", "kernel_breakdown_ms_per_step"):
        assert leg not in line, leg
    a, b = dumps
    assert {"loss.npy", "ldisp.npy", "rpan.npy", "parameters.npy", "gradients.npy"} <= set(a) and a.keys() == b.keys()
    assert all(v.dtype == np.float32 for v in a.values())
    assert abs(float(a["loss.npy"]) - line["config"]["final_loss"]) <= 1e-6 * abs(line["config"]["final_loss"])
    assert a["ldisp.npy"].shape == (2, 1, 64, 128) and np.isfinite(a["ldisp.npy"]).all()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _bench_dump(tmp_path, name, args, env=None, small=True):
    import subprocess, sys, json
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    d = tmp_path / name
    size = ["--batch", "2", "--height", "64", "--width", "128"] if small else []
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + size + ["--dump-outputs", str(d)] + args,
                       capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), {f.name: np.load(f) for f in sorted(d.iterdir())}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_bench_last_step_starts_from_seeded_state(dtype, tmp_path):
    """The last timed step of bench.py starts from the seeded starting state again (bench.StartState: weights and their packed copies, Adam
    moments, step count, f16 loss scale): in deterministic mode its outputs after warm-up and earlier timed steps are bit-identical to those
    of a run whose only step is the first one."""
    det = {"FALNET_DETERMINISTIC": "1"}
    line_r, restored = _bench_dump(tmp_path, "restored", ["--steps", "4", "--warmup", "2", "--dtype", dtype], det)
    line_f, first = _bench_dump(tmp_path, "first", ["--steps", "1", "--warmup", "0", "--dtype", dtype], det)
    assert line_r["steps"] == 4 and line_f["steps"] == 1
    assert restored.keys() == first.keys()
    for k in restored:
        assert np.array_equal(restored[k], first[k]), k


def test_bench_dumps_repeat_in_default_mode(tmp_path):
    """Two runs of the same plain bench.py arguments at the benchmark's own configuration (its kernel choices replayed from the committed
    autotune cache), default (non-deterministic) mode: the f32 atomics of the step round differently in every run, but the last step computes
    from the same inputs, so its outputs agree up to that rounding -- the forward outputs and losses to 1e-3, the gradients to 1e-2 of their
    largest element, the weights after Adam's first step to the +-lr of a sign flip of a gradient that rounds across zero, on few elements.
    (Without the restore the losses of two runs differ by several per cent and nearly every weight differs.)"""
    args = ["--steps", "12", "--warmup", "3"]
    (la, a), (lb, b) = _bench_dump(tmp_path, "a", args, small=False), _bench_dump(tmp_path, "b", args, small=False)
    assert a.keys() == b.keys()
    rel = lambda x, y: float(np.abs(x.astype(np.float64) - y).max() / max(np.abs(y).max(), 1e-30))
    for k in ("loss.npy", "rec.npy", "sm.npy", "ldisp.npy", "rpan.npy"):
        assert rel(a[k], b[k]) < 1e-3, k
    assert abs(la["config"]["final_loss"] - lb["config"]["final_loss"]) < 1e-3 * abs(lb["config"]["final_loss"])
    assert rel(a["gradients.npy"], b["gradients.npy"]) < 1e-2
    dp = np.abs(a["parameters.npy"].astype(np.float64) - b["parameters.npy"])
    assert dp.max() <= 2e-4 + 1e-6 and np.mean(dp > 1e-6) < 0.1


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_highres_n96_step_properties(dt):
    """BASELINE configs[4] (384x1280, N=96, fp16; B=2 here) and the same shape in bf16: size-independent properties -- finite
    loss that decreases over a few Adam steps, disparities inside [min_disp, max_disp], synthesised view a convex blend."""
    left, right, mn, mx = synthetic.synthetic_pair(2, 384, 1280, seed=5)
    m = build(96, dt).train()
    opt = train.FlatAdam(m, lr=1e-4)
    losses = []
    for _ in range(4):
        out = train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV))
        losses.append(float(out["loss"]))
    LF.set_compute_dtype(torch.float32)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    d = out["ldisp"]
    assert float(d.min()) >= 2.0 - 1e-2 and float(d.max()) <= 300.0 + 1e-2
    assert float(out["rpan"].abs().max()) <= float(left.abs().max()) + 1e-3


def test_pack_after_optimizer_tracks_weight_changes(monkeypatch):
    """FlatAdam re-packs the compute-dtype weight copies right behind its update and the next forward skips its own re-pack;
    an in-place change of the parameters by anybody else (version counters) must still trigger one.  Same losses either way."""
    LF.set_compute_dtype(torch.float32)
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=5)
    left, right, mx = left.to(DEV), right.to(DEV), mx.to(DEV)

    def run(flag):
        monkeypatch.setenv("FALNET_AB", "1")  # experiment switches are honoured only with FALNET_AB=1
        monkeypatch.setenv("FALNET_PACK_AFTER_ADAM", flag)
        m = build(7).train()
        opt = train.FlatAdam(m, lr=1e-3, betas=(0.5, 0.999))
        losses = []
        for i in range(4):
            losses.append(float(train.stage1_step(m, opt, left, right, mx)["loss"]))
            if i == 1:
                with torch.no_grad():
                    for p in m.parameters():
                        p.mul_(0.999)
        return losses
    a, b = run("0"), run("1")
    assert a[2] != a[1]
    for i, (x, y) in enumerate(zip(a, b)):
        # steps 0-2 (2 = right after the external change) agree to rounding; later ones only to what Adam's normalisation of
        # near-zero gradients leaves of it (the two instances autotune independently: different summation orders)
        assert abs(x - y) < (1e-5 if i < 3 else 2e-3) * abs(x), (a, b)


def test_reduced_precision_trains_like_f32():
    """400 Stage-1 steps on STRUCTURED synthetic stereo (synthetic.structured_stereo: the right view is the left one displaced by a smooth
    known disparity, so the self-supervised loss has a defined minimum and ground truth exists), from the same seeded weights, in f32, bf16
    and f16 (tools/trajectory.py; the 600-step run and the deterministic control are in profiles/r04_trajectory_*.json).  The f32 path must
    LEARN the disparity (depth abs_rel against ground truth 0.70 at the seeded weights -> < 0.12), and each 16-bit path must reach
    <= 1.5 x the f32 value: a broken 16-bit kernel does not train to ground truth (round 3's bounds on noise images could not tell)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("trajectory", os.path.join(os.path.dirname(__file__), "..", "tools", "trajectory.py"))
    traj = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(traj)
    r = traj.run(steps=400, height=128, width=256, batch=4, pool=8, levels=49, dtypes=("f32", "bf16", "f16"))
    print(r)
    f32 = r["f32"]
    assert f32["finite"] and f32["loss_last"] < 0.6 * f32["loss_first"]
    assert f32["abs_rel_vs_gt_start"] > 0.4 and f32["abs_rel_vs_gt"] < 0.12, f32
    for k in ("bf16", "f16"):
        assert r[k]["finite"] and r[k]["loss_last"] < 0.6 * r[k]["loss_first"], (k, r[k])
        # (ten runs of this configuration, round 4: every dtype 0.024-0.035 at 400 steps; a path that does not train stays above 0.1)
        assert r[k]["abs_rel_vs_gt"] <= 1.5 * f32["abs_rel_vs_gt"] + 0.01, (k, r[k]["abs_rel_vs_gt"], f32["abs_rel_vs_gt"])
        assert r[k]["abs_rel_vs_gt_heldout"] <= 1.5 * f32["abs_rel_vs_gt_heldout"] + 0.01, (k, r[k], f32)


def test_deterministic_f32_trajectories_are_identical():
    """The control of the trajectory evidence: two fresh processes with FALNET_DETERMINISTIC=1 train bit-identical models (distance 0)."""
    import json
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(__file__), "..")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "trajectory.py"), "--control", "--steps", "40", "--height", "64", "--width", "128",
                        "--batch", "2", "--pool", "4"], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["bit_identical"] and out["disp_max_abs_diff"] == 0.0, out


def test_stage2_step_256x512_vs_oracle():
    """Stage-2 step at the benchmark resolution (BASELINE configs[3]: 256 x 512, N = 49; B = 2 here, f32) against the CPU oracle:
    loss scalars, both occlusion masks and every parameter's gradient -- norm and element-wise (grad_parity) against the float64 oracle
    (the 64 x 128 case is pinned by golden G3)."""
    LF.set_compute_dtype(torch.float32)
    sd = synthetic.seeded_falnetb_state_dict(49)
    left, right, mn, mx = synthetic.synthetic_pair(2, 256, 512, seed=41, distinct=True)
    m, fix = build(49).train(), build(49).eval()
    out = train.stage2_step(m, fix, train.FlatAdam(m, lr=5e-5), left.to(DEV), right.to(DEV), mx.to(DEV))
    params, sd64, vsd64, *x64 = oracle64(sd, left, right, mn, mx)  # float64: the f32 oracle's own sums over 131k pixels needed 1e-3 here
    ref = O.stage2_losses(params, sd64, vsd64, *x64)
    for k in ("loss", "rec", "sm", "mirror"):
        assert abs(float(out[k]) - float(ref[k])) / abs(float(ref[k])) < TOL, (k, float(out[k]), float(ref[k]))
    for k in ("O_L", "O_R"):
        assert rel(out[k], ref[k]) < 2e-4, k
    ref["loss"].backward()
    for k, p in m.named_parameters():
        if params[k].grad is None:
            continue
        gn = float(params[k].grad.norm())
        assert abs(float(p.grad.norm()) - gn) / gn < 2e-3, (k, float(p.grad.norm()), gn)
    grad_parity({k: p.grad for k, p in m.named_parameters() if params[k].grad is not None},
                {k: p.grad for k, p in params.items() if p.grad is not None}, norm_tol=2e-3, what="Stage-2 B=2 256x512")


def test_vgg_plans_are_released_and_shared_feature_gradients_sum():
    """A grad-enabled vgg() whose graph is dropped without a backward gives its plan back (no HBM growth), and two perceptual
    losses on the SAME feature maps backpropagate their sum (not twice the last one)."""
    import gc
    LF.set_compute_dtype(torch.float32)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 3, 64, 128, generator=g).to(DEV).requires_grad_(True)
    label = LF.vgg(torch.rand(1, 3, 64, 128, generator=g).to(DEV))
    label2 = tuple(2 * v for v in label)
    for _ in range(12):
        feats = LF.vgg(x)  # never backpropagated
        del feats
        gc.collect()
    pool = LF.vgg._plans[(1, 64, 128, True)]
    assert len(pool) == 1 and not pool[0].busy
    held = [LF.vgg(x) for _ in range(7)]  # alive at once: the pool is capped, the oldest plans are recycled
    assert len(pool) <= LF._MAX_HELD_PLANS
    with pytest.raises(RuntimeError, match="recycled"):
        LF.perceptual_loss(held[0], label).backward()
    del held
    gc.collect()

    def grad_of(fn):
        x.grad = None
        fn(LF.vgg(x)).backward()
        return x.grad.clone()

    ga = grad_of(lambda f: LF.perceptual_loss(f, label))
    gb = grad_of(lambda f: LF.perceptual_loss(f, label2))
    gab = grad_of(lambda f: LF.perceptual_loss(f, label) + LF.perceptual_loss(f, label2))
    assert rel(gab, ga + gb) < 1e-5


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_fused_step_matches_autograd_step(dt):
    """train.stage1_step's static launch sequence (no autograd graph) against its autograd form: same losses, outputs and
    parameter gradients (f32: to reordering of the f32 atomics; bf16: to a flipped rounding)."""
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=11, distinct=True)
    left, right, mx = left.to(DEV), right.to(DEV), mx.to(DEV)
    res = {}
    for fused in (False, True):
        m = build(49, dt).train()
        opt = train.FlatAdam(m, lr=1e-4)
        old = train._FUSED_STEP
        train._FUSED_STEP = fused
        try:
            out = train.stage1_step(m, opt, left, right, mx, optimize=False)
        finally:
            train._FUSED_STEP = old
        res[fused] = (float(out["loss"]), float(out["rec"]), float(out["sm"]), out["ldisp"].clone(), out["rpan"].clone(),
                      m.flat_gradients().clone())
    a, f = res[False], res[True]
    tol = 1e-5 if dt == torch.float32 else 2e-3
    for i in range(3):
        assert abs(a[i] - f[i]) <= tol * abs(a[i]), i
    # two module instances may autotune to different kernels / split-K factors: bf16 activations then round differently
    # (same spread as two autograd-form instances, test_16bit_steps_run_and_track_f32)
    otol = 1e-5 if dt == torch.float32 else 6e-2
    assert rel(f[3], a[3]) < otol and rel(f[4], a[4]) < otol
    ga, gf = a[5].double(), f[5].double()
    if dt == torch.float32:
        assert float((ga - gf).norm() / ga.norm()) < 1e-4
    else:
        assert float(torch.nn.functional.cosine_similarity(ga, gf, dim=0)) > 0.999
    LF.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("fused", [True, False])
def test_f16_overflow_skips_the_step_and_backs_the_scale_off(fused):
    """f16 path with a loss scale far too large: activation gradients overflow IEEE half -> inf / NaN in the flat f32 gradient.
    The device-side guard must skip the whole Adam update (weights, moments and step count untouched), halve the scale, and the
    run must recover once the scale fits; a clean step must move the weights and leave the scale alone.  No host sync in the step."""
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=3, distinct=True)
    left, right, mx = left.to(DEV), right.to(DEV), mx.to(DEV)
    m = build(49, torch.float16).train()
    opt = train.FlatAdam(m, lr=1e-4)
    old = train._FUSED_STEP
    train._FUSED_STEP = fused
    try:
        out = train.stage1_step(m, opt, left, right, mx)  # clean step at the default scale
        sc = out["scaler"]
        assert sc is not None and sc.check() == (8192.0, 0)
        w0, t0 = m.flat_parameters().clone(), float(opt.state[1])
        m0 = opt.m.clone()
        sc.state[0] = 2.0 ** 40  # forces an overflow in backward
        train.stage1_step(m, opt, left, right, mx)
        assert not torch.isfinite(m.flat_gradients()).all()
        assert torch.equal(m.flat_parameters(), w0) and torch.equal(opt.m, m0) and float(opt.state[1]) == t0
        scale, skipped = sc.check()
        assert scale == 2.0 ** 39 and skipped == 1
        sc.state[0] = 8192.0
        train.stage1_step(m, opt, left, right, mx)
        assert torch.isfinite(m.flat_gradients()).all() and not torch.equal(m.flat_parameters(), w0) and float(opt.state[1]) == t0 + 1
        assert sc.check() == (8192.0, 1)
        # growth: after `interval` clean steps the scale doubles
        sc.interval = 2
        train.stage1_step(m, opt, left, right, mx)
        assert sc.check()[0] == 8192.0 * 2 or sc.check()[0] == 8192.0  # (one or two clean steps since the last change)
        train.stage1_step(m, opt, left, right, mx)
        assert sc.check()[0] >= 8192.0 * 2
        # a back-off that merely ARRIVES at the floor is not a diverged run: no step has been tried at that scale yet
        sc.state[0], sc.min_scale, sc.max_scale = 2.0 ** 41, 2.0 ** 40, 2.0 ** 42
        train.stage1_step(m, opt, left, right, mx)
        assert sc.check()[0] == 2.0 ** 40
        assert train.LossScaler(DEV).state_dict()["state"][0] == 8192.0  # (checkpointable: Train_Stage1_K.py saves / restores it)
        # a scale at its floor that still overflows is a diverged run: check() raises
        sc.state[0], sc.min_scale, sc.max_scale = 2.0 ** 40, 2.0 ** 40, 2.0 ** 41
        train.stage1_step(m, opt, left, right, mx)
        with pytest.raises(FloatingPointError):
            sc.check()
    finally:
        train._FUSED_STEP = old
        LF.set_compute_dtype(torch.float32)


def test_overlapped_allreduce_equals_single_allreduce_world1():
    """The bucketed asynchronous all-reduce (hook fired from the weight-gradient side stream while backward continues) against
    `_no_overlap` (one all-reduce of the whole flat buffer after backward) on a world-size-1 RCCL group, f32 and loss-scaled f16:
    one step each from the same weights: same gradients (to the reordering of f32 atomics / a flipped 16-bit rounding when the two
    module instances autotune differently) and same weights (to Adam's +-lr on sign-unstable near-zero gradients)."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_dist_world1.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(res)
    for name, tol in (("f32", 2e-3), ("f16", 5e-2)):
        x = res[name]
        assert x["finite"]
        assert abs(x["loss"][0] - x["loss"][1]) <= (1e-5 if name == "f32" else 5e-3) * abs(x["loss"][1]), (name, x)
        assert x["grad_rel"] < tol, (name, x)
        assert x["w_maxabs"] <= 2.1e-4, (name, x)  # one Adam step of lr = 1e-4: at most a flipped +-lr on sign-unstable elements


def test_hooked_backward_replay_world1():
    """the N > 1 step must be the benchmarked step.  With gradient-bucket hooks installed (world-size-1 RCCL group) the
    backward is a RECORDED sequence cut at the hooks -- segment, Python collective, segment, ... (`_lib.SegmentChain`) -- and must be bit-identical to
    the same steps issued launch by launch (deterministic mode, six steps), fire every in-backward hook exactly once per step in bucket order, and
    have run the stream / hardware-queue self-test with the collective's stream in the picture (tests/_dist_world1_replay.py)."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_dist_world1_replay.py")], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rep, eag = res["replayed"], res["eager"]
    assert res["identical"], (rep["steps"], eag["steps"])
    assert rep["segments"] == ["SegmentChain"] and rep["cuts"] == [3], rep  # buckets 0, 1, 2 inside backward; the last one fires behind the join
    assert eag["segments"] == []
    for x in (rep, eag):
        assert x["fired"] == [0, 1, 2, 3] * 5, x["fired"]
        # the self-test RAN with the collective in the picture; whether the box's queue mapping let every pair overlap is a measurement, printed
        # below, not a property of the replay
        assert x["hooked_selftest"] is True and x["selftest"] is not None
    print("stream self-test:", rep["selftest"])


def test_deterministic_mode_is_bit_identical():
    """FALNET_DETERMINISTIC=1: two fresh model instances, two optimiser steps each (Stage-1 in f32 and bf16, Stage-2 in f32) from the
    same weights and inputs give bit-identical losses, gradients, weights and disparities -- ordered scalar reductions, no
    split-K / fused-bias atomics, single-writer slab reduce, cached-or-heuristic kernel choices (no timing)."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_deterministic.py")], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for name, x in res.items():
        assert x["identical"], (name, x)


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
def test_data_parallel_two_ranks_one_gpu(dtype_name, tmp_path):
    """World size 2 with real kernels (two processes on cuda:0, gloo transport: RCCL refuses two ranks on one device): start-up
    broadcast + checksum from diverged weights, the overlapped bucket all-reduce fired from the weight-gradient side stream, 1/world in
    Adam.  After two steps both ranks hold bit-identical parameters, and they equal the single-process update on the whole batch
    (mean losses over equal shards): f32 to the reordering of f32 atomics, bf16 to its rounding."""
    import json
    import subprocess
    import sys
    out = tmp_path / "dp2.json"
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_dp2_gloo_gpu.py"), str(out), dtype_name],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.load(open(out))
    print(res)
    assert res["same_params_across_ranks"]
    # per-rank mean losses differ from the full-batch mean (different pairs); their average is the full-batch loss of the FIRST step
    assert res["grad_cos"] > (0.9999 if dtype_name == "f32" else 0.99)
    assert res["grad_rel"] < (2e-3 if dtype_name == "f32" else 0.15)
    assert res["w_maxabs"] <= 4.2e-4  # two Adam steps of lr = 1e-4: at most +-lr per step on sign-unstable elements


@pytest.mark.parametrize("launch", ["torchrun", "self"])
def test_bench_two_ranks_reports_allreduce(launch):
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank) AND typed as is (`python3 bench.py --gpus 2`,
    WORLD_SIZE unset: the script starts its ranks as child processes itself), on the one GPU of a test box over gloo
    (FALNET_DIST_BACKEND): the line must carry n_gpus = 2, the whole-job rate, and the `allreduce` block -- both ranks seen, parameters still
    identical across ranks after the timed steps, isolated times per bucket, the step time without the collective and the exposed part."""
    import json
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["FALNET_DIST_BACKEND"] = "gloo"
    head = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29541"] \
        if launch == "torchrun" else [sys.executable]
    cmd = head + [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "2", "--height", "64", "--width", "128",
           "--full", "--no-cpu-baseline", "--dtype", "f32"] + (["--no-roofline"] if launch == "torchrun" else ["--no-live-traffic"])
    # (the self-launched form runs rank 0's measurement legs too -- phase marks, the instrumented pass: steps on ONE rank after the timed region, which
    #  must not issue collectives the other rank never joins)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    if launch == "self":
        assert r.stdout.strip().splitlines()[-1] == line  # the relayed JSON is the LAST line of stdout
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 4 and d["scaling"] == "weak"
    a = d["allreduce"]
    assert a["ranks_seen"] == 2 and a["param_checksum_equal"] is True and a["bytes"] > 60e6 and len(a["buckets_bytes"]) == 4
    assert sum(a["buckets_bytes"]) == a["bytes"]
    assert a["isolated_ms"]["whole_buffer"] > 0 and a["ms_per_step_without_collective"] > 0 and np.isfinite(a["exposed_ms"])
    assert abs(d["value"] - 2 * 2 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]  # whole-job pairs/s = world * batch / step time
    if launch == "self":
        assert d["roofline"]["achieved"] > 0 and d["roofline"]["traffic"] is None or isinstance(d["roofline"]["traffic"], dict)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_adam_fused_with_repack_equals_standalone_update(dt):
    """FlatAdam.step's default path -- the optimiser update of every packed layer inside the launch that re-packs it
    (falnet_adam_pack_batched) + a range list for the rest (falnet_adam_ranges) -- against the stand-alone flat update followed by the
    re-pack: same gradients, two steps each (bias-corrected moments), then weights, moments and every packed operand compared.
    Reference: Train_Stage1_K.py:177-180 (torch.optim.Adam, lr 1e-4, betas (0.5, 0.999)); the stand-alone kernel is pinned to it by G2."""
    LF.set_compute_dtype(dt)
    left, right, mn, mx = synthetic.synthetic_pair(1, 64, 128, seed=9)
    results = []
    for fused in (True, False):
        m = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(7)}, no_levels=7, compute_dtype=dt).to(DEV).train()
        opt = train.FlatAdam(m)
        old = train._ADAM_PACK
        train._ADAM_PACK = fused
        try:
            for _ in range(2):
                train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV), optimize=False)
                g = m.flat_gradients()
                g.copy_(torch.sin(torch.arange(g.numel(), device=DEV) * 0.37) * 1e-3)  # the same gradient for both variants
                opt.step(0.5, scaler=train.loss_scaler(m))
            disp = m(left.to(DEV), mn.to(DEV), mx.to(DEV)).detach().clone()  # uses the packed copies the update left behind
        finally:
            train._ADAM_PACK = old
        packed = {k: (pc.wf.float().clone(), pc.wd.float().clone(), None if pc.wu is None else pc.wu.float().clone()) for k, pc in m._packed.items() if pc.wf is not None}
        results.append((m.flat_parameters().clone(), opt.m.clone(), opt.v.clone(), packed, disp, float(opt.state[1])))
        del m, opt
    LF.set_compute_dtype(torch.float32)
    (fa, ma, va, pa, da, ta), (fb, mb, vb, pb, db, tb) = results
    assert ta == tb == 2.0
    assert float((fa - fb).abs().max()) <= 1e-7 * float(fb.abs().max()) and rel(ma, mb) < 1e-6 and rel(va, vb) < 1e-6
    assert pa.keys() == pb.keys()
    for k in pa:
        for x, y in zip(pa[k], pb[k]):
            assert (x is None) == (y is None)
            if x is not None:  # a master that differs in its last f32 bit may round to the neighbouring 16-bit value: one 16-bit ulp
                assert float((x - y).abs().max()) <= (2.0 ** -7 if dt != torch.float32 else 1e-6) * float(y.abs().max()), k
    assert rel(da, db) < (1e-5 if dt == torch.float32 else 5e-2)  # (two instances autotune their 16-bit kernels independently)
