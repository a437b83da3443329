"""GPU: weight decay / bias decay of the fused Adam on every optimiser path -- the range kernel, the update fused with the weight re-pack,
the stand-alone flat update, the f16 guard -- plus the optimiser's checkpoint state and the training scripts' flags.

Reference for every numeric check: torch.optim.Adam on the CPU in float64 with the reference's two param groups (Train_Stage1_K.py:177-180),
fed the same f32 inputs (tests/_adam_decay_ref.py; never the code under test, never the decay-0 HIP path).  Tolerance per element after K
steps: K * 2^-23 * |p_ref64| + K * 16 * lr * 2^-20 (derivation there).  Every decay test also asserts that the decayed result lies more than
100 x that bound away from the decay-0 run of the same inputs.  Measured on an MI355X: worst element 0.452 of the bound, smallest
decayed-vs-decay-0 distance 591 x the bound (every comparison prints its figure before it asserts: run with -s)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import synthetic, train  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402

import _adam_decay_ref as R  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LR, BETAS, EPS = 1e-4, (0.5, 0.999), 1e-8
WD, BD = 1e-2, 3e-3  # large on purpose: well above gradient noise


def build(n_levels, dtype=torch.float32, sd=None):
    LF.set_compute_dtype(dtype)
    m = FAL_netB({"state_dict": sd or synthetic.seeded_falnetb_state_dict(n_levels)}, no_levels=n_levels, compute_dtype=dtype)
    return m.to(DEV).train()


@pytest.fixture(autouse=True)
def _f32_losses_afterwards():
    yield
    LF.set_compute_dtype(torch.float32)


def trainable(m):
    return {n: p for n, p in m._trainable_named()}


def grads_by_name(m, flat_grad_cpu):
    return {n: flat_grad_cpu[off:off + p.numel()] for (n, p), off in zip(m._trainable_named(), m._offsets)}


def hand_gradient(numel, step, amp=1e-3):
    """A gradient that changes in size and sign with every step."""
    i = torch.arange(numel, device=DEV, dtype=torch.float32)
    return torch.sin(i * 0.37 + 1.3 * step) * amp * (1 + step) * (-1) ** step


def padding_mask(m):
    """True at the 16-B padding elements between the parameter slices of the flat buffer."""
    mask = torch.ones(m.flat_parameters().numel(), dtype=torch.bool)
    for (n, p), off in zip(m._trainable_named(), m._offsets):
        mask[off:off + p.numel()] = False
    return mask


def compare_model(m, ref, ref0, K, what):
    for n, p in trainable(m).items():
        R.check(p, ref.p[n].detach(), K, LR, f"{what} {n}")
    if ref0 is not None:
        for n, p in trainable(m).items():
            R.check_decay_seen(p, ref0.p[n].detach(), K, LR, f"{what} {n}")


# ---------------------------------------------------------------------------------------------------------------- range kernel
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_ranges_kernel_decays_each_range_by_its_own_value(grad_scale):
    """falnet_adam_ranges_wd on a synthetic flat buffer: 7 slices of odd sizes (one shorter than 4 elements, neighbours with different
    decays), each padded to 16 B, one range per padded slice with its own decay; random p and g, m = v = 0, K = 5 steps with a gradient
    that changes every step.  Padding elements must still be exactly 0 in p, m and v."""
    lib = L.lib()
    sizes = [10007, 33, 3, 4096, 7, 129, 1025]
    names = ["a.weight", "a.bias", "b.bias", "b.weight", "c.bias", "c.weight", "d.bias"]  # (a.bias | b.bias | b.weight: 3e-3, 3e-3, 1e-2 side by side)
    padded = [(s + 3) // 4 * 4 for s in sizes]
    offs = [sum(padded[:i]) for i in range(len(sizes))]
    total = sum(padded)
    gen = torch.Generator().manual_seed(5)
    buf = torch.zeros(4, total, device=DEV)  # rows: p, g, m, v -- one layout, element offsets g_off = total, m_off = 2 total, v_off = 3 total
    named = {}
    for n, s, o in zip(names, sizes, offs):
        named[n] = torch.randn(s, generator=gen) * 0.1
        buf[0, o:o + s] = named[n].to(DEV)
    ranges = torch.tensor([x for o, c in zip(offs, padded) for x in (o, c)], dtype=torch.int64, device=DEV)
    decays = torch.tensor([BD if "bias" in n else WD for n in names], dtype=torch.float64, device=DEV)
    state = torch.tensor([LR, 0.0], device=DEV)
    ref = R.RefAdam64(named, LR, BETAS, EPS, WD, BD)
    ref0 = R.RefAdam64(named, LR, BETAS, EPS)
    K = 5
    for s in range(K):
        grads = {n: torch.randn(sz, generator=gen) * 1e-3 * (1 + s) * (-1) ** s for n, sz in zip(names, sizes)}
        for n, sz, o in zip(names, sizes, offs):
            buf[1, o:o + sz] = grads[n].to(DEV)
        L.check(lib.falnet_adam_ranges_wd(L.ptr(buf), total, 2 * total, 3 * total, L.ptr(ranges), L.ptr(decays), len(sizes), L.ptr(state),
                                          BETAS[0], BETAS[1], EPS, grad_scale, None, L.stream_ptr()), "adam_ranges_wd")
        L.check(lib.falnet_adam_tick(L.ptr(state), None, L.stream_ptr()), "adam_tick")
        ref.step(grads, grad_scale)
        ref0.step(grads, grad_scale)
    assert float(state[1]) == K
    got = buf.cpu()
    pad = torch.ones(total, dtype=torch.bool)
    for n, sz, o in zip(names, sizes, offs):
        pad[o:o + sz] = False
        R.check(got[0, o:o + sz], ref.p[n].detach(), K, LR, f"ranges gs={grad_scale} {n}")
        R.check_decay_seen(got[0, o:o + sz], ref0.p[n].detach(), K, LR, f"ranges gs={grad_scale} {n}")
    assert int(pad.sum()) > 0
    for row in (0, 2, 3):
        assert torch.equal(got[row][pad], torch.zeros(int(pad.sum()))), row


# ---------------------------------------------------------------------------------------------------------------- model-level paths
def run_decayed_steps(m, opt, steps=3):
    """`steps` stage1_steps; after each the flat gradient the update consumed goes to the CPU and advances the float64 references
    (decayed and decay-0) with THOSE gradients; every trainable tensor is compared after every step."""
    left, right, mn, mx = synthetic.synthetic_pair(2, 64, 128, seed=3, distinct=True)
    ref = R.RefAdam64(trainable(m), LR, BETAS, EPS, WD, BD)
    ref0 = R.RefAdam64(trainable(m), LR, BETAS, EPS)
    amask = {n: p.detach().clone() for n, p in m.named_parameters() if "amask_conv" in n}
    assert amask
    for k in range(1, steps + 1):
        out = train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV))
        assert torch.isfinite(out["loss"]).item()
        g = grads_by_name(m, m.flat_gradients().detach().cpu())
        ref.step(g)
        ref0.step(g)
        compare_model(m, ref, ref0 if k == steps else None, k, f"step {k}")
    assert float(opt.state[1]) == steps
    for n, p in m.named_parameters():
        if "amask_conv" in n:
            assert torch.equal(p.detach(), amask[n]) and p.grad is None, n
    pad = padding_mask(m)
    for t in (m.flat_parameters(), opt.m, opt.v):
        assert torch.equal(t.detach().cpu()[pad], torch.zeros(int(pad.sum())))
    return left, mn, mx


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_pack_fused_update_decays_and_repacks_the_decayed_masters(dt):
    """FAL_netB, N = 49, 2 x 64 x 128: three stage1_steps with weight_decay 1e-2 / bias_decay 3e-3 through the update fused with the re-pack
    (falnet_adam_pack_batched_wd + falnet_adam_ranges_wd); masters are f32 in both dtypes.  Then a FRESH model loaded from m.state_dict():
    every packed operand the update left behind -- wf / wd of each layer, the composed logits weights, the sub-pixel deconv weights -- is
    bit-identical to what the fresh model packs from the decayed masters.  (The bit-identical ret_disp forward of the two models is asserted
    by test_fresh_model_forward_is_bit_identical_after_decayed_steps, in the mode where a forward is reproducible at all.)"""
    m = build(49, dt)
    opt = train.FlatAdam(m, LR, BETAS, EPS, weight_decay=WD, bias_decay=BD)
    assert train._ADAM_PACK
    left, mn, mx = run_decayed_steps(m, opt)
    assert m._packed_is_fresh()  # what the optimiser packed is what the next forward would run on
    fresh = build(49, dt, sd={k: v.detach().clone() for k, v in m.state_dict().items()})
    with torch.no_grad():
        fresh(left.to(DEV), mn.to(DEV), mx.to(DEV))  # builds the plan: packs from the masters
        d1, d2 = (m(left.to(DEV), mn.to(DEV), mx.to(DEV)).detach().clone() for _ in range(2))
    # why the forward comparison lives in deterministic mode: the figure, not an assertion (it may well be 0 on a quiet run)
    print(f"adam-decay default-mode forward, ONE model twice ({dt}): max |d1 - d2| = {float((d1 - d2).abs().max()):.3e} of {float(d1.abs().max()):.1f}")
    assert m._packed.keys() == fresh._packed.keys()
    seen = 0
    for k, pc in m._packed.items():
        qc = fresh._packed[k]
        assert torch.equal(pc.weight.detach(), qc.weight.detach()), k  # (includes the composed logits master)
        for name in ("wf", "wd", "wu", "wdd"):
            a, b = getattr(pc, name, None), getattr(qc, name, None)
            assert (a is None) == (b is None), (k, name)
            if a is not None:
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (k, name)
                seen += 1
    assert seen >= 30 and "logits" in m._packed  # (the derived logits weights among them)
    if dt != torch.float32:  # (sub-pixel deconv weights exist in the 16-bit types only)
        assert any(pc.wu is not None for pc in m._packed.values())


def test_fresh_model_forward_is_bit_identical_after_decayed_steps():
    """After three decayed steps (f32 and bf16 compute) a fresh model loaded from m.state_dict() gives a BIT-identical ret_disp forward: the
    packed 16-bit copies and the derived weights were rebuilt from the decayed masters.  Run in a child process with FALNET_DETERMINISTIC=1
    (tests/_adam_decay_repack.py): in the default mode one and the same model's forward differs from call to call (split-K atomics;
    measured 2.4e-4 of 161 in f32 at this shape, with and without decay; the pack-fused test above prints the figure of its own run), so bit
    equality of two models cannot be asked there."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_adam_decay_repack.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])
    assert set(res) == {"f32", "bf16"}
    for name, x in res.items():
        assert x["moved"], name
        assert x["trained"] == x["again"], (name, x)  # (the premise: reproducible in this mode)
        assert x["trained"] == x["fresh"], (name, x)


def test_standalone_update_with_pack_fusion_off(monkeypatch):
    """The same comparison with the pack fusion off: every step's update is the stand-alone flat launch (falnet_adam_step_wd)."""
    monkeypatch.setattr(train, "_ADAM_PACK", False)
    m = build(49)
    opt = train.FlatAdam(m, LR, BETAS, EPS, weight_decay=WD, bias_decay=BD)
    run_decayed_steps(m, opt)


def test_standalone_update_before_any_plan_exists():
    """opt.step() on a hand-set gradient before the model has a plan: FlatAdam falls through to the stand-alone flat update."""
    m = build(49)
    m.ensure_flat()
    assert not m._plans
    opt = train.FlatAdam(m, LR, BETAS, EPS, weight_decay=WD, bias_decay=BD)
    ref = R.RefAdam64(trainable(m), LR, BETAS, EPS, WD, BD)
    ref0 = R.RefAdam64(trainable(m), LR, BETAS, EPS)
    K = 5
    for s in range(K):
        g = hand_gradient(m.flat_gradients().numel(), s)
        g[padding_mask(m).to(DEV)] = 0  # (backward never writes the padding)
        m.flat_gradients().copy_(g)
        opt.step(0.125)
        gn = grads_by_name(m, g.cpu())
        ref.step(gn, 0.125)
        ref0.step(gn, 0.125)
    assert not m._plans and float(opt.state[1]) == K
    compare_model(m, ref, ref0, K, "no plan")
    pad = padding_mask(m)
    for t in (m.flat_parameters(), opt.m, opt.v):
        assert torch.equal(t.detach().cpu()[pad], torch.zeros(int(pad.sum())))


def test_decay_changed_between_steps_holds_from_the_next_step():
    """The decays are read at every step: two steps at (1e-2, 3e-3), then two at (2e-3, 0) -- both the stand-alone table and (after a plan
    exists) the range table are refreshed."""
    m = build(7)
    m.ensure_flat()
    opt = train.FlatAdam(m, LR, BETAS, EPS, weight_decay=WD, bias_decay=BD)
    ref = R.RefAdam64(trainable(m), LR, BETAS, EPS, WD, BD)
    ref0 = R.RefAdam64(trainable(m), LR, BETAS, EPS)
    left, right, mn, mx = synthetic.synthetic_pair(1, 64, 128, seed=9)
    pad = padding_mask(m).to(DEV)
    for s in range(6):
        if s == 2:
            opt.weight_decay, opt.bias_decay = 2e-3, 0.0
            ref.set_decays(2e-3, 0.0)
        if s == 3:  # from here on a plan exists: the pack-fused path
            train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV), optimize=False)
        if s == 5:
            opt.weight_decay, opt.bias_decay = WD, BD
            ref.set_decays(WD, BD)
        g = hand_gradient(m.flat_gradients().numel(), s)
        g[pad] = 0
        m.flat_gradients().copy_(g)
        opt.step()
        ref.step(grads_by_name(m, g.cpu()))
        ref0.step(grads_by_name(m, g.cpu()))
        compare_model(m, ref, ref0 if s == 5 else None, s + 1, f"changing decay, step {s + 1}")


def test_captured_step_decays_through_the_standalone_update():
    """train.GraphedStage1Step with non-zero decays (tests/_adam_decay_graph.py, a child process: a capture that fails leaves the HIP context
    of its process unusable).  Under stream capture FlatAdam takes the stand-alone flat update (falnet_adam_step_wd), whose decay tables must
    already be on the device -- the eager steps before the capture all went through the pack-fused path, and a host-to-device copy cannot
    be captured.  Two eager steps, the constructor's warm-up step, then three replays, every one against the float64 reference advanced
    with the gradient that step left in the flat buffer (the usual bound; the last one more than 100 x the bound away from decay 0)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_adam_decay_graph.py")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "graphed decay: ok" in r.stdout


def test_stale_decay_tables_are_refused_under_capture(monkeypatch):
    """A decay changed without an eager step in between must not be copied to the device inside a capture: FlatAdam refuses.  (The capture
    state is faked: no real capture is broken off half way.)"""
    m = build(7)
    m.ensure_flat()
    opt = train.FlatAdam(m, LR, BETAS, EPS, weight_decay=WD, bias_decay=BD)
    real = torch.cuda.is_current_stream_capturing
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="eager step"):  # no table yet
        opt._decay_segments(m.flat_parameters())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", real)
    m.flat_gradients().zero_()
    opt.step()
    opt.weight_decay = 2e-3
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="eager step"):  # a table for other values
        opt._decay_segments(m.flat_parameters())
    opt.weight_decay = WD
    assert opt._decay_segments(m.flat_parameters())[1] is opt._segments[1].dev  # current tables: used as they are


# ---------------------------------------------------------------------------------------------------------------- f16 guard
@pytest.mark.parametrize("fused", [False, True])
def test_f16_guard_skips_update_and_decay(fused):
    """With a LossScaler and non-zero decays: a clean step, then one `inf` in the flat gradient -- p, m, v bit-unchanged, the step count
    unchanged, the scale halved -- then a clean step that matches the reference (which never saw the skipped one)."""
    m = build(7, torch.float16)
    m.ensure_flat()
    left, right, mn, mx = synthetic.synthetic_pair(1, 64, 128, seed=9)
    opt = train.FlatAdam(m, LR, BETAS, EPS, weight_decay=WD, bias_decay=BD)
    sc = train.loss_scaler(m)
    assert sc is not None
    if fused:  # a plan exists: FlatAdam takes the pack-fused path
        train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV), optimize=False)
        assert m._plans
    ref = R.RefAdam64(trainable(m), LR, BETAS, EPS, WD, BD)
    ref0 = R.RefAdam64(trainable(m), LR, BETAS, EPS)
    pad = padding_mask(m).to(DEV)
    n = m.flat_gradients().numel()

    def clean_step(s):
        scale = float(sc.state[0])
        g = hand_gradient(n, s, amp=1e-3 * scale)  # the backward of a scaled loss: `scale` times too large
        g[pad] = 0
        m.flat_gradients().copy_(g)
        opt.step(0.5, scaler=sc)
        for r in (ref, ref0):
            r.step(grads_by_name(m, g.cpu()), 0.5 / scale)

    clean_step(0)
    compare_model(m, ref, None, 1, f"f16 fused={fused} step 1")
    before = [t.detach().clone() for t in (m.flat_parameters(), opt.m, opt.v)]
    scale0, skipped0 = float(sc.state[0]), float(sc.state[3])
    g = hand_gradient(n, 1, amp=1e-3 * scale0)
    g[pad] = 0
    g[n // 3] = float("inf")
    m.flat_gradients().copy_(g)
    opt.step(0.5, scaler=sc)
    for a, b in zip(before, (m.flat_parameters(), opt.m, opt.v)):
        assert torch.equal(a, b.detach())
    assert float(opt.state[1]) == 1.0  # the skipped step does not count
    assert float(sc.state[0]) == 0.5 * scale0 and float(sc.state[3]) == skipped0 + 1 and float(sc.state[2]) == 0.0
    clean_step(2)
    assert float(opt.state[1]) == 2.0
    compare_model(m, ref, ref0, 2, f"f16 fused={fused} step 2")


# ---------------------------------------------------------------------------------------------------------------- default untouched
@pytest.mark.parametrize("with_plan", [False, True])
def test_zero_decays_are_the_default_optimiser_bit_for_bit(with_plan):
    """FlatAdam(m) and FlatAdam(m, weight_decay=0.0, bias_decay=0.0): bit-identical parameters and moments after two step()s from the same
    seeded start on the same hand-set gradient buffer (elementwise kernels, no atomics)."""
    left, right, mn, mx = synthetic.synthetic_pair(1, 64, 128, seed=9)
    res = []
    for kw in ({}, {"weight_decay": 0.0, "bias_decay": 0.0}):
        m = build(7)
        m.ensure_flat()
        opt = train.FlatAdam(m, **kw)
        if with_plan:
            train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV), optimize=False)
        for s in range(2):
            m.flat_gradients().copy_(hand_gradient(m.flat_gradients().numel(), s) * ~padding_mask(m).to(DEV))  # (backward never writes the padding)
            opt.step()
        res.append([t.detach().clone() for t in (m.flat_parameters(), opt.m, opt.v, opt.state)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- resume
def test_optimizer_state_dict_resumes_bit_identically():
    """Two decayed steps, state_dict(), a new model and optimiser built from the saved weights and optimiser state: t, m, v and the device
    step counter equal bitwise; one more step() on an identical hand-set gradient gives bit-identical parameters in both.  A model of another
    no_levels refuses the state."""
    m = build(7)
    m.ensure_flat()
    opt = train.FlatAdam(m, LR, BETAS, EPS, weight_decay=WD, bias_decay=BD)
    n = m.flat_gradients().numel()
    real = ~padding_mask(m).to(DEV)  # (backward never writes the padding elements: their gradient is 0)
    for s in range(2):
        m.flat_gradients().copy_(hand_gradient(n, s) * real)
        opt.step()
    sd = opt.state_dict()
    assert sd["t"] == 2 and sd["m"].device.type == "cpu" and sd["weight_decay"] == WD and sd["bias_decay"] == BD
    m2 = build(7, sd={k: v.detach().clone() for k, v in m.state_dict().items()})
    opt2 = train.FlatAdam(m2, LR, BETAS, EPS)
    opt2.load_state_dict(sd)
    assert opt2.t == 2 and (opt2.weight_decay, opt2.bias_decay) == (WD, BD)
    assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and torch.equal(opt2.state, opt.state)
    assert torch.equal(m2.flat_parameters(), m.flat_parameters())
    for mm, oo in ((m, opt), (m2, opt2)):
        mm.flat_gradients().copy_(hand_gradient(n, 2) * real)
        oo.step()
    assert torch.equal(m2.flat_parameters(), m.flat_parameters())
    assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and float(opt2.state[1]) == float(opt.state[1]) == 3.0
    with pytest.raises(ValueError, match="layout"):
        train.FlatAdam(build(9)).load_state_dict(sd)


# ---------------------------------------------------------------------------------------------------------------- scripts
@pytest.mark.parametrize("script", ["Train_Stage1_K.py", "Train_Stage2_K.py"])
def test_training_scripts_take_the_decay_flags(script, tmp_path):
    """A fresh child process under its own time limit: exit status 0, finite loss lines, and a checkpoint that holds the four reference keys
    plus 'optimizer' (loadable, with the decays of the command line)."""
    cmd = [sys.executable, os.path.join(ROOT, script), "--synthetic", "--epochs", "1", "--epoch_size", "2", "-b", "2", "-ch", "64", "-cw", "128",
           "--weight-decay", "1e-4", "--bias-decay", "1e-5", "--save-path", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{") and '"loss"' in line]
    assert losses
    for rec in losses:
        assert rec["loss"] == rec["loss"] and abs(rec["loss"]) != float("inf")
    ckpt = torch.load(os.path.join(str(tmp_path), "checkpoint.pth.tar"), map_location="cpu")
    assert {"epoch", "m_model", "state_dict", "best_rmse", "optimizer"} <= set(ckpt)
    o = ckpt["optimizer"]
    assert o["t"] == 2 and o["weight_decay"] == 1e-4 and o["bias_decay"] == 1e-5
    assert o["m"].dtype == torch.float32 and o["m"].shape == o["v"].shape and float(o["v"].abs().sum()) > 0
    if script == "Train_Stage1_K.py":
        # a resumed run of the same stage (--pretrained carries 'optimizer') continues the step count and the moments instead of restarting them
        again = tmp_path / "resumed"
        cmd2 = cmd[:-1] + [str(again), "--pretrained", os.path.join(str(tmp_path), "checkpoint.pth.tar"), "--start-epoch", "1", "--epochs", "2"]
        r2 = subprocess.run(cmd2, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r2.returncode == 0, r2.stderr[-2000:]
        o2 = torch.load(os.path.join(str(again), "checkpoint.pth.tar"), map_location="cpu")["optimizer"]
        assert o2["t"] == 4 and o2["layout"] == o["layout"]
