"""GPU: csrc/ssim.hip against the float64 definition of tests/_ssim_ref.py -- the metric per frame, the loss value and its gradient per element,
the training step with the SSIM term against the float64 oracle, and the --view-metrics command line.

Bounds.  The metric is f64 on both sides: 1e-9 absolute (the two separable passes differ in order from the reference's double sum by at most 22
roundings on sums of at most 65 025, <= 1.6e-10 in each second moment, <= 1e-9 in the sigma terms over denominators >= C2 = 58.5: |dS| < 5e-11; the
bound leaves a margin of 20).  The loss is f32 in the kernel, so its tolerance is what f32 rounding alone does to the same formulas, measured per
case on the CPU: 16 x the worst per-window error of the f32 restatement for the value (the error of a mean cannot exceed the worst error of its
terms), 16 x the worst per-element error of its autograd gradient for the gradient (the factor covers another summation order; an indexing or
halo error is of order 1).  FALNET_SSIM_REPORT=<file> writes both reference errors and the kernel's, per case."""
import functools
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import metrics as M  # noqa: E402
from fal_net_amd import myUtils as utils  # noqa: E402
from fal_net_amd import synthetic, train  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402
from oracle import falnet_oracle as O  # noqa: E402

import _ssim_ref as R  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = "cuda"
METRIC_BOUND = 1e-9
FACTOR = 16
A_SSIM = 0.15
REPORT = {}  # case -> figures, written by test_zz_report


# ---- the metric ------------------------------------------------------------------------------------------------------------------------------
def metric_pair(B, H, W, seed):
    """A right image in the loader's range and a synthesised view around it that leaves [0, 255] in places (the clamp) -- CPU tensors."""
    gen = torch.Generator().manual_seed(seed)
    right = torch.rand(B, 3, H, W, generator=gen) - torch.tensor(R.MEAN).view(1, 3, 1, 1)
    p_im = right + 0.08 * torch.randn(B, 3, H, W, generator=gen)
    return p_im, right


def ssim_of(p_im, right, **kw):
    return float(M.ssim(p_im.to(DEV), right.to(DEV), **kw)[M.COL["ssim"]])


@pytest.mark.parametrize("shape", R.METRIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metric_vs_f64(shape):
    p_im, right = metric_pair(*shape, seed=sum(shape))
    x, _ = R.metric_operands(p_im, right)
    assert shape == (1, 11, 11) or (float(x.min()) == 0 and float(x.max()) == 255)  # the clamp is exercised
    ref, got = R.metric(p_im, right), ssim_of(p_im, right)
    REPORT["metric %dx%dx%d" % shape] = {"f64": ref, "kernel": got, "abs": abs(got - ref), "bound": METRIC_BOUND}
    print("metric", shape, "f64", repr(ref), "kernel", repr(got), "abs", abs(got - ref))
    assert 0 < ref < 1 and abs(got - ref) <= METRIC_BOUND


def test_metric_identical_and_constant_images():
    gen = torch.Generator().manual_seed(5)
    img = (torch.rand(1, 3, 29, 41, generator=gen) > 0.5).float()  # 0 and 1 with mean 0: 0 and 255 on both sides, exactly
    x, y = R.metric_operands(img, img, mean=(0.0, 0.0, 0.0))
    assert torch.equal(x, y)
    got = ssim_of(img, img, mean=(0.0, 0.0, 0.0))
    print("identical images:", repr(got))
    assert abs(got - 1.0) <= 1e-12
    a, b = torch.full((2, 3, 19, 23), 0.4), torch.full((2, 3, 19, 23), 0.6)
    x, y = R.metric_operands(a, b, mean=(0.0, 0.0, 0.0))
    av, bv = float(x[0, 0, 0, 0]), float(y[0, 0, 0, 0])
    assert av == 102.0 and abs(bv - 153.0) < 1e-4
    want = (2 * av * bv + R.METRIC_C1) / (av * av + bv * bv + R.METRIC_C1)
    got = ssim_of(a, b, mean=(0.0, 0.0, 0.0))
    print("constant images:", repr(got), "expected", repr(want))
    assert abs(got - want) <= 1e-9


def test_metric_writes_its_column_only_and_repeats_in_bits():
    p_im, right = (t.to(DEV) for t in metric_pair(1, 45, 77, seed=9))
    table = M.MetricTable(3)
    gen = torch.Generator().manual_seed(2)
    table.table.view(torch.int64).copy_(torch.randint(-2 ** 62, 2 ** 62, (3, M.ROW), generator=gen, dtype=torch.int64))  # any bits, NaNs included
    before = table.table.view(torch.int64).clone()
    lib = L.lib()
    vals = []
    for det in (0, 1, 0, 1):
        lib.falnet_set_deterministic(det)
        try:
            M.ssim(p_im, right, out=table.row(1))
        finally:
            lib.falnet_set_deterministic(int(L.DETERMINISTIC))
        after = table.table.view(torch.int64)
        keep = torch.ones(3, M.ROW, dtype=torch.bool, device=DEV)
        keep[1, M.COL["ssim"]] = False
        assert torch.equal(after[keep], before[keep])  # the other 23 columns of the row, and the other rows, in bits
        vals.append(int(after[1, M.COL["ssim"]]))
    assert len(set(vals)) == 1 and vals[0] != int(before[1, M.COL["ssim"]])


class _FixedView(torch.nn.Module):
    """Stands in for the model in train.validate: returns the views it was given, frame by frame."""

    def __init__(self, views):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1, device=DEV))
        self.views, self.i = views, 0

    def forward(self, left, mn, mx, ret_disp=True, ret_pan=True, ret_subocc=True):
        p = self.views[self.i % len(self.views)]
        self.i += 1
        z = torch.zeros(1, 1, *p.shape[-2:], device=DEV)
        return p, z, z, z


def test_metric_value_is_the_same_through_every_caller():
    """MetricTable.result(), metrics.ssim, myUtils.get_ssim and train.validate (both modes) report the kernel's value of the same frames."""
    gen = torch.Generator().manual_seed(4)
    frames = []
    for _ in range(2):
        left_u8, right_u8 = (torch.randint(0, 256, (37, 52, 3), generator=gen, dtype=torch.uint8) for _ in range(2))
        frames.append((left_u8, right_u8))
    from fal_net_amd import datasets as DS
    rights = [DS.to_model_input(r, DEV) for _, r in frames]
    views = [r + 0.05 * torch.randn(r.shape, generator=gen).to(DEV) for r in rights]
    table = M.MetricTable(2)
    direct = []
    for i, (v, r) in enumerate(zip(views, rights)):
        M.ssim(v, r, out=table.row(i))
        direct.append(float(utils.get_ssim(v, r)))
        assert abs(direct[-1] - R.metric(v, r)) <= METRIC_BOUND
    res = table.result()
    assert list(res["ssim"]) == direct and res["ssim_mean"] == float(np.mean(direct))
    assert len(res["view"]) == 0 and res["rmse_mean"] == 0  # the view group was not written: its keys are what they were
    assert table.running_mean("ssim") == float(np.mean(direct))
    loader = [[(l, r, None)] for l, r in frames]
    for device_metrics in (False, True):
        out = train.validate(_FixedView(views), loader, log=None, device_metrics=device_metrics)
        assert out["ssim"] == pytest.approx(float(np.mean(direct)), abs=1e-15) and set(out) == {"rmse", "epe", "kitti", "ssim"}
        assert out["rmse"] == pytest.approx(float(np.mean([float(utils.get_rmse(v, r)) for v, r in zip(views, rights)])), rel=1e-6)


class _FixedEval(torch.nn.Module):
    """Stands in for the model in inference.evaluate: a zero disparity, and the views it was given where the loop asks for the view."""

    def __init__(self, views):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1, device=DEV))
        self.views, self.i = views, 0

    def forward(self, left, mn, mx, ret_disp=True, ret_subocc=False, ret_pan=False):
        z = torch.zeros(1, 1, *left.shape[-2:], device=DEV)
        if not ret_pan:
            return z
        self.i += 1
        return [self.views[(self.i - 1) % len(self.views)], z]


def test_evaluate_view_metrics():
    """inference.evaluate(products=[ViewMetrics()]): the view's errors and SSIM against the loader's right image in a table of their own, read once."""
    from fal_net_amd import datasets as DS
    from fal_net_amd import inference
    gen = torch.Generator().manual_seed(6)
    frames = [tuple(torch.randint(0, 256, (23, 61, 3), generator=gen, dtype=torch.uint8) for _ in range(2)) for _ in range(3)]
    rights = [DS.to_model_input(r, DEV) for _, r in frames]
    views = [r + 0.05 * torch.randn(r.shape, generator=gen).to(DEV) for r in rights]
    loader = [[(l, r, None)] for l, r in frames]
    plain = inference.evaluate(_FixedEval(views), loader, post="none", log=None)
    out = inference.evaluate(_FixedEval(views), loader, post="none", log=None, products=[inference.ViewMetrics(len(loader), DEV)])
    assert "view" not in plain and set(out) == set(plain) | {"view"} and out["n"] == plain["n"] == 3
    view = out["view"]
    assert set(view) == {"rmse", "mea", "psnr", "ssim", "n"} and view["n"] == 3
    assert view["ssim"] == pytest.approx(float(np.mean([R.metric(v, r) for v, r in zip(views, rights)])), abs=METRIC_BOUND)
    for k, f in (("rmse", utils.get_rmse), ("mea", utils.get_mea), ("psnr", utils.get_psnr)):
        assert view[k] == pytest.approx(float(np.mean([float(f(v, r)) for v, r in zip(views, rights)])), rel=1e-5), k


def test_too_small_images_raise():
    z = torch.zeros(1, 3, 10, 40, device=DEV)
    with pytest.raises(RuntimeError, match="smaller than one 11 x 11 window"):
        M.ssim(z, z)
    with pytest.raises(RuntimeError, match="smaller than one 11 x 11 window"):
        M.ssim(z.transpose(2, 3).contiguous(), z.transpose(2, 3).contiguous())
    s = torch.zeros(1, 3, 2, 9, device=DEV)
    with pytest.raises(RuntimeError, match="smaller than one 3 x 3 window"):
        LF.ssim_loss(s, s)


# ---- the loss: value and gradient ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_case(shape):
    """The inputs of a case and its references, computed once: f64 (the definition) and f32 (the same formulas: what rounding alone does)."""
    synth, label = R.pair(shape, seed=zlib.crc32(repr(shape).encode()) % 1000)
    m64, v64, g64 = R.loss_and_grad(synth, label, dtype=torch.float64)
    m32, v32, g32 = R.loss_and_grad(synth, label, dtype=torch.float32)
    return {"synth": synth, "label": label, "v64": float(v64), "g64": g64, "map_err32": float((m32.double() - m64).abs().max()),
            "grad_err32": float((g32.double() - g64).abs().max()), "n_win": m64.numel()}


def _ws(shape):
    B, C, H, W = shape
    return torch.zeros(int(L.lib().falnet_ssim_workspace_bytes(B, C, H, W, 1)) // 8, dtype=torch.float64, device=DEV)


def k_fwd(s, l, scale, out=None, accumulate=0, radius=1):
    B, C, H, W = s.shape
    out = torch.full((1,), float("nan"), device=DEV) if out is None else out
    ws = _ws(s.shape)
    rc = L.lib().falnet_ssim_loss_fwd(L.ptr(s), L.ptr(l), *R.MEAN, B, C, H, W, radius, scale, L.ptr(out), accumulate, L.ptr(ws), L.stream_ptr())
    return rc, out


def k_bwd(s, l, scale, ga, accumulate=0, gscale=None, radius=1):
    B, C, H, W = s.shape
    return L.lib().falnet_ssim_loss_bwd(L.ptr(s), L.ptr(l), *R.MEAN, B, C, H, W, radius, scale, L.ptr(gscale), L.ptr(ga), accumulate, L.stream_ptr())


def k_fwd_bwd(s, l, scale_out, out, scale_grad, ga, add, gscale=None, radius=1):
    B, C, H, W = s.shape
    ws = _ws(s.shape)
    rc = L.lib().falnet_ssim_loss_fwd_bwd(L.ptr(s), L.ptr(l), *R.MEAN, B, C, H, W, radius, scale_out, L.ptr(out), scale_grad, L.ptr(gscale), L.ptr(ga), add,
                                          L.ptr(ws), L.stream_ptr())
    return rc, ws


GUARD = 4096


def guarded(n, seed=1):
    """n floats of NaN between two guard zones of random bits -> (whole buffer, the view in the middle, a copy of the whole as int32)."""
    whole = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 2 * GUARD,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(DEV).view(torch.float32)
    mid = whole[GUARD:GUARD + n]
    mid.fill_(float("nan"))
    return whole, mid, whole.view(torch.int32).clone()


def guards_intact(whole, before, n):
    w = whole.view(torch.int32)
    return torch.equal(w[:GUARD], before[:GUARD]) and torch.equal(w[GUARD + n:], before[GUARD + n:])


@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_value_and_gradient_vs_f64(shape):
    c = loss_case(shape)
    s, l = c["synth"].to(DEV), c["label"].to(DEV)
    n = s.numel()
    scale = 1.0 / c["n_win"]
    assert c["n_win"] == shape[0] * shape[1] * (shape[2] - 2) * (shape[3] - 2)
    rc, out = k_fwd(s, l, scale)
    assert rc == 0, L.lib().falnet_last_error()
    whole, ga, before = guarded(n)
    assert k_bwd(s, l, scale, ga) == 0, L.lib().falnet_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ga).all()) and guards_intact(whole, before, n)  # every element written (assign mode, NaN pre-fill), nothing beyond
    v_err = abs(float(out) - c["v64"])
    g_err = float((ga.view(shape).double().cpu() - c["g64"]).abs().max())
    REPORT["loss %dx%dx%dx%d" % shape] = {"value_f64": c["v64"], "value_err_f32_ref_worst_window": c["map_err32"], "value_err_kernel": v_err,
                                          "grad_max_f64": float(c["g64"].abs().max()), "grad_err_f32_ref": c["grad_err32"], "grad_err_kernel": g_err}
    print("loss", shape, REPORT["loss %dx%dx%dx%d" % shape])
    assert c["map_err32"] > 0 and c["grad_err32"] > 0
    assert v_err <= FACTOR * c["map_err32"]
    assert g_err <= FACTOR * c["grad_err32"]


@pytest.mark.parametrize("shape", [R.LOSS_SHAPES[0], R.LOSS_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_loss_modes_agree(shape):
    """add mode is prior + gradient; _fwd_bwd is _fwd followed by _bwd; out accumulates; gscale multiplies; all of it twice, in both deterministic
    modes, with equal bits."""
    c = loss_case(shape)
    s, l = c["synth"].to(DEV), c["label"].to(DEV)
    n, scale = s.numel(), 1.0 / c["n_win"]
    lib = L.lib()
    g_assign = torch.empty(n, device=DEV)
    assert k_bwd(s, l, scale, g_assign) == 0
    prior = torch.randn(n, generator=torch.Generator().manual_seed(8)).to(DEV)
    whole, ga, before = guarded(n, seed=3)
    ga.copy_(prior)
    assert k_bwd(s, l, scale, ga, accumulate=1) == 0
    assert torch.equal(ga, prior + g_assign) and guards_intact(whole, before, n)
    _, v = k_fwd(s, l, scale)
    runs = []
    for det in (0, 1, 0, 1):
        lib.falnet_set_deterministic(det)
        try:
            out = torch.tensor([2.5], device=DEV)
            whole, gb, before = guarded(n, seed=4)
            rc, ws = k_fwd_bwd(s, l, 0.25 * scale, out, scale, gb, 0)
            assert rc == 0, lib.falnet_last_error()
            gc = prior.clone()
            rc, _ = k_fwd_bwd(s, l, 0.25 * scale, out, scale, gc, 1)
            assert rc == 0
        finally:
            lib.falnet_set_deterministic(int(L.DETERMINISTIC))
        assert guards_intact(whole, before, n)
        assert torch.equal(gb, g_assign) and torch.equal(gc, prior + g_assign)  # the same kernel: the same bits
        # the value: the two kernels give the windows to their threads in different orders -- each thread adds at most 5 f32 terms before the sums
        # are f64, so each side is within 5 * 2^-24 of the exact sum of its f32 terms
        assert abs(float(out) - (2.5 + 2 * 0.25 * float(v))) <= 1e-6 * (2.5 + float(v))
        assert abs(float(ws[-1]) * scale - float(v)) <= 1e-6 * float(v)  # the plain sum the finalising kernel leaves in the workspace's last word
        runs.append((out.clone(), gb.clone(), ws.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))
                   for a, b in zip(r, runs[0]))
    gs = torch.tensor([-3.0], device=DEV)
    g3 = torch.empty(n, device=DEV)
    assert k_bwd(s, l, scale, g3, gscale=gs) == 0
    assert float((g3.view(shape).double().cpu() + 3.0 * c["g64"]).abs().max()) <= 3.0 * FACTOR * c["grad_err32"]  # the upstream scalar multiplies
    acc = torch.tensor([1.0], device=DEV)
    k_fwd(s, l, scale, out=acc, accumulate=1)
    assert abs(float(acc) - (1.0 + float(v))) <= 2 ** -23 * 2
    for bad in (0, 2, 5):  # only the 3 x 3 window is built
        assert k_bwd(s, l, scale, g3, radius=bad) != 0 and b"radius" in lib.falnet_last_error()
        assert k_fwd(s, l, scale, radius=bad)[0] != 0
    assert lib.falnet_ssim_workspace_bytes(1, 3, 64, 128, 2) == 0 and lib.falnet_ssim_workspace_bytes(1, 3, 64, 128, 1) == 8 * (3 * 4 * 2 + 1)


def test_ssim_loss_through_autograd():
    shape = R.LOSS_SHAPES[3]
    c = loss_case(shape)
    s = c["synth"].to(DEV).requires_grad_(True)
    loss = LF.ssim_loss(s, c["label"].to(DEV))
    (loss * 3.7).backward()
    assert abs(float(loss) - c["v64"]) <= FACTOR * c["map_err32"]
    assert float((s.grad.double().cpu() - 3.7 * c["g64"]).abs().max()) <= 3.7 * FACTOR * c["grad_err32"]
    s2 = c["synth"][:, :1].contiguous().to(DEV).requires_grad_(True)  # one channel: the first mean
    l2 = c["label"][:, :1].contiguous()
    _, v64, g64 = R.loss_and_grad(s2.detach().cpu(), l2)
    _, _, g32 = R.loss_and_grad(s2.detach().cpu(), l2, dtype=torch.float32)
    LF.ssim_loss(s2, l2.to(DEV)).backward()
    assert float((s2.grad.double().cpu() - g64).abs().max()) <= FACTOR * float((g32.double() - g64).abs().max())


# ---- the training step -------------------------------------------------------------------------------------------------------------------------
TOL = 1e-4  # tests/test_gpu_step.py: loss scalars of the f32 path within 1e-4 relative


def sample_idx(key, numel, k=16):
    g = np.random.default_rng(zlib.crc32(("idx:" + key).encode()))
    return g.integers(0, numel, size=min(k, numel))


def build(n_levels, dtype=torch.float32):
    LF.set_compute_dtype(dtype)
    return FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(n_levels)}, no_levels=n_levels, compute_dtype=dtype).to(DEV)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@pytest.fixture(scope="module")
def pair():
    return synthetic.synthetic_pair(2, 64, 128, seed=17, distinct=True)


@pytest.fixture(scope="module")
def oracle(pair):
    """The float64 oracle's Stage-1 losses (as tests/test_gpu_step.py's oracle64 prepares them) plus A_SSIM x the f64 reference loss on its rpan."""
    left, right, mn, mx = pair
    sd = {k: v.double() for k, v in synthetic.seeded_falnetb_state_dict(49).items()}
    vsd = {k: v.double() for k, v in synthetic.seeded_vgg19_state_dict().items()}
    params = O.leaf_params(sd)
    out = O.stage1_losses(params, vsd, left.double(), right.double(), mn.double(), mx.double())
    ssim = R.loss(out["rpan"], right.double())
    rec = out["rec"] + A_SSIM * ssim
    loss = out["loss"] + A_SSIM * ssim
    loss.backward()
    return {"loss": float(loss), "rec": float(rec), "sm": float(out["sm"]), "ssim": float(ssim),
            "grads": {k: p.grad.detach() for k, p in params.items() if p.grad is not None}}


def run_step(pair, dtype, fused, a_ssim=A_SSIM):
    left, right, mn, mx = pair
    m = build(49, dtype).train()
    opt = train.FlatAdam(m, lr=1e-4, betas=(0.5, 0.999))
    old = train._FUSED_STEP
    train._FUSED_STEP = fused
    try:
        out = train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV), optimize=False, a_ssim=a_ssim)
    finally:
        train._FUSED_STEP = old
        LF.set_compute_dtype(torch.float32)
    res = {k: float(out[k]) for k in ("loss", "rec", "sm", "ssim") if k in out}
    res.update(ldisp=out["ldisp"].clone(), rpan=out["rpan"].clone(), flat=m.flat_gradients().clone(),
               grads={k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    return res


@pytest.fixture(scope="module")
def fused32(pair):
    return run_step(pair, torch.float32, True)


def test_fused_step_with_ssim_vs_f64_oracle(fused32, oracle):
    """Bounds of test_stage1_step_vs_golden: loss scalars 1e-4, gradient norms 5e-4, sampled elements 5e-4 of the norm."""
    for k in ("loss", "rec", "sm", "ssim"):
        print(k, fused32[k], oracle[k])
        assert abs(fused32[k] - oracle[k]) / abs(oracle[k]) < TOL, (k, fused32[k], oracle[k])
    for k, g in fused32["grads"].items():
        ref = oracle["grads"][k].reshape(-1)
        gn = float(ref.norm())
        gr = g.reshape(-1)
        assert abs(float(gr.norm()) - gn) / gn < 5e-4, k
        idx = sample_idx(k, gr.numel())
        assert np.abs(gr[idx].cpu().numpy() - ref[idx].numpy()).max() <= 5e-4 * gn + 1e-9, k


def test_fused_step_with_ssim_matches_autograd_form(pair, fused32):
    """Bounds of test_fused_step_matches_autograd_step (f32)."""
    a, f = run_step(pair, torch.float32, False), fused32
    for k in ("loss", "rec", "sm", "ssim"):
        assert abs(a[k] - f[k]) <= 1e-5 * abs(a[k]), (k, a[k], f[k])
    assert rel(f["ldisp"], a["ldisp"]) < 1e-5 and rel(f["rpan"], a["rpan"]) < 1e-5
    ga, gf = a["flat"].double(), f["flat"].double()
    assert float((ga - gf).norm() / ga.norm()) < 1e-4


def test_step_without_the_term_is_unchanged(pair, fused32):
    base = run_step(pair, torch.float32, True, a_ssim=0.0)
    assert "ssim" not in base
    assert abs(fused32["rec"] - (base["rec"] + A_SSIM * fused32["ssim"])) <= 1e-5 * fused32["rec"] and abs(fused32["sm"] - base["sm"]) <= 1e-5 * base["sm"]
    gb, gf = base["flat"].double(), fused32["flat"].double()
    assert float((gf - gb).norm() / gb.norm()) > 1e-2  # the term reaches the parameters


def test_f16_fused_step_with_ssim(pair, fused32):
    """The project's 16-bit criterion: finite, gradient cosine >= 0.999 to the f32 step."""
    h = run_step(pair, torch.float16, True)
    assert all(np.isfinite(h[k]) for k in ("loss", "rec", "sm", "ssim")) and bool(torch.isfinite(h["flat"]).all())
    cos = float(torch.nn.functional.cosine_similarity(h["flat"].double(), fused32["flat"].double(), dim=0))
    print("f16 fused step with the SSIM term: gradient cosine to f32", cos, "ssim", h["ssim"], fused32["ssim"])
    assert cos >= 0.999 and abs(h["ssim"] - fused32["ssim"]) < 2e-2 * fused32["ssim"]


def test_slow_step_with_ssim_matches_its_composition(pair):
    left, right, mn, mx = (t.to(DEV) for t in pair)
    outs = {}
    for a in (0.0, A_SSIM):
        m = build(49).train()
        outs[a] = train.stage1_slow_step(m, train.FlatAdam(m), left, right, mx, a_ssim=a)
    base, out = outs[0.0], outs[A_SSIM]
    assert "ssim" not in base
    term = (LF.ssim_loss(out["rpan"].detach(), right) + LF.ssim_loss(out["lpan"].detach(), left)) / 2
    assert float(out["ssim"]) == float(term) and 0 < float(term) < 1
    assert abs(float(out["rec"]) - (float(base["rec"]) + A_SSIM * float(term))) <= 1e-5 * float(out["rec"])
    assert abs(float(out["loss"]) - (float(out["rec"]) + 0.2 * 2 / 512 * float(out["sm"]))) <= 1e-6 * float(out["loss"])


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------
def test_test_kitti_view_metrics_line(tmp_path):
    outs = {}
    for flag in ((), ("--view-metrics",)):
        save = tmp_path / ("with" if flag else "without")
        cmd = [sys.executable, os.path.join(ROOT, "Test_KITTI.py"), "--synthetic", "--height", "64", "--width", "128", "--iters", "1", "-no_levels", "7",
               "--dtype", "f32", "--save-path", str(save)] + list(flag)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[bool(flag)] = ([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")], save)
    (plain, plain_dir), (lines, save) = outs[False], outs[True]
    assert len(plain) == 1 and len(lines) == 2 and set(lines[-1]) == set(plain[-1]) and not os.path.exists(plain_dir / "view_errors.txt")
    assert all(lines[-1][k] == plain[-1][k] for k in ("image", "dtype", "post"))
    view = lines[0]["view"]
    assert set(view) == {"rmse", "mea", "psnr", "ssim", "n"} and view["n"] == 1
    assert np.isfinite(view["psnr"]) and 0 < view["ssim"] <= 1 and view["rmse"] > 0
    txt = open(save / "view_errors.txt").read()
    assert "ssim" in txt and "{:.4f}".format(view["ssim"]) in txt and lines[0]["file"] == str(save / "view_errors.txt")


def test_zz_report():
    """Prints the figures of this session; FALNET_SSIM_REPORT=<file> also writes them (profiles/ssim_vs_f64.txt is such a file)."""
    text = "".join("{}: {}\n".format(k, json.dumps(v)) for k, v in REPORT.items())
    print(text)
    path = os.environ.get("FALNET_SSIM_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("csrc/ssim.hip against the float64 definition (tests/_ssim_ref.py), per case.  metric: absolute error of a frame's SSIM.  loss: the worst\n"
                    "per-window error of the f32 restatement and the kernel's error of the mean; the worst per-element error of the f32 restatement's\n"
                    "autograd gradient and of the kernel's gradient (the tests allow the kernel {} x the restatement's).\n\n".format(FACTOR) + text)
