"""GPU: the 4-bit argmax codes of the fused max pool (falnet_conv_t::pool_code, conv3x3_dma16_kernel<PoolCodes<T>, ...>) and the pool backward that reads
them (falnet_maxpool2_bwd_codes), against the kernels that keep the full-resolution map and against float64 autograd, bit for bit; the
argument checks; and the VGG plan built with and without the codes.

Kernel-level inputs are exact in bf16 and f16 and full of ties: x integer in [-2, 2], w in {-1, 0, 1} kept with probability 1/16, bias
integer in [-3, 1] -> integer outputs of magnitude <= ~35, ~15 % of the windows without a positive element, ~5 % with a tied positive maximum
(every test asserts >= 10 % / >= 3 % on its own float64 reference, so that it cannot pass vacuously)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import ops  # noqa: E402
from test_gpu_ops import TOL  # noqa: E402

DEV = "cuda"
f64 = torch.float64
H16 = [torch.bfloat16, torch.float16]
GUARD = 256  # elements in front of and behind every output buffer


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _guarded(shape, dtype, fill):
    """(view of `shape`, guard in front, guard behind) inside one allocation filled with the sentinel."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return flat[GUARD:GUARD + n].view(*shape), flat[:GUARD], flat[GUARD + n:]


def _is_sentinel(t):
    return bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == 0xFF).all())


def _inputs(B, cin, cout, H, W, dtype, seed):
    g = _gen(seed)
    x = torch.randint(-2, 3, (B, H, W, cin), generator=g).float()
    w = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float() * (torch.rand(cout, cin, 3, 3, generator=g) < 1 / 16).float()
    b = torch.randint(-3, 2, (cout,), generator=g).float()
    gy = torch.randn(B, H // 2, W // 2, cout, generator=g).to(dtype)
    wp, bp = torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV))
    pc = ops.PackedConv("t", wp, bp, [cin], 1)
    pc.alloc(dtype, torch.device(DEV))
    pc.pack_call()()
    return x, w, b, gy.to(DEV), pc


def _conv(pc, x_t, dtype, B, H, W, cout, out, pooled, codes=None, variant=23):
    return ops.conv_call(dtype, [ops.nhwc_src(x_t)], H, W, pc.wf, pc.cin_pad, ops.fwd_taps(3), 9, pc.cout_pad, 1, B, H, W, out, H, W, cout, cout,
                         bias=pc.bias, act=L.ACT_RELU, pool_out=pooled, pool_code=codes, variant=variant)


def _window_stats(y):
    """y (B, H, W, C) float64 -> (fraction of windows without a positive element, fraction with a tied positive maximum)."""
    B, H, W, Cc = y.shape
    win = y.view(B, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    mx = win.max(1).values
    tied = ((win == mx[:, None]).sum(1) > 1) & (mx > 0)
    return float((mx <= 0).double().mean()), float(tied.double().mean())


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("H,W", [(16, 32),    # one tile
                                 (40, 96),    # ragged bottom tile
                                 (34, 70)])   # ragged bottom and right, W / 2 odd
@pytest.mark.parametrize("cin,cout", [(64, 64), (128, 128)])  # the second: two 64-channel output blocks, four K chunks
def test_codes_kernel_exact(cin, cout, H, W, dtype):
    B = 2
    x, w, b, gy, pc = _inputs(B, cin, cout, H, W, dtype, seed=H + cin)
    x_t = x.to(dtype).to(DEV)
    lib, st, code = L.lib(), L.stream_ptr(), L.dtype_code(dtype)
    nan = float("nan")
    # the existing kernel: full-resolution map + pooled map
    y_full, yf0, yf1 = _guarded((B, H, W, cout), dtype, nan)
    p_old, po0, po1 = _guarded((B, H // 2, W // 2, cout), dtype, nan)
    old = _conv(pc, x_t, dtype, B, H, W, cout, y_full, p_old)
    assert "conv3x3_dma16_kernelIDF16" in old.tag
    old()
    # the new instantiation: pooled map + codes, no full-resolution map
    p_new, pn0, pn1 = _guarded((B, H // 2, W // 2, cout), dtype, nan)
    codes, c0, c1 = _guarded((B, H // 2, W // 2, cout // 2), torch.uint8, 0xFF)
    new = _conv(pc, x_t, dtype, B, H, W, cout, None, p_new, codes)
    assert "conv3x3_dma16_kernelI9PoolCodes" in new.tag
    new()
    gx_old, go0, go1 = _guarded((B, H, W, cout), dtype, nan)
    gx_new, gn0, gn1 = _guarded((B, H, W, cout), dtype, nan)
    L.check(lib.falnet_maxpool2_bwd(L.ptr(y_full), L.ptr(p_old), L.ptr(gy), L.ptr(gx_old), B, H, W, cout, code, st))
    L.check(lib.falnet_maxpool2_bwd_codes(L.ptr(codes), L.ptr(gy), L.ptr(gx_new), B, H, W, cout, code, st))
    torch.cuda.synchronize()
    for guard in (yf0, yf1, po0, po1, pn0, pn1, c0, c1, go0, go1, gn0, gn1):
        assert _is_sentinel(guard)
    # the stored map is the exact integer convolution (f32 sums of small integers are exact)
    y_ref = F.relu(F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)).permute(0, 2, 3, 1)
    assert torch.equal(y_full.float().cpu(), y_ref)
    y64 = y_full.to(f64).cpu()
    nonpos, tied = _window_stats(y64)
    print(f"windows without a positive element {nonpos:.3f}, with a tied positive maximum {tied:.3f}")
    assert nonpos >= 0.10 and tied >= 0.03
    # pooled maps: bit-identical
    assert torch.equal(p_new.view(torch.int16), p_old.view(torch.int16))
    # codes: every mapped byte written, every nibble one-hot or zero
    cb = codes.cpu()
    for nib in (cb & 15, cb >> 4):
        assert bool(((nib == 0) | (nib == 1) | (nib == 2) | (nib == 4) | (nib == 8)).all())
    # gradients: every element written, bit-identical, and equal to float64 autograd on the stored map
    assert not bool(torch.isnan(gx_new).any()) and not bool(torch.isnan(gx_old).any())
    assert torch.equal(gx_new.view(torch.int16), gx_old.view(torch.int16))
    yr = y64.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(F.relu(yr), 2).backward(gy.to(f64).cpu().permute(0, 3, 1, 2))
    g_ref = yr.grad.permute(0, 2, 3, 1)
    assert torch.equal(gx_new.to(f64).cpu(), g_ref)
    assert torch.equal(gx_old.to(f64).cpu(), g_ref)


def test_argument_checks():
    """Return codes only: nothing is launched."""
    lib, st = L.lib(), L.stream_ptr()
    B, cin, cout, H, W = 1, 64, 64, 16, 32
    buf = C.create_string_buffer(160)

    def refused(call, what):
        assert lib.falnet_conv2d_kernel_name(call.ref, buf, 160) == -2, what
        assert "pool_code" in lib.falnet_last_error().decode(), what
        assert lib.falnet_conv2d(call.ref, st) == -2, what

    dt = torch.bfloat16
    x, w, b, gy, pc = _inputs(B, cin, cout, H, W, dt, seed=1)
    x_t = x.to(dt).to(DEV)
    pooled = torch.empty(B, H // 2, W // 2, cout, dtype=dt, device=DEV)
    codes = torch.empty(B, H // 2, W // 2, cout // 2, dtype=torch.uint8, device=DEV)
    call = _conv(pc, x_t, dt, B, H, W, cout, None, pooled, codes)
    assert lib.falnet_conv2d_kernel_name(call.ref, buf, 160) == 0
    call.desc.variant = 16
    refused(call, "variant 16")
    call.desc.variant = 0
    refused(call, "heuristic variant")
    call.desc.variant = 23
    call.desc.pool_mode = 1
    refused(call, "pool_mode 1")
    call.desc.pool_mode = 0
    assert lib.falnet_conv2d_kernel_name(call.ref, buf, 160) == 0
    with pytest.raises(ValueError):  # ops.conv_call reports it the same way
        _conv(pc, x_t, dt, B, H, W, cout, None, pooled, codes, variant=16)
    # f32
    x32, w32, b32, gy32, pc32 = _inputs(B, cin, cout, H, W, torch.float32, seed=2)
    x32_t = x32.to(DEV)
    pooled32 = torch.empty(B, H // 2, W // 2, cout, dtype=torch.float32, device=DEV)
    old = ops.AUTOTUNE
    ops.AUTOTUNE = False
    try:
        c32 = _conv(pc32, x32_t, torch.float32, B, H, W, cout, None, pooled32, None, variant=None)
    finally:
        ops.AUTOTUNE = old
    c32.desc.pool_code = codes.data_ptr()
    for v in (23, 0, 4):
        c32.desc.variant = v
        refused(c32, f"f32 variant {v}")
    # the unpool entry: odd H / W, C not a multiple of 8
    gx = torch.full((B, H, W, cout), float("nan"), dtype=dt, device=DEV)
    for hh, ww, cc in ((H - 1, W, cout), (H, W - 1, cout), (H, W, 12)):
        assert lib.falnet_maxpool2_bwd_codes(L.ptr(codes), L.ptr(gy), L.ptr(gx), B, hh, ww, cc, L.dtype_code(dt), st) != 0
    assert lib.falnet_maxpool2_bwd_codes(None, L.ptr(gy), L.ptr(gx), B, H, W, cout, L.dtype_code(dt), st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(gx).all())


# ------------------------------------------------------------------------------------------------------------------- plan level
def _vgg_f64(sd, x, gouts):
    """float64 VGG19 features[0:19] in three slices on the CPU: (features, d sum_i <f_i, g_i> / dx)."""
    xr = x.to(f64).clone().requires_grad_(True)
    cur = xr
    feats = []
    for convs in LF._SLICES:
        for i in convs:
            cur = F.relu(F.conv2d(cur, sd[f"features.{i}.weight"].to(f64), sd[f"features.{i}.bias"].to(f64), padding=1))
        cur = F.max_pool2d(cur, 2)
        feats.append(cur)
    sum((f * g.to(f64)).sum() for f, g in zip(feats, gouts)).backward()
    return [f.detach() for f in feats], xr.grad


def _run_plan(plan, x, gouts):
    plan.c3_call.set_input(x)
    plan.run_fwd()
    for buf, g in zip(plan.gouts, gouts):
        buf.copy_(g.permute(0, 2, 3, 1))
    plan.run_bwd()
    torch.cuda.synchronize()
    return [o.clone() for o in plan.outs], plan.g_in.clone()


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("B,H,W,fallback", [(1, 64, 128, ()),      # slice 3 is exactly one 16 x 32 tile
                                            (2, 32, 64, (2,))])   # slice 3 (8 x 16) falls back to the full-resolution form
def test_vgg_plan_codes_vs_full_maps(B, H, W, fallback, dtype):
    """Codes on / off with the SAME conv kernel on both sides (variant 23 forced on the full-resolution side): features and the input gradient
    are bit-identical.  The three feature maps of both forms -- the full-resolution side with its autotuned kernel -- agree with the float64
    F.conv2d VGG within test_gpu_ops.TOL.  (The input gradient against float64 is printed, not asserted: max-pool / ReLU routing under 16-bit
    rounding has no a-priori bound.)"""
    from fal_net_amd import synthetic
    dev = torch.device(DEV, torch.cuda.current_device())
    owner = LF.Vgg19_pc(compute_dtype=dtype)
    owner._prepare(dev, dtype)
    g = _gen(B + H)
    x = torch.rand(B, 3, H, W, generator=g)
    chans = (64, 128, 256)
    gouts = [torch.randn(B, c, H >> (i + 1), W >> (i + 1), generator=g) / c for i, c in enumerate(chans)]
    xd, gd = x.to(dev), [t.to(dev).to(dtype) for t in gouts]
    tune = ops.AUTOTUNE
    ops.AUTOTUNE = False  # the library's own choice for every other launch: at these sizes the autotuner may pick a split-K data gradient, whose
    try:                  # f32 atomics sum in a different order from run to run -- nothing bit-identical could be asked behind it
        with_codes = LF._VggPlan(owner, B, H, W, dtype, dev, need_grad=True, pool_codes=True, pool_variant=23)
        same_kernel = LF._VggPlan(owner, B, H, W, dtype, dev, need_grad=True, pool_codes=False, pool_variant=23)
    finally:
        ops.AUTOTUNE = tune
    assert not any(c.desc.ksplit > 1 for c in with_codes.bwd + same_kernel.bwd if hasattr(c, "desc"))
    autotuned = LF._VggPlan(owner, B, H, W, dtype, dev, need_grad=True, pool_codes=False)
    # the codes plan holds no full-resolution map in front of a pool (except where it fell back); the other form holds all three
    for s in range(3):
        if s in fallback:
            assert with_codes.pool_codes[s] is None and with_codes.pool_maps[s] is not None
        else:
            assert with_codes.pool_maps[s] is None and with_codes.pool_codes[s].dtype == torch.uint8
            assert tuple(with_codes.pool_codes[s].shape) == (B, H >> (s + 1), W >> (s + 1), chans[s] // 2)
        assert same_kernel.pool_codes[s] is None and tuple(same_kernel.pool_maps[s].shape) == (B, H >> s, W >> s, chans[s])
    names = [c.name for c in with_codes.bwd]
    assert sum("falnet_maxpool2_bwd_codes" in n for n in names) == 3 - len(fallback)
    fa, ga = _run_plan(with_codes, xd, gd)
    fb, gb = _run_plan(same_kernel, xd, gd)
    for a, b in zip(fa, fb):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gb).all())
    assert torch.equal(ga, gb)
    fc, gc = _run_plan(autotuned, xd, gd)
    sd = synthetic.seeded_vgg19_state_dict()
    f_ref, g_ref = _vgg_f64(sd, x, [t.float().cpu() for t in gd])
    for s in range(3):
        ea, ec = _rel(fa[s].permute(0, 3, 1, 2), f_ref[s]), _rel(fc[s].permute(0, 3, 1, 2), f_ref[s])
        print(f"slice {s + 1}: codes {ea:.3e}, full maps (autotuned) {ec:.3e}")
        assert ea < TOL[dtype] and ec < TOL[dtype]
    print(f"input gradient vs float64: codes {_rel(ga, g_ref):.3e}, full maps (autotuned) {_rel(gc, g_ref):.3e}")


def test_vgg_plan_f32_keeps_the_full_maps():
    """f32: no slice has the codes kernel; the plan is the full-resolution one whatever the switch says."""
    dev = torch.device(DEV, torch.cuda.current_device())
    owner = LF.Vgg19_pc(compute_dtype=torch.float32)
    owner._prepare(dev, torch.float32)
    plan = LF._VggPlan(owner, 1, 32, 64, torch.float32, dev, need_grad=True, pool_codes=True)
    assert plan.pool_codes == [None, None, None] and all(m is not None for m in plan.pool_maps)
    assert not any("codes" in c.name for c in plan.bwd)
