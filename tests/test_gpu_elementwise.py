"""The layer-glue kernels of csrc/elementwise.hip through the C-ABI, element by element against exact or float64 references, at the sizes
where they take another path: beyond the grid cap of ew_grid (8192 blocks x 256 threads = 2 097 152 threads: the second trip of every
grid-stride loop, with a ragged end), the vector and the scalar form of maxpool2_bwd (C % 8 and the 16-byte alignment test), the scalar
store path of nchw_to_nhwc (Cpad % 8 != 0), both forms of gemm_f32_small and the limits between them.

Every destination is NaN before its launch and has a NaN guard behind it; a refused call must return non-zero and write nothing.
Bounds (u_T: unit roundoff of the stored type, u = 2^-24; all derived, none measured):
  act_bwd       ELU: (u_T + 3 u) |ref| -- y + 1, the product and the store, each rounded once.  ReLU: exact.
  maxpool2      forward exact; backward exact (a routed gradient is a copied value) against float64 autograd of relu -> max_pool2d.
  upsample_bwd  u_T |ref| + (k + 2) u mag for k summed taps, mag = the same sum over |g| (the taps may cancel).
  layout        exact: to f32 a copy, to 16 bits tensor.to(dtype).
  gemm          (K + 1) u sum_k |a| |b| (+ |c| when accumulating).
  resize        nearest exact; bilinear 6 u sum |w| |v| at sizes whose source coordinates (H - 1) / (OH - 1) x index are exact in float32
                (the bound counts the six roundings of the blend, not a coordinate error; tests/test_gpu_ops.py holds a ragged ratio).
An f16 store of a value below 2^-14 is subnormal: spacing 2^-24, so half of that is added for f16."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402

DEV = "cuda"
NAN = float("nan")
f64 = torch.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUB = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
U32 = 2.0 ** -24
CAP = 8192 * 256  # threads of the largest grid ew_grid launches
P = L.ptr


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _guarded(n, dtype, guard):
    """NaN-filled flat buffer of n + guard elements on the device: (the n elements, the guard)."""
    flat = torch.full((n + guard,), NAN, dtype=dtype, device=DEV)
    return flat[:n], flat[n:]


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _within(got, ref, bound):
    got = got.detach().cpu().to(f64)
    err = (got - ref).abs()
    ok = err <= bound  # NaN fails
    return int((~ok).sum()), float(torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bound.clamp_min(1e-300)).max())


def _nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype)


def _offset_copy(t, elems):
    """The same tensor on the device, `elems` elements into a fresh allocation (an 8-byte offset breaks the 16-byte alignment test)."""
    flat = torch.empty(t.numel() + elems, dtype=t.dtype, device=DEV)
    v = flat[elems:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


# ------------------------------------------------------------------------------------------------------------------- act_bwd
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 257, CAP + 257])
def test_act_bwd(n, dtype):
    """n = CAP + 257: the second trip of the grid-stride loop, ragged.  Planted: y = 0, y just below 0, y = -1 + ulp, g = 0."""
    g = _gen(n)
    y = (torch.rand(n, generator=g) * 4 - 1).to(dtype)
    gr = torch.randn(n, generator=g).to(dtype)
    fi = torch.finfo(dtype)
    planted = [0.0, -fi.tiny, -(1.0 - fi.eps / 2), 0.5]
    for i, v in enumerate(planted[:n]):
        y[(i * 97) % n] = v
    if n > 3:
        gr[(3 * 97) % n] = 0.0
        assert float(y[(2 * 97) % n]) == -(1.0 - fi.eps / 2) and float(y[97]) < 0.0
    yd, gd = y.to(DEV), gr.to(DEV)
    y64, g64 = y.to(f64), gr.to(f64)
    for kind, ref in ((L.ACT_ELU, g64 * torch.where(y64 > 0, torch.ones_like(y64), y64 + 1)), (L.ACT_RELU, g64 * (y64 > 0))):
        gx, guard = _guarded(n, dtype, 1)
        L.check(L.lib().falnet_act_bwd(P(gd), P(yd), P(gx), n, kind, L.dtype_code(dtype), L.stream_ptr()))
        if kind == L.ACT_RELU:
            assert torch.equal(gx.cpu().to(f64), ref)
        else:
            bad, worst = _within(gx, ref, (U[dtype] + 3 * U32) * ref.abs() + SUB[dtype])
            assert bad == 0, (bad, worst)
        assert _all_nan(guard)


# ------------------------------------------------------------------------------------------------------------------- maxpool2
def _untied(B, C, H, W, seed):
    """(B, C, H, W) f32 whose 2x2 windows hold a random arrangement of four distinct levels (-1, 1, 2, 3) x 2^e: no window ties, in
    any of the dtypes (every value is a small dyadic number), some inputs negative."""
    g = _gen(seed)
    OH, OW = H // 2, W // 2
    perm = torch.rand(B, C, OH, OW, 4, generator=g).argsort(-1)
    lv = torch.tensor([-1.0, 1.0, 2.0, 3.0])[perm] * 2.0 ** torch.randint(-2, 3, (B, C, OH, OW, 1), generator=g)
    x = torch.zeros(B, C, H, W)
    x[:, :, :2 * OH, :2 * OW] = lv.view(B, C, OH, OW, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * OH, 2 * OW)
    return x


def _pool_ref(x, gy, dev="cpu"):
    """float64 autograd of relu -> max_pool2d: (pooled, d / dx)."""
    x64 = x.to(dev).to(f64).requires_grad_(True)
    p = F.max_pool2d(F.relu(x64), 2)
    p.backward(gy.to(dev).to(f64))
    return p.detach(), x64.grad


def _run_pool(x, gy, dtype, offset=0):
    """x (B, C, H, W), gy (B, C, H/2, W/2) as stored values of `dtype` -> (pooled, gx) from the kernels, NCHW float64 on the CPU."""
    B, C, H, W = x.shape
    lib, st, code = L.lib(), L.stream_ptr(), L.dtype_code(dtype)
    xt, gt = _nhwc(x, dtype), _nhwc(gy, dtype)
    xd, gd = (_offset_copy(xt, offset), _offset_copy(gt, offset)) if offset else (xt.to(DEV), gt.to(DEV))
    y, yguard = _guarded(gt.numel(), dtype, 8)
    L.check(lib.falnet_maxpool2_fwd(P(xd), P(y), B, H, W, C, code, st))
    flat = torch.full((xt.numel() + offset + 8,), NAN, dtype=dtype, device=DEV)
    gx, gguard = flat[offset:offset + xt.numel()], flat[offset + xt.numel():]
    L.check(lib.falnet_maxpool2_bwd(P(xd), P(y), P(gd), P(gx), B, H, W, C, code, st))
    assert _all_nan(yguard) and _all_nan(gguard) and _all_nan(flat[:offset])
    return (y.view(B, H // 2, W // 2, C).permute(0, 3, 1, 2).to(f64), gx.view(B, H, W, C).permute(0, 3, 1, 2).to(f64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,H,W,offset", [(2, 64, 8, 12, 0),    # vector form (C % 8 == 0, aligned)
                                            (2, 64, 8, 12, 8),    # the same tensors 8 bytes off: scalar form by the alignment test
                                            (1, 12, 6, 10, 0)])   # scalar form by C % 8
def test_maxpool2_forms(B, C, H, W, offset, dtype):
    x = _untied(B, C, H, W, seed=C + offset).to(dtype).float()
    gy = torch.randn(B, C, H // 2, W // 2, generator=_gen(7)).to(dtype).float()
    p_ref, g_ref = _pool_ref(x, gy)
    p, gx = _run_pool(F.relu(x), gy, dtype, offset // x.to(dtype).element_size())
    assert torch.equal(p.cpu(), p_ref)
    assert torch.equal(gx.cpu(), g_ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,offset", [(64, 0), (64, 8), (12, 0)])
def test_maxpool2_bwd_ties_and_non_positive_windows(C, offset, dtype):
    """Four windows per channel: a four-way tie (aten routes to the first in row-major order), a two-way tie on the second row, an
    all-zero window and an all-negative one (both: zero gradient everywhere)."""
    x = torch.zeros(1, C, 4, 4)
    x[:, :, 0:2, 0:2] = 2.0
    x[:, :, 0:2, 2:4] = torch.tensor([[1.0, 0.5], [3.0, 3.0]])
    x[:, :, 2:4, 2:4] = torch.tensor([[-1.0, -2.0], [-0.5, -3.0]])
    gy = (torch.arange(C * 4, dtype=torch.float32).view(1, C, 2, 2) % 13 + 1) / 4
    p_ref, g_ref = _pool_ref(x, gy)
    expect = torch.zeros(1, C, 4, 4, dtype=f64)
    expect[:, :, 0, 0] = gy[:, :, 0, 0].to(f64)
    expect[:, :, 1, 2] = gy[:, :, 0, 1].to(f64)
    assert torch.equal(g_ref, expect)  # the rule the kernel is held to is aten's
    p, gx = _run_pool(x, gy, dtype, offset // x.to(dtype).element_size())  # (the raw tensor: the kernel sees the negative window)
    assert torch.equal(gx.cpu(), expect)
    assert torch.equal(p.cpu(), F.max_pool2d(x, 2).to(f64))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_maxpool2_beyond_the_grid_cap(dtype):
    """B = 2, 256 x 258, C = 64, 8 bytes off 16-byte alignment: 2 113 536 outputs > CAP in the forward and in the scalar backward (each
    thread of the first 16 384 takes a second trip)."""
    B, C, H, W = 2, 64, 256, 258
    assert B * (H // 2) * (W // 2) * C > CAP
    x = _untied(B, C, H, W, seed=11)
    gy = torch.randn(B, C, H // 2, W // 2, generator=_gen(12)).to(dtype).float()
    p_ref, g_ref = _pool_ref(x, gy, DEV)
    p, gx = _run_pool(F.relu(x), gy, dtype, 4)
    assert torch.equal(p, p_ref)
    assert torch.equal(gx, g_ref)


def test_maxpool2_odd_sizes():
    """Forward: F.max_pool2d's floor behaviour.  Backward: refused with a non-zero return, gx untouched."""
    lib, st = L.lib(), L.stream_ptr()
    for dtype in DTYPES:
        for H, W in ((5, 7), (4, 7), (5, 6)):
            x = _untied(2, 16, H, W, seed=H * 10 + W)
            x[:, :, 2 * (H // 2):, :] = 9.0  # the row / column the pool must ignore holds the largest values
            x[:, :, :, 2 * (W // 2):] = 9.0
            xt = _nhwc(x, dtype).to(DEV)
            y, guard = _guarded(2 * (H // 2) * (W // 2) * 16, dtype, 8)
            L.check(lib.falnet_maxpool2_fwd(P(xt), P(y), 2, H, W, 16, L.dtype_code(dtype), st))
            assert torch.equal(y.view(2, H // 2, W // 2, 16).permute(0, 3, 1, 2).float().cpu(), F.max_pool2d(x, 2)) and _all_nan(guard)
            gx = torch.full_like(xt, NAN)
            assert lib.falnet_maxpool2_bwd(P(xt), P(y), P(y), P(gx), 2, H, W, 16, L.dtype_code(dtype), st) != 0
            torch.cuda.synchronize()
            assert _all_nan(gx)


# ------------------------------------------------------------------------------------------------------------------- upsample_bwd
def _upsample_ref(gup, y, H, W, dev="cpu"):
    """gup (B, C, IH, IW), y (B, C, H, W) or None, stored values -> float64 (ref, mag): autograd of F.interpolate(nearest) times ELU's
    derivative from the stored output y; mag the same with |gup|."""
    B, C, IH, IW = gup.shape
    g64 = gup.to(dev).to(f64)
    z = torch.zeros(B, C, H, W, dtype=f64, device=dev, requires_grad=True)
    up = F.interpolate(z, size=(IH, IW), mode="nearest")
    ref, = torch.autograd.grad((up * g64).sum(), z, retain_graph=True)
    mag, = torch.autograd.grad((up * g64.abs()).sum(), z)
    if y is not None:
        y64 = y.to(dev).to(f64)
        d = torch.where(y64 > 0, torch.ones_like(y64), y64 + 1)
        ref, mag = ref * d, mag * d
    return ref, mag


UPSAMPLE_CASES = [(2, 32, 6, 12, 12, 24),   # exact 2x in both axes (the deconv blocks)
                  (1, 8, 5, 7, 5, 7),       # identity
                  (1, 8, 4, 5, 12, 15),     # 3x
                  (2, 32, 6, 12, 11, 23)]   # ragged 11/6, 23/12


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_act", [True, False])
@pytest.mark.parametrize("B,C,H,W,IH,IW", UPSAMPLE_CASES)
def test_upsample_bwd(B, C, H, W, IH, IW, with_act, dtype):
    g = _gen(IH * 100 + IW)
    gup = torch.randn(B, C, IH, IW, generator=g).to(dtype).float()
    y = F.elu(torch.randn(B, C, H, W, generator=g)).to(dtype).float() if with_act else None
    # F.interpolate's nearest map is floor(i * H / IH) in integers for these sizes (what the kernel inverts)
    idx = F.interpolate(torch.arange(H * W, dtype=f64).view(1, 1, H, W), size=(IH, IW), mode="nearest").long()
    iy, ix = torch.arange(IH) * H // IH, torch.arange(IW) * W // IW
    assert torch.equal(idx[0, 0], iy.view(-1, 1) * W + ix.view(1, -1))
    ref, mag = _upsample_ref(gup, y, H, W)
    k = -(-IH // H) * -(-IW // W)
    gt = _nhwc(gup, dtype).to(DEV)
    yt = _nhwc(y, dtype).to(DEV) if with_act else None
    out, guard = _guarded(B * H * W * C, dtype, 8)
    L.check(L.lib().falnet_upsample_bwd(P(gt), P(out), P(yt), B, IH, IW, H, W, C, L.dtype_code(dtype), L.stream_ptr()))
    got = out.view(B, H, W, C).permute(0, 3, 1, 2)
    bad, worst = _within(got, ref, U[dtype] * ref.abs() + (k + 2) * U32 * mag + SUB[dtype])
    assert bad == 0 and _all_nan(guard), (bad, worst)


def test_upsample_bwd_beyond_the_grid_cap_and_refusals():
    """1025 x 2047 pixels of 8 channels: one thread per pixel, 2 098 175 > CAP, the last 1023 on the second trip (2x in H, identity in W,
    with actout).  Refused without a write: C = 12, and a width whose index products W x IW leave 32 bits (the kernel's column ranges
    ((s + 1) IW + W - 1) / W are int: W = IW = 2 097 157 read far outside gup before the entry point refused such sizes)."""
    dtype, B, C, H, W, IH, IW = torch.bfloat16, 1, 8, 1025, 2047, 2050, 2047
    assert B * H * W * (C // 8) > CAP
    g = torch.Generator(device=DEV).manual_seed(5)
    gt = torch.randn(B, IH, IW, C, generator=g, device=DEV).to(dtype)
    yt = F.elu(torch.randn(B, H, W, C, generator=g, device=DEV)).to(dtype)
    ref, mag = _upsample_ref(gt.permute(0, 3, 1, 2), yt.permute(0, 3, 1, 2), H, W, DEV)
    out, guard = _guarded(B * H * W * C, dtype, 8)
    lib, st, code = L.lib(), L.stream_ptr(), L.dtype_code(dtype)
    L.check(lib.falnet_upsample_bwd(P(gt), P(out), P(yt), B, IH, IW, H, W, C, code, st))
    got = out.view(B, H, W, C).permute(0, 3, 1, 2).to(f64)
    err = (got - ref).abs()
    assert bool((err <= U[dtype] * ref.abs() + 4 * U32 * mag).all()) and _all_nan(guard)
    small = torch.full((1, 2, 2, 12), NAN, dtype=dtype, device=DEV)
    assert lib.falnet_upsample_bwd(P(gt), P(small), P(None), 1, 2, 2, 2, 2, 12, code, st) != 0
    wide = torch.full((46341 * 8,), NAN, dtype=dtype, device=DEV)
    assert lib.falnet_upsample_bwd(P(gt), P(wide), P(None), 1, 1, 46341, 1, 46341, 8, code, st) != 0
    assert lib.falnet_upsample_bwd(P(gt), P(wide), P(None), 1, 46341, 1, 46341, 1, 8, code, st) != 0
    torch.cuda.synchronize()
    assert _all_nan(small) and _all_nan(wide)


# ------------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,Cpad", [(5, 5),       # Cpad % 8 != 0: the scalar store path
                                    (3, 32),      # the workload's input
                                    (512, 512)])  # the largest the guard admits: 64 x 513 floats of LDS
def test_layout_conversions(C, Cpad, dtype):
    """HW in {1, 63, 64, 65}: below, at and one past the 64-pixel tile.  To f32 a copy, to 16 bits tensor.to(dtype); padding channels
    exactly zero; the NaN row behind each destination untouched; padding channels of the source never reach the planar result."""
    lib, st, code = L.lib(), L.stream_ptr(), L.dtype_code(dtype)
    for HW in (1, 63, 64, 65):
        B, H, W = 2, 1, HW
        src = torch.randn(B, C, H, W, generator=_gen(C * 100 + HW))
        srcd = src.to(DEV)
        dst, guard = _guarded(B * HW * Cpad, dtype, Cpad)
        L.check(lib.falnet_nchw_to_nhwc(P(srcd), P(dst), B, C, H, W, Cpad, code, st))
        d = dst.view(B, HW, Cpad)
        assert torch.equal(d[..., :C].cpu(), src.view(B, C, HW).permute(0, 2, 1).to(dtype))
        assert Cpad == C or bool((d[..., C:] == 0).all())
        assert _all_nan(guard)
        back_src = d.clone()
        back_src[..., C:] = 7.0
        back, bguard = _guarded(B * C * HW, torch.float32, 64)
        L.check(lib.falnet_nhwc_to_nchw(P(back_src), P(back), B, C, H, W, Cpad, code, st))
        assert torch.equal(back.view(B, C, HW).cpu(), src.to(dtype).float().view(B, C, HW))
        assert _all_nan(bguard)
    one = torch.zeros(1, 513, 1, 1, device=DEV)
    out = torch.full((513,), NAN, dtype=dtype, device=DEV)
    assert lib.falnet_nchw_to_nhwc(P(one), P(out), 1, 513, 1, 1, 513, code, st) != 0  # beyond the guard: refused
    torch.cuda.synchronize()
    assert _all_nan(out)


# ------------------------------------------------------------------------------------------------------------------- gemm_f32_small
def _gemm_case(M, N, K, ta, tb, accumulate, seed):
    g = _gen(seed)
    a, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    c0 = torch.randn(M, N, generator=g)
    ad = (a.t().contiguous() if ta else a).to(DEV)  # stored [K][M] when ta
    bd = (b.t().contiguous() if tb else b).to(DEV)  # stored [N][K] when tb
    sam, sak = (1, M) if ta else (K, 1)
    sbk, sbn = (1, K) if tb else (N, 1)
    c, guard = _guarded(M * N, torch.float32, 8)
    if accumulate:
        c.copy_(c0.view(-1))
    L.check(L.lib().falnet_gemm_f32_small(P(ad), sam, sak, P(bd), sbk, sbn, P(c), M, N, K, accumulate, L.stream_ptr()))
    ref = a.to(f64) @ b.to(f64) + (c0.to(f64) if accumulate else 0)
    mag = a.abs().to(f64) @ b.abs().to(f64) + (c0.abs().to(f64) if accumulate else 0)
    bad, worst = _within(c.view(M, N), ref, (K + 1) * U32 * mag)
    assert bad == 0 and _all_nan(guard), (M, N, K, ta, tb, accumulate, bad, worst)


def test_gemm_f32_small_thread_and_wave_forms():
    """K in {1, 7, 8, 9, 255}: thread-per-output form with 8-step unroll tails of 1, 7, 0, 1, 7; K in {256, 257, 864}: wave-per-output
    form with a full, a one-element and a 32-element last lane trip.  Both operands in either storage order, accumulate 0 and 1."""
    i = 0
    for K in (1, 7, 8, 9, 255, 256, 257, 864):
        for ta, tb in ((0, 0), (1, 0), (0, 1), (1, 1)):
            _gemm_case(5, 7, K, ta, tb, i & 1, seed=i)
            _gemm_case(49, 49 if K >= 256 else 3, K, ta, tb, 1 - (i & 1), seed=100 + i)
            i += 1


def test_gemm_f32_small_limits():
    """M N in {1, 65 536, 65 537} at K = 256: one wave, the wave form's limit, and the fall back to the thread form just above it (a
    65 537 x 1 product whose A is a Hankel view, strides (1, 1), of K + 65 536 floats -- every stride pair is legal); M N K > 2^32 refused."""
    lib, st = L.lib(), L.stream_ptr()
    _gemm_case(1, 1, 256, 0, 0, 0, seed=1)
    _gemm_case(256, 256, 256, 0, 1, 1, seed=2)
    M, K = 65537, 256
    g = _gen(3)
    buf, b = torch.randn(M + K - 1, generator=g), torch.randn(K, generator=g)
    ref = F.conv1d(buf.to(f64).view(1, 1, -1), b.to(f64).view(1, 1, -1)).view(-1)
    mag = F.conv1d(buf.abs().to(f64).view(1, 1, -1), b.abs().to(f64).view(1, 1, -1)).view(-1)
    bufd, bd = buf.to(DEV), b.to(DEV)
    c, guard = _guarded(M, torch.float32, 8)
    L.check(lib.falnet_gemm_f32_small(P(bufd), 1, 1, P(bd), 1, 0, P(c), M, 1, K, 0, st))
    bad, worst = _within(c, ref, (K + 1) * U32 * mag)
    assert bad == 0 and _all_nan(guard), (bad, worst)
    c = torch.full((4,), NAN, device=DEV)
    assert lib.falnet_gemm_f32_small(P(bufd), 1, 1, P(bd), 1, 0, P(c), 2048, 2048, 2048, 0, st) != 0
    torch.cuda.synchronize()
    assert _all_nan(c)


# ------------------------------------------------------------------------------------------------------------------- disp_prologue
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 64, 65])
def test_disp_prologue(B, dtype):
    """min_disp given and derived (mx * mul / div, the same float32 expression on the CPU: exact); flow written at flow_stride only."""
    lib, st, code = L.lib(), L.stream_ptr(), L.dtype_code(dtype)
    mx = torch.rand(B, generator=_gen(B)) * 250 + 20
    mn = torch.rand(B, generator=_gen(B + 1)) * 3 + 0.5
    stride = 3
    for given in (True, False):
        mn_out, g1 = _guarded(B, torch.float32, 4)
        mx_out, g2 = _guarded(B, torch.float32, 4)
        flow = torch.full((B * stride + 2,), NAN, dtype=dtype, device=DEV)
        mxd, mnd = mx.to(DEV), mn.to(DEV)
        L.check(lib.falnet_disp_prologue(P(mxd), P(mnd if given else None), 2.0, 300.0, P(mn_out), P(mx_out), P(flow), stride, B, code, st))
        assert torch.equal(mn_out.cpu(), mn if given else mx * 2.0 / 300.0)
        assert torch.equal(mx_out.cpu(), mx)
        f = flow[:B * stride].view(B, stride)
        assert torch.equal(f[:, 0].cpu(), (mx / 100.0).to(dtype))
        assert _all_nan(f[:, 1:]) and _all_nan(flow[B * stride:]) and _all_nan(g1) and _all_nan(g2)
    mn_out, _ = _guarded(B, torch.float32, 4)
    mx_out, _ = _guarded(B, torch.float32, 4)
    assert lib.falnet_disp_prologue(P(mxd), P(None), 2.0, 0.0, P(mn_out), P(mx_out), P(flow), stride, B, code, st) != 0
    torch.cuda.synchronize()
    assert _all_nan(mn_out) and _all_nan(mx_out)


# ------------------------------------------------------------------------------------------------------------------- resize_planar
def _resize(src, OH, OW, bilinear, scale=1.0):
    planes, H, W = src.shape
    dst, guard = _guarded(planes * OH * OW, torch.float32, 8)
    L.check(L.lib().falnet_resize_planar(P(src), P(dst), planes, H, W, OH, OW, int(bilinear), scale, L.stream_ptr()))
    assert _all_nan(guard)
    return dst.view(planes, OH, OW)


def _resize_check(src, OH, OW):
    """bilinear within 6 u sum |w| |v| of float64 F.interpolate(align_corners=True); nearest exact."""
    s64 = src.to(f64).unsqueeze(0)
    ref = F.interpolate(s64, size=(OH, OW), mode="bilinear", align_corners=True)[0]
    mag = F.interpolate(s64.abs(), size=(OH, OW), mode="bilinear", align_corners=True)[0]
    bad, worst = _within(_resize(src, OH, OW, True), ref.cpu(), 6 * U32 * mag.cpu())
    assert bad == 0, (tuple(src.shape), OH, OW, bad, worst)
    near = F.interpolate(src.unsqueeze(0), size=(OH, OW), mode="nearest")[0]
    assert torch.equal(_resize(src, OH, OW, False), near)


def test_resize_planar_edges():
    """One output row / column (source index 0 along that axis: a copy of the first row / column in both modes), the identity size
    bit-exact in both modes, exact-coordinate ratios (1/2, 2, 3/4), and 2 100 planes of 33 x 33 outputs: 2 286 900 > CAP, the second
    trip of the loop."""
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randn(6, 9, 13, generator=g, device=DEV)
    for bil in (True, False):
        assert torch.equal(_resize(x, 1, 13, bil), x[:, :1, :])
        assert torch.equal(_resize(x, 9, 1, bil), x[:, :, :1])
        assert torch.equal(_resize(x, 1, 1, bil), x[:, :1, :1])
        assert torch.equal(_resize(x, 9, 13, bil), x)
        assert torch.equal(_resize(x, 9, 13, bil, 1.5), x * 1.5)
    _resize_check(x, 17, 25)                                               # ratio 1/2 in both axes
    _resize_check(x, 1, 25)
    _resize_check(x, 17, 1)
    _resize_check(torch.randn(3, 17, 25, generator=g, device=DEV), 9, 13)  # ratio 2
    _resize_check(torch.randn(3, 4, 7, generator=g, device=DEV), 5, 9)     # ratio 3/4
    assert 2100 * 33 * 33 > CAP
    _resize_check(torch.randn(2100, 17, 17, generator=g, device=DEV), 33, 33)
