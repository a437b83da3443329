"""Reference of the weight packers (fal_net_amd/csrc/pack.hip), the value sets and the case lists of tests/test_pack_host.py and
tests/test_gpu_pack.py.  Written from the layouts documented in include/falnet_hip.h (falnet_pack_weights, falnet_pack_t,
falnet_pack_up2_t) and fal_net_amd.ops.PackedConv, not from the kernels: index arithmetic and torch on the CPU only.

Packing is data movement plus ONE rounding, so the operands are held bit for bit (the tests compare int16 / int32 views):
  wf [cout_pad][taps][cin_pad], wd [cin_pad][taps][cout_pad]: the f32 master converted once with round-to-nearest-even, +0 in the padding;
  wu [cout_pad][16][cin_pad], wdd [cin_pad][4][4 cout_pad]: up to four f32 taps summed in f32 (ky-major, from 0.f), rounded once.
The Adam step fused with the re-pack is held to a float64 step from the device's own pre-step state (ref_adam_step), per element:
  |m - m64| <= 6 u A_m   (u = 2^-24, A_m = b1 |m| + (1 - b1) |gr|: one rounding each for gs, g gs, the two products, the sum, one spare)
  |v - v64| <= 8 u A_v   (A_v = b2 v + (1 - b2) gr^2: the relative error of gr doubles in the square; the square, two products, the sum)
  |p - p64| <= _adam_decay_ref.bound(p64, K=1, lr)
and whatever the Adam arithmetic does, wf / wd must equal the reference of the master AS THE KERNEL LEFT IT, exactly.

CPU stand-in (torch f32 arithmetic in the kernel's operation order, 1 M elements, tests/test_pack_host.py): worst m 0.318, v 0.569,
p 0.476 of the bound; the wrong stand-ins (gradient not scaled / gr where gr^2 belongs / t instead of t + 1) land 2.7e9 / 6.9e11 / 3.0e3 x outside.

Measured on an MI355X (tests/test_gpu_pack.py, every figure printed before it is asserted: run with -s):
  operand elements compared bit for bit, padding included, guards not counted: f32 15 736 832, bf16 112 058 368 (the two models' tables among
  them), f16 17 358 848 -- zero mismatching bits, every guard intact; the f16 extremes (subnormal results, 65519.996 -> 65504, 65520 -> inf)
  come out of the device's conversion as IEEE round-to-nearest-even, so the contract in include/falnet_hip.h stands as written;
  worst bound ratios of the fused Adam over all steps, layers, dtypes, decays, scales and both row orders: m 0.318, v 0.521, p 0.485.
"""
import math

import numpy as np
import torch

import _adam_decay_ref as AR

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
DTYPE_NAME = {F32: "f32", BF16: "bf16", F16: "f16", F64: "f64"}
CPAD = 32
U = 2.0 ** -24
M_ULPS, V_ULPS = 6, 8


def pad_c(c):
    return (c + CPAD - 1) // CPAD * CPAD


# ------------------------------------------------------------------------------------------------------------------ cases
def _kernel(k):
    return (k, k) if isinstance(k, int) else k


def layer_case(name, cout, groups, kernel, what):
    """Geometry of one layer the way ops.PackedConv derives it: one group -> c0_real = cin, c0_pad = cin_pad; two groups -> the first
    group's real / padded size."""
    kh, kw = _kernel(kernel)
    cin = sum(groups)
    pads = [pad_c(g) for g in groups]
    c0_real, c0_pad = (groups[0], pads[0]) if len(groups) == 2 else (cin, sum(pads))
    return dict(name=name, cout=cout, cin=cin, groups=list(groups), kh=kh, kw=kw, taps=kh * kw, c0_real=c0_real, c0_pad=c0_pad,
                cin_pad=sum(pads), cout_pad=pad_c(cout), what=what)


LAYER_CASES = [
    layer_case("a", 32, [32], 3, "one tile"),
    layer_case("b", 64, [3], 3, "conv0: 29 padded columns"),
    layer_case("c", 49, [32, 1], 3, "conv1's shape: second group of one channel, 15 padded rows"),
    layer_case("d", 7, [64, 32], 3, "composed logits, N = 7"),
    layer_case("e", 40, [49, 17], 3, "c0_real < c0_pad with a second group"),
    layer_case("f", 96, [64], 3, "3 x 2 tiles: rel / ctiles against rel % ctiles"),
    layer_case("g", 32, [64], (3, 1), "FAL_netA's separable convs"),
    layer_case("h", 64, [32], (1, 3), "FAL_netA's separable convs"),
    layer_case("i", 64, [49], 1, "the 1x1 logits layer"),
    layer_case("j", 1, [1], 3, "the smallest layer"),
]
BY_NAME = {c["name"]: c for c in LAYER_CASES}
assert all((c["cout_pad"] // 32) * (c["cin_pad"] // 32) <= 9 for c in LAYER_CASES)
UP2_CASES = [(32, 32), (49, 96), (64, 40)]  # (cout, cin) of the sub-pixel layers


def n_blocks(c):
    return (c["cout_pad"] // 32) * (c["cin_pad"] // 32)


# ------------------------------------------------------------------------------------------------------------------ value sets
def normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 0.1


def dyadic(shape, seed):
    """k 2^-10 with |k| <= 4096: any four-term sum is exact in f32, so wu / wdd cannot depend on the order of the additions."""
    k = torch.randint(-4096, 4097, shape, generator=torch.Generator().manual_seed(seed))
    return k.to(F32) * 2.0 ** -10


def _f32_from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.int64).astype(np.uint32).view(np.float32).copy())


def ties(dtype, seed=0, n=3000, moderate=False):
    """f32 masters at the rounding boundaries of the 16-bit type `dtype` (f32 itself: those of bf16 -- the f32 packers copy).
    For n random finite normal 16-bit values h of both signs and their upper neighbour in magnitude h': the f32 midpoint of h and h'
    (an exact tie), the midpoint - 1 f32 ulp, the midpoint + 1 f32 ulp, and h itself; then +0, -0, +-largest finite; for f16 also
    +-65519.996 (the float below 65520: must round to 65504), +-65520 (must round to inf) and normal f32 values in [2^-24, 2^-14) (f16
    subnormal results).  No f32 subnormal, NaN or inf among the masters.  moderate: |h| in [2^-12, 2^12] and no extremes, so that sums of four
    of them stay finite and normal (the sub-pixel weights).  Order: [mid - ulp | mid | mid + ulp | h | extras], each block n long."""
    gen = torch.Generator().manual_seed(1000 + seed)
    if dtype == F16:
        lo, hi = (0x0400 + (3 << 10), 0x0400 + (27 << 10)) if moderate else (0x0400, 0x7bff)  # (hi exclusive: h' stays finite)
        mag = torch.randint(lo, hi, (n,), generator=gen).numpy().astype(np.int64)
        h = mag.astype(np.uint16).view(np.float16).astype(np.float32)
        h2 = (mag + 1).astype(np.uint16).view(np.float16).astype(np.float32)
        mid = (h + h2) * np.float32(0.5)  # 12 significant bits: exact in f32
        assert np.all(mid.astype(np.float64) == (h.astype(np.float64) + h2.astype(np.float64)) / 2)
        mid_bits = mid.view(np.uint32).astype(np.int64)
        h_bits = h.view(np.uint32).astype(np.int64)
        largest = 65504.0
    else:
        lo, hi = (0x0080 + (114 << 7), 0x0080 + (138 << 7)) if moderate else (0x0080, 0x7f7f)
        mag = torch.randint(lo, hi, (n,), generator=gen).numpy().astype(np.int64)
        h_bits = mag << 16
        mid_bits = h_bits + 0x8000
        largest = float(torch.tensor([0x7f7f], dtype=torch.int16).view(BF16).float())
    sign = torch.randint(0, 2, (n,), generator=gen).numpy().astype(np.int64) << 31
    blocks = [_f32_from_bits((mid_bits - 1) | sign), _f32_from_bits(mid_bits | sign), _f32_from_bits((mid_bits + 1) | sign), _f32_from_bits(h_bits | sign)]
    if not moderate:
        extra = [0.0, -0.0, largest, -largest]
        if dtype == F16:
            below = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))
            extra += [below, -below, 65520.0, -65520.0]
            e = torch.rand(64, generator=gen) * 10 - 24  # exponents in [-24, -14)
            sub = (2.0 ** e.double()).float().clamp(2.0 ** -24, float(np.nextafter(np.float32(2.0 ** -14), np.float32(0.0))))
            extra_t = torch.cat([torch.tensor(extra, dtype=F32), sub, -sub])
        else:
            extra_t = torch.tensor(extra, dtype=F32)
        blocks.append(extra_t)
    out = torch.cat(blocks)
    assert bool(torch.isfinite(out).all()) and bool(((out == 0) | (out.abs() >= 2.0 ** -126)).all())
    return out


def fill_from(values, shape, seed):
    """A tensor of `shape` drawn from the 1-D set `values`: every value at least once when it fits, the rest with replacement, shuffled."""
    gen = torch.Generator().manual_seed(2000 + seed)
    n = math.prod(shape)
    idx = torch.randint(0, values.numel(), (n,), generator=gen)
    k = min(n, values.numel())
    idx[:k] = torch.randperm(values.numel(), generator=gen)[:k]
    return values[idx[torch.randperm(n, generator=gen)]].reshape(shape).clone()


def master(case, kind, dtype, seed=0):
    """f32 OIHW master of a layer case; kind: 'normal' | 'ties' | 'dyadic'."""
    shape = (case["cout"], case["cin"], case["kh"], case["kw"])
    seed = seed * 131 + ord(case["name"][0])
    if kind == "normal":
        return normal(shape, seed)
    if kind == "dyadic":
        return dyadic(shape, seed)
    return fill_from(ties(dtype, seed), shape, seed)


def truncate(x, dtype):
    """f32 -> 16-bit by dropping bits (round toward zero): the WRONG conversion a packer could implement."""
    if dtype == BF16:
        return (x.view(torch.int32) >> 16).to(torch.int16).view(BF16)
    r = x.to(F16)
    bits = r.view(torch.int16).clone()
    over = r.float().abs() > x.abs()  # (inf from a finite master included)
    bits[over] -= 1  # one step toward zero in magnitude (sign-magnitude bit patterns)
    return bits.view(F16)


def bits_of(t):
    """Raw bit patterns: int16 view of the 16-bit types, int32 of f32."""
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ------------------------------------------------------------------------------------------------------------------ wf / wd
def ref_wf_wd(w_oihw_f32, c0_real, c0_pad, cin_pad, cout_pad, dtype):
    """(wf [cout_pad][taps][cin_pad], wd [cin_pad][taps][cout_pad], real) -- `real`: bool mask of wf's shape, True where a master element
    lands.  Packed column cp holds real channel cp when cp < c0_real; channel c0_real + (cp - c0_pad) when cp >= c0_pad and that channel
    is < cin; padding (+0) otherwise.  Tap index kh KW + kw.  One conversion of the f32 master to `dtype`, round-to-nearest-even."""
    cout, cin, kh, kw = w_oihw_f32.shape
    taps = kh * kw
    assert c0_real <= c0_pad and c0_real <= cin and c0_pad + (cin - c0_real) <= cin_pad and cout <= cout_pad
    q = w_oihw_f32.reshape(cout, cin, taps).to(dtype)
    wf = torch.zeros(cout_pad, taps, cin_pad, dtype=dtype)
    real = torch.zeros(cout_pad, taps, cin_pad, dtype=torch.bool)
    for cp in range(cin_pad):
        if cp < c0_pad:
            ci = cp if cp < c0_real else -1
        else:
            ci = c0_real + (cp - c0_pad)
            ci = ci if ci < cin else -1
        if ci >= 0:
            wf[:cout, :, cp] = q[:, ci, :]
            real[:cout, :, cp] = True
    return wf, wf.permute(2, 1, 0).contiguous(), real


def ref_case(case, w, dtype):
    return ref_wf_wd(w, case["c0_real"], case["c0_pad"], case["cin_pad"], case["cout_pad"], dtype)


# ------------------------------------------------------------------------------------------------------------------ sub-pixel weights
def row_offset(parity, k):
    """Nearest x2 upsampling then a 'same' 3x3 convolution: output row 2 y + parity reads, through tap k, upsampled row 2 y + parity + k - 1,
    i.e. low-resolution row y + floor((parity + k - 1) / 2)."""
    return (parity + k - 1) // 2  # (Python's floor division)


def up_taps(parity, a):
    """3x3 taps (along one axis) that coincide on the a-th of the two distinct low-resolution offsets of `parity`, in increasing order."""
    offs = sorted({row_offset(parity, k) for k in range(3)})
    assert len(offs) == 2 and offs[1] == offs[0] + 1
    return [k for k in range(3) if row_offset(parity, k) == offs[a]], offs[a]


def adj_taps(d, e):
    """Adjoint along one axis: upstream row Y = 2 (i + d) - 1 + e = 2 y + parity contributes to input row i through the taps k with
    y + row_offset(parity, k) == i."""
    parity = (e + 1) % 2            # Y = 2 (i + d) - 1 + e
    y_minus_i = d + (e - 1 - parity) // 2
    return [k for k in range(3) if y_minus_i + row_offset(parity, k) == 0]


def _tap_sum(w, kys, kxs):
    """f32 sum of the coinciding taps, ky-major, starting from 0.f (so a lone -0 becomes +0, as 0.f + -0.f does)."""
    v = torch.zeros(w.shape[:2], dtype=w.dtype)
    for ky in kys:
        for kx in kxs:
            v = v + w[:, :, ky, kx]
    return v


def ref_wu(w, dtype=None, cin_pad=None, cout_pad=None):
    """wu[co][4 (2 py + px) + 2 a + b][ci] = sum of the taps (ky, kx) that read low-resolution neighbour (a, b) for output parity (py, px).
    Summed in w's own dtype (f32: the kernel's arithmetic; f64: the definition), converted once to `dtype` when given; +0 padding."""
    cout, cin = w.shape[:2]
    cin_pad, cout_pad = cin_pad or pad_c(cin), cout_pad or pad_c(cout)
    out = torch.zeros(cout_pad, 16, cin_pad, dtype=dtype or w.dtype)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    v = _tap_sum(w, up_taps(py, a)[0], up_taps(px, b)[0])
                    out[:cout, 4 * (2 * py + px) + 2 * a + b, :cin] = v.to(out.dtype)
    return out


def ref_wdd(w, dtype=None, cin_pad=None, cout_pad=None):
    """wdd[ci][2 du + dv][(2 e + f) cout_pad + co] = coefficient of upstream pixel (2 (i + du) - 1 + e, 2 (j + dv) - 1 + f) in the gradient
    of input (i, j): the adjoint of ref_wu's layer on the low-resolution grid."""
    cout, cin = w.shape[:2]
    cin_pad, cout_pad = cin_pad or pad_c(cin), cout_pad or pad_c(cout)
    out = torch.zeros(cin_pad, 4, 4 * cout_pad, dtype=dtype or w.dtype)
    for du in range(2):
        for dv in range(2):
            for e in range(2):
                for f in range(2):
                    v = _tap_sum(w, adj_taps(du, e), adj_taps(dv, f))  # [cout][cin]
                    c0 = (2 * e + f) * cout_pad
                    out[:cin, 2 * du + dv, c0:c0 + cout] = v.t().to(out.dtype)
    return out


# ------------------------------------------------------------------------------------------------------------------ Adam
def f32c(x):
    """The f32 value a C float argument receives."""
    return float(np.float32(x))


def ref_adam_step(p, g, m, v, steps, lr, betas=(0.5, 0.999), eps=1e-8, grad_scale=1.0, scaler=None, decay=0.0):
    """One step of torch.optim.Adam (L2 decay: gr = g gs + decay p) in float64 from the f32 state the device held BEFORE the step; t = steps + 1.
    Returns p64, m64, v64, A_m, A_v (the magnitudes the moment bounds scale with)."""
    b1, b2 = f32c(betas[0]), f32c(betas[1])
    gs = f32c(grad_scale) / (float(scaler[0]) if scaler is not None else 1.0)
    t = steps + 1
    p, g, m, v = (x.detach().cpu().to(F64) for x in (p, g, m, v))
    gr = g * gs + decay * p
    m64 = b1 * m + (1 - b1) * gr
    v64 = b2 * v + (1 - b2) * gr * gr
    p64 = p - f32c(lr) / (1 - b1 ** t) * m64 / (v64.sqrt() / math.sqrt(1 - b2 ** t) + f32c(eps))
    return p64, m64, v64, b1 * m.abs() + (1 - b1) * gr.abs(), b2 * v + (1 - b2) * gr * gr


def adam_ratios(p, m, v, ref, lr):
    """Worst |got - ref64| / bound of one step for (m, v, p); an element whose bound is 0 must match exactly."""
    p64, m64, v64, a_m, a_v = ref

    def worst(got, want, bound):
        err = (got.detach().cpu().to(F64).reshape(want.shape) - want).abs()
        r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        return float(r.max()) if r.numel() else 0.0
    return {"m": worst(m, m64, M_ULPS * U * a_m), "v": worst(v, v64, V_ULPS * U * a_v), "p": worst(p, p64, AR.bound(p64, 1, lr))}


def f32_adam_standin(p, g, m, v, steps, lr, betas=(0.5, 0.999), eps=1e-8, grad_scale=1.0, scaler=None, decay=0.0, wrong=None):
    """pack_tile's update written with torch f32 arithmetic on the CPU in the kernel's operation order (the decayed gradient in double,
    rounded once): what stands in for the device in tests/test_pack_host.py.  wrong: 'unscaled' | 'gr_not_squared' | 't_not_plus_1'."""
    f = lambda x: torch.tensor(x, dtype=F32)  # noqa: E731
    b1, b2, eps_, gs = f(betas[0]), f(betas[1]), f(eps), f(grad_scale)
    if scaler is not None:
        gs = gs / f(float(scaler[0]))
    t = f(float(steps)) + (f(0.0) if wrong == "t_not_plus_1" else f(1.0))
    step_size = f(lr) / (f(1.0) - torch.pow(b1, t))
    rsqrt_bc2 = f(1.0) / torch.sqrt(f(1.0) - torch.pow(b2, t))
    if wrong == "unscaled":
        gs = f(1.0)
    if decay:
        gr = (decay * p.double() + g.double() * gs.double()).float()
    else:
        gr = g * gs
    m1 = b1 * m + (f(1.0) - b1) * gr
    v1 = b2 * v + ((f(1.0) - b2) * gr if wrong == "gr_not_squared" else (f(1.0) - b2) * gr * gr)
    p1 = p - step_size * m1 / (torch.sqrt(v1) * rsqrt_bc2 + eps_)
    return p1, m1, v1
