"""Float64 reference of ONE falnet_wgrad launch and of the bias gradient, written from the falnet_wgrad_t contract in
include/falnet_hip.h, not from the kernels; the integer operand generator that makes every weight-gradient sum EXACT in f32; and the
float64 sum of raw split slabs.

Why integers: dW[co, tap, ci] = sum_p gout[p, co] * in[nbr(p, tap), ci] accumulates in f32.  With sources in [0, 15] and the output
gradient in [-7, 8] (both exact in bf16, f16 and f32) every product and every partial sum is an integer below 2^24 as long as
n * max|x| * max|g| < 2^24 (n = positions summed), so the result does not depend on summation order, split count, MFMA shape or the
order of f32 atomics: the tests compare with torch.equal and need no tolerance.  assert_exact() checks that condition.

wgrad_ref() works in torch float64 on the device of its operands (one GEMM per tap), so a GPU test runs it through the BLAS library.

The `desc` dict (the descriptor's fields under the names of falnet_wgrad_t, plus what the slab reduce needs):
  B, TH, TW, IH, IW, stride, taps [(dy, dx), ...], gC, cout, cin_total,
  srcs  [{"C": channels consumed, "form": "nhwc" | "bcast" | "planar"}, ...]   (an NHWC source may be at half the launch size),
  up2   (optional) != 0: gout at [B][2 TH][2 TW][gC], the one source at TH x TW; the result is the full 3x3 gradient through nearest x2,
  cin, c0_real, c0_pad: the channel groups of falnet_wgrad_reduce (packed column cp holds real channel cp for cp < c0_real, or
  c0_real + (cp - c0_pad) for cp >= c0_pad).
"""
import torch

X_RANGE = (0, 15)   # sources
G_RANGE = (-7, 8)   # output gradient
EXACT_LIMIT = 2 ** 24
F64 = torch.float64


def int_operand(shape, lo, hi, seed, dtype=torch.float32, device="cpu"):
    """Integers in [lo, hi] (inclusive), drawn on the CPU from a seeded generator, stored as `dtype` on `device`."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(dtype).to(device)


def assert_exact(n, xmax, gmax, unit=1.0):
    """The exactness condition: with operands that are multiples of `unit`, n positions, |x| <= xmax and |g| <= gmax, every partial sum
    is a multiple of `unit` of magnitude below 2^24 units.  Returns the bound (in units)."""
    bound = n * (xmax / unit) * gmax
    assert bound < EXACT_LIMIT, f"sums are not exact in f32: n={n} max|x|={xmax} max|g|={gmax} unit={unit}: {bound} >= 2^24"
    return bound


def positions(desc):
    """n = positions one weight-gradient element is summed over."""
    return desc["B"] * desc["TH"] * desc["TW"] * (4 if desc.get("up2") else 1)


def nearest_index(n_out, n_src, device):
    """Source index of F.interpolate(mode='nearest'): floor(i * n_src / n_out) (tests/_conv_ref.py: _virtual_input)."""
    return torch.div(torch.arange(n_out, device=device) * n_src, n_out, rounding_mode="floor")


def virtual_input(src, form, IH, IW):
    """[B][IH][IW][C] float64 view of one source: NHWC at the launch size or nearest-upsampled to it, a per-sample constant [B][C]
    broadcast, or the planar f32 image [B][3][IH][IW] of variant 6."""
    src = src.to(F64)
    if form == "bcast":
        B, Cc = src.shape
        return src.view(B, 1, 1, Cc).expand(B, IH, IW, Cc)
    if form == "planar":
        assert src.shape[1] == 3 and tuple(src.shape[2:]) == (IH, IW)
        return src.permute(0, 2, 3, 1)
    assert form == "nhwc", form
    _, H, W, _ = src.shape
    if (H, W) != (IH, IW):
        src = src[:, nearest_index(IH, H, src.device)][:, :, nearest_index(IW, W, src.device)]
    return src


def packed_input(desc, srcs):
    """[B][IH][IW][cin_total] float64: the sources side by side on the packed channel axis (a planar image fills columns 0..2 of its
    32-column group, the rest of the group is zero)."""
    IH, IW = desc["IH"], desc["IW"]
    cols = []
    for t, s in zip(srcs, desc["srcs"]):
        v = virtual_input(t, s["form"], IH, IW)
        if s["form"] == "planar":
            pad = torch.zeros(*v.shape[:3], desc["cin_total"] - 3, dtype=F64, device=v.device)
            v = torch.cat([v, pad], dim=3)
        else:
            v = v[..., :s["C"]]
        cols.append(v)
    xin = torch.cat(cols, dim=3)
    assert xin.shape[3] == desc["cin_total"], (xin.shape, desc["cin_total"])
    return xin


def unpack_columns(desc):
    """Packed column of every real input channel (the inverse of the slab reduce's un-padding)."""
    cin, c0_real, c0_pad = desc["cin"], desc["c0_real"], desc["c0_pad"]
    return [ci if ci < c0_real else c0_pad + (ci - c0_real) for ci in range(cin)]


def wgrad_ref(desc, srcs, gout, tap_shift=None, drop_last_column=False, swap_groups=False):
    """(slab, oihw): dW[tap][co][packed ci] float64 [ntaps][gC][cin_total] and the un-padded gradient [cout][cin][ntaps] (taps in the
    order of desc["taps"]: kh * kw + kw for the forward tap tables), exact on the operands as given.
    The three keyword arguments are deliberate MUTATIONS for the tests of this reference (each must change the result): tap_shift
    (tap index, extra dx), drop_last_column (the last tile column contributes nothing), swap_groups (the two sources change places)."""
    B, TH, TW, IH, IW, s = desc["B"], desc["TH"], desc["TW"], desc["IH"], desc["IW"], desc["stride"]
    gC, cout = desc["gC"], desc["cout"]
    srcs = list(srcs)
    d = dict(desc)
    if swap_groups:
        assert len(srcs) == 2
        srcs, d["srcs"] = srcs[::-1], desc["srcs"][::-1]
    if desc.get("up2"):
        # nearest x2 of the one source, then the ordinary dense 3x3 gradient on the 2 TH x 2 TW grid
        assert len(srcs) == 1 and s == 1 and (IH, IW) == (TH, TW) and tuple(srcs[0].shape[1:3]) == (TH, TW)
        TH, TW, IH, IW = 2 * TH, 2 * TW, 2 * IH, 2 * IW
        d.update(IH=IH, IW=IW)
    xin = packed_input(d, srcs)
    g = gout.to(F64)
    assert tuple(g.shape) == (B, TH, TW, gC), (tuple(g.shape), (B, TH, TW, gC))
    if drop_last_column:
        g = g.clone()
        g[:, :, TW - 1] = 0
    dev = g.device
    M, K = B * TH * TW, xin.shape[3]
    gm = g.reshape(M, gC)
    ty, tx = torch.arange(TH, device=dev) * s, torch.arange(TW, device=dev) * s
    slab = torch.zeros(len(desc["taps"]), gC, K, dtype=F64, device=dev)
    for t, (dy, dx) in enumerate(desc["taps"]):
        if tap_shift is not None and tap_shift[0] == t:
            dx = dx + tap_shift[1]
        iy, ix = ty + dy, tx + dx
        my, mx = (iy >= 0) & (iy < IH), (ix >= 0) & (ix < IW)
        v = xin[:, iy.clamp(0, IH - 1)][:, :, ix.clamp(0, IW - 1)]
        v = v * (my.view(1, TH, 1, 1) & mx.view(1, 1, TW, 1)).to(F64)
        slab[t] = gm.t() @ v.reshape(M, K)
    cols = torch.tensor(unpack_columns(desc), device=dev)
    oihw = slab[:, :cout][:, :, cols].permute(1, 2, 0).contiguous()
    return slab, oihw


def bias_ref(gout, cout):
    """db[co] = sum over positions of gout[., co] for co < cout (float64)."""
    return gout.to(F64).reshape(-1, gout.shape[-1])[:, :cout].sum(0)


def slab_sum(ws, nsplit, ntaps, w_rows, cin_total, first=0):
    """Float64 sum of the raw slabs [first, nsplit) of a workspace laid out [nsplit][ntaps][w_rows][cin_total]."""
    n = ntaps * w_rows * cin_total
    return ws[:nsplit * n].view(nsplit, ntaps, w_rows, cin_total)[first:].to(F64).sum(0)


def conv_autograd(desc, srcs_nchw, gout_nchw):
    """The same gradient by float64 autograd of F.conv2d (through F.interpolate(mode='nearest') and torch.cat where the mode has them):
    (dW OIHW [cout][cin][kh][kw], db [cout]).  srcs_nchw: the REAL channels of every source, NCHW float64 ([B][C] for a constant);
    gout_nchw [B][cout][TH'][TW'].  Independent of wgrad_ref: it is what the CPU tests hold the reference to."""
    import torch.nn.functional as Fn
    IH, IW, s = desc["IH"], desc["IW"], desc["stride"]
    dys, dxs = sorted({t[0] for t in desc["taps"]}), sorted({t[1] for t in desc["taps"]})
    kh, kw = len(dys), len(dxs)
    assert [(dy, dx) for dy in dys for dx in dxs] == [tuple(t) for t in desc["taps"]], "forward tap table expected"
    xs = []
    for t, sd in zip(srcs_nchw, desc["srcs"]):
        t = t.to(F64)
        if sd["form"] == "bcast":
            t = t.view(*t.shape, 1, 1).expand(*t.shape, IH, IW)
        elif tuple(t.shape[2:]) != (IH, IW) and not desc.get("up2"):
            t = Fn.interpolate(t, size=(IH, IW), mode="nearest")
        xs.append(t)
    x = torch.cat(xs, 1) if len(xs) > 1 else xs[0]
    if desc.get("up2"):
        x = Fn.interpolate(x, scale_factor=2, mode="nearest")
    w = torch.zeros(desc["cout"], x.shape[1], kh, kw, dtype=F64, requires_grad=True)
    b = torch.zeros(desc["cout"], dtype=F64, requires_grad=True)
    y = Fn.conv2d(x, w, b, stride=s, padding=(kh // 2, kw // 2))
    assert y.shape == gout_nchw.shape, (y.shape, gout_nchw.shape)
    (y * gout_nchw.to(F64)).sum().backward()
    return w.grad, b.grad
