"""Case runners of tests/test_gpu_losses.py: each drives the loss kernels of csrc/losses.hip through the C-ABI on one set of inputs and
asserts (exact cases) or returns its figures (random cases).  They live here so that tests/_loss_det.py can re-run the same cases in a
child process with deterministic reductions on.

The launch arithmetic (grid sizes, strides, tile counts) is restated here from the constants PARSED out of losses.hip, so the coverage
claims of the test module are computed, not remembered: a change of RED_BLOCKS, RED_THREADS, SM_TX or SM_TY moves these numbers and the
coverage test fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import torch

from fal_net_amd import _lib as L

import _loss_ref as R

DEV = "cuda"
NAN = float("nan")
_SRC = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc", "losses.hip")


def _source_constants():
    txt = open(_SRC).read()
    out = {}
    for name in ("RED_THREADS", "RED_BLOCKS", "SM_TY", "SM_TX"):
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, txt, re.M)
        assert m, f"{name} is no longer a plain #define in losses.hip"
        out[name] = int(m.group(1))
    for name, pat in (("GUARD_BLOCKS", r"grad_guard_kernel, dim3\((\d+)\), dim3\(RED_THREADS\)"),
                      ("ROWMAX_THREADS", r"rowmax_kernel, dim3\(B\), dim3\((\d+)\)"),
                      ("MSE3_FLOOR", r"if \(nb < (\d+)\) nb = \1;"),
                      ("SEEDS_THREADS", r"loss_seeds_kernel, dim3\(1\), dim3\((\d+)\)")):
        m = re.search(pat, txt)
        assert m, f"the launch of {name} in losses.hip no longer reads as this module restates it"
        out[name] = int(m.group(1))
    assert "i + 3 * stride < n8; i += 4 * stride" in txt and "i + 3 * 1024 < n4; i += 4 * 1024" in txt, "the 4x unrolled loops changed shape"
    return out


K = _source_constants()
RED_THREADS, RED_BLOCKS, SM_TY, SM_TX = K["RED_THREADS"], K["RED_BLOCKS"], K["SM_TY"], K["SM_TX"]
CAP = RED_THREADS * RED_BLOCKS  # work items of one sweep of a capped grid


# ------------------------------------------------------------------------------------------ launch arithmetic
def red_grid(n):
    return max(1, min(RED_BLOCKS, -(-n // RED_THREADS)))


def l1_launch(total, aligned=True, masked=False):
    """l1_fwd_kernel: the float4 path needs no mask, total % 4 == 0 and 16-B aligned pointers; the grid is sized by `total` either way."""
    vec = (not masked) and total % 4 == 0 and aligned
    items, stride = (total // 4 if vec else total), red_grid(total) * RED_THREADS
    return {"vec": vec, "unit": 4 if vec else 1, "items": items, "stride": stride, "trips": -(-items // stride)}


def unrolled_loops(n8, stride):
    """The 4x unrolled loop + remainder loop of mse_fwd_kernel<T, true> / mse3_fwd_bwd_kernel over all `stride` threads:
    (most unrolled trips of a thread, most remainder trips, number of threads that take BOTH loops)."""
    t = np.arange(stride, dtype=np.int64)
    u = np.maximum(0, -(-(n8 - 3 * stride - t) // (4 * stride)))
    r = np.maximum(0, -(-(n8 - (t + 4 * stride * u)) // stride))
    return int(u.max()), int(r.max()), int(((u > 0) & (r > 0)).sum())


def mse_launch(total, aligned=True):
    vec = total % 8 == 0 and aligned
    items = total // 8 if vec else total
    stride = red_grid(items) * RED_THREADS
    out = {"vec": vec, "unit": 8 if vec else 1, "items": items, "stride": stride, "trips": -(-items // stride)}
    if vec:
        out["unrolled"], out["remainder"], out["both"] = unrolled_loops(items, stride)
    return out


def mse3_begin(numel):
    """falnet_mse3_fwd_bwd: RED_BLOCKS workgroups shared out by size, at least MSE3_FLOOR each."""
    total, used, begin, floor = sum(numel), 0, [], K["MSE3_FLOOR"]
    for k in range(3):
        begin.append(used)
        nb = RED_BLOCKS - used if k == 2 else int(float(numel[k]) / float(total) * RED_BLOCKS)
        nb = max(nb, floor)
        if used + nb > RED_BLOCKS - floor * (2 - k):
            nb = RED_BLOCKS - floor * (2 - k) - used
        used += nb
    return begin + [used]


def smooth_tiles(B, H, W, x0, x1):
    ty = -(-H // SM_TY)
    fwd, bwd = B * ty * (-(-(x1 - x0) // SM_TX)), B * ty * (-(-W // SM_TX))
    txs = range(0, W, SM_TX)
    return {"fwd_tiles": fwd, "fwd_grid": min(fwd, RED_BLOCKS), "bwd_tiles": bwd, "bwd_grid": min(bwd, 4 * RED_BLOCKS),
            "fused_grid": min(bwd, RED_BLOCKS), "tiles_y": ty, "fwd_tiles_x": -(-(x1 - x0) // SM_TX), "bwd_tiles_x": len(txs),
            "empty_tiles_x": sum(1 for t in txs if not (t < x1 and t + SM_TX > x0)),
            "edge_inside_tile": x0 % SM_TX != 0 or (x1 % SM_TX != 0 and x1 != W)}


def rowmax_launch(n, aligned=True):
    th = K["ROWMAX_THREADS"]
    vec = n % 4 == 0 and aligned
    if not vec:
        return {"vec": False, "trips": -(-n // th)}
    n4 = n // 4
    t = np.arange(th, dtype=np.int64)
    u = np.maximum(0, -(-(n4 - 3 * th - t) // (4 * th)))
    r = np.maximum(0, -(-(n4 - (t + 4 * th * u)) // th))
    return {"vec": True, "n4": n4, "unrolled": int(u.max()), "remainder": int(r.max())}


# ------------------------------------------------------------------------------------------ plumbing
def dev(t, dtype=torch.float32, off=0):
    """Flat device copy of `t` in `dtype`; off > 0: at an offset of `off` elements into a larger buffer (a base pointer that is NOT
    16-B aligned; torch's allocator hands out 512-B aligned blocks).  The view keeps the buffer alive."""
    buf = torch.empty(t.numel() + off, dtype=dtype, device=DEV)
    v = buf[off:]
    v.copy_(t.reshape(-1).to(dtype))
    assert v.data_ptr() % 16 == (0 if off == 0 else (off * v.element_size()) % 16)
    return v


def filled(n, value, dtype=torch.float32, off=0):
    return torch.full((n + off,), value, dtype=dtype, device=DEV)[off:]


def scalar(v):
    return torch.tensor([float(v)], device=DEV)


def call(name, *args):
    L.check(getattr(L.lib(), name)(*args, L.stream_ptr()), name)


def same(got, want, what):
    """Element for element; a NaN left over from the pre-fill fails (NaN != NaN)."""
    want = want.reshape(-1).to(device=got.device, dtype=got.dtype)
    if not torch.equal(got.reshape(-1), want):
        bad = (got.reshape(-1) != want).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {want.numel()} elements differ, first at {i}: got {float(got.reshape(-1)[i])!r}, "
                             f"want {float(want[i])!r}")


def eq(got, want, what):
    got = float(got)
    assert got == want, f"{what}: got {got!r}, want {want!r} (difference {got - want!r})"


def _around(stride, items, unit):
    """First and last element of the work items on both sides of every k * stride (the seams of the grid-stride and unrolled loops)."""
    pos = []
    for k in range(1, items // stride + 1):
        for item in (k * stride - 1, k * stride):
            if item < items:
                pos += [item * unit, item * unit + unit - 1]
    return pos


# ------------------------------------------------------------------------------------------ exact cases
SCALE, GSV = 2.0 ** -12, 8.0  # powers of two: integer count x scale is exact


def l1_exact(shape, off_a=0, off_all=0, seed=1):
    """falnet_l1_fwd / _bwd (masked and not, accumulate 0 and 1), _l1_fwd_bwd, _l1_fwd_bwd_add on a - b in {0, +-1, +-2}."""
    B, Cc, H, W = shape
    HW, total = H * W, B * Cc * H * W
    launch = l1_launch(total, aligned=(off_a == 0 and off_all == 0))
    a8, b8, d8 = R.exact_diff(total, seed)
    R.plant(a8, b8, d8, [0, total - 1, total - 8] + _around(launch["stride"], launch["items"], launch["unit"]))
    g = torch.Generator().manual_seed(seed + 100)
    m8 = torch.randint(0, 3, (B, 1, H, W), generator=g, dtype=torch.int8)  # {0, 1, 2}: products stay integers
    s1, _ = R.exact_counts(d8)
    dm = (d8.reshape(B, Cc, H, W).to(torch.int64) * m8.to(torch.int64))
    sm = int(dm.abs().sum())
    assert 2 * sm < (1 << 24) and 3 * 4096 + 2 * s1 < (1 << 24)
    ref_v, ref_g = R.l1(a8[:4096].reshape(1, 1, 1, -1), b8[:4096].reshape(1, 1, 1, -1), None, SCALE)  # the closed form is the reference's
    assert float(ref_v) == int(d8[:4096].to(torch.int64).abs().sum()) * SCALE and torch.equal(ref_g.reshape(-1), SCALE * torch.sign(d8[:4096].double()))
    a, b = dev(a8, off=max(off_a, off_all)), dev(b8, off=off_all)
    m = dev(m8)
    sgn, sgn_m = torch.sign(d8.float()), torch.sign(dm.float()).reshape(-1) * m8.expand(B, Cc, H, W).reshape(-1).float()
    gsd = scalar(GSV)
    out = scalar(NAN)
    for mask, cnt in ((None, s1), (m, sm)):
        out.fill_(NAN)  # accumulate = 0 overwrites whatever is there
        call("falnet_l1_fwd", L.ptr(a), L.ptr(b), L.ptr(mask), B, Cc, HW, SCALE, L.ptr(out), 0)
        eq(out, cnt * SCALE, f"l1_fwd masked={mask is not None}")
        call("falnet_l1_fwd", L.ptr(a), L.ptr(b), L.ptr(mask), B, Cc, HW, SCALE, L.ptr(out), 1)
        eq(out, 2 * cnt * SCALE, f"l1_fwd accumulate masked={mask is not None}")
    for mask, sg in ((None, sgn), (m, sgn_m)):
        for gscale, gs in ((None, SCALE), (gsd, SCALE * GSV)):
            ga = filled(total, NAN, off=off_all)
            call("falnet_l1_bwd", L.ptr(a), L.ptr(b), L.ptr(mask), B, Cc, HW, SCALE, L.ptr(gscale), L.ptr(ga), 0)
            same(ga, sg * gs, f"l1_bwd masked={mask is not None} gscale={gscale is not None}")
            ga = filled(total, 3.0, off=off_all)
            call("falnet_l1_bwd", L.ptr(a), L.ptr(b), L.ptr(mask), B, Cc, HW, SCALE, L.ptr(gscale), L.ptr(ga), 1)
            same(ga, 3.0 + sg * gs, f"l1_bwd accumulate masked={mask is not None} gscale={gscale is not None}")
    out.fill_(3.0)  # the fused forms add onto the scalar
    ga = filled(total, NAN, off=off_all)
    call("falnet_l1_fwd_bwd", L.ptr(a), L.ptr(b), B, Cc, HW, SCALE, L.ptr(out), L.ptr(gsd), L.ptr(ga))
    eq(out, 3.0 + s1 * SCALE, "l1_fwd_bwd value")
    same(ga, sgn * (SCALE * GSV), "l1_fwd_bwd gradient")
    add8 = torch.randint(-3, 4, (total,), generator=g, dtype=torch.int8)
    gadd, ga = dev(add8, off=off_all), filled(total, NAN, off=off_all)
    call("falnet_l1_fwd_bwd_add", L.ptr(a), L.ptr(b), B, Cc, HW, SCALE, L.ptr(out), L.ptr(gsd), L.ptr(gadd), L.ptr(ga))
    eq(out, 3.0 + 2 * s1 * SCALE, "l1_fwd_bwd_add value")
    same(ga, sgn * (SCALE * GSV) + add8.float(), "l1_fwd_bwd_add gradient")
    torch.cuda.synchronize()
    return launch


SG, MSE_GSV = 2.0 ** -6, 0.125


def mse_exact(dtype, total, off=0, seed=2, max_sum=1 << 21):
    """falnet_mse_fwd (accumulate 0 and 1), _mse_bwd (with and without gscale), _mse_fwd_bwd on a - b in {0, +-1, +-2} stored in `dtype`."""
    launch = mse_launch(total, aligned=(off == 0))
    a8, b8, d8 = R.exact_diff(total, seed, max_sum)
    R.plant(a8, b8, d8, [0, total - 1, total // 8 * 8 - 8, total // 8 * 8 - 1] + _around(launch["stride"], launch["items"], launch["unit"]))
    _, s2 = R.exact_counts(d8)
    assert 3 * 4096 + 2 * s2 < (1 << 24)
    cpad = 8 if total % 8 == 0 else 1
    npix, code = total // cpad, L.dtype_code(dtype)
    a, b = dev(a8, dtype, off), dev(b8, dtype, off)
    df = d8.float()
    out = scalar(NAN)
    call("falnet_mse_fwd", L.ptr(a), L.ptr(b), npix, cpad, SCALE, L.ptr(out), 0, code)
    eq(out, s2 * SCALE, "mse_fwd")
    call("falnet_mse_fwd", L.ptr(a), L.ptr(b), npix, cpad, SCALE, L.ptr(out), 1, code)
    eq(out, 2 * s2 * SCALE, "mse_fwd accumulate")
    gsd = scalar(MSE_GSV)
    for gscale, gs in ((None, 2 * SG), (gsd, 2 * SG * MSE_GSV)):
        ga = filled(total, NAN, dtype, off)
        call("falnet_mse_bwd", L.ptr(a), L.ptr(b), npix, cpad, SG, L.ptr(gscale), L.ptr(ga), code)
        same(ga, df * gs, f"mse_bwd gscale={gscale is not None}")
    out.fill_(3.0)
    ga = filled(total, NAN, dtype, off)
    call("falnet_mse_fwd_bwd", L.ptr(a), L.ptr(b), npix, cpad, SCALE, L.ptr(out), SG, L.ptr(gsd), L.ptr(ga), code)
    eq(out, 3.0 + s2 * SCALE, "mse_fwd_bwd value")
    same(ga, df * (2 * SG * MSE_GSV), "mse_fwd_bwd gradient")
    torch.cuda.synchronize()
    return launch


P3, L3, F3 = C.c_void_p * 3, C.c_int64 * 3, C.c_float * 3
MSE3_SCALE_OUT, MSE3_SCALE_GRAD = (2.0 ** -12, 2.0 ** -11, 2.0 ** -10), (2.0 ** -6, 2.0 ** -5, 2.0 ** -7)


def mse3_exact(dtype, numels, seed=3):
    """falnet_mse3_fwd_bwd: three tensors, own scales, one launch."""
    begin = mse3_begin(numels)
    ds, av, bv, loops = [], [], [], []
    units = 0
    for k, n in enumerate(numels):
        stride = (begin[k + 1] - begin[k]) * RED_THREADS
        a8, b8, d8 = R.exact_diff(n, seed + k, 1 << 20)
        R.plant(a8, b8, d8, [0, n - 1, n - 8] + _around(stride, n // 8, 8))
        units += R.exact_counts(d8)[1] * (1 << k)
        ds.append(d8.float())
        av.append(dev(a8, dtype))
        bv.append(dev(b8, dtype))
        loops.append((n // 8, stride) + unrolled_loops(n // 8, stride))
    assert 3 * 4096 + units < (1 << 24)
    gas = [filled(n, NAN, dtype) for n in numels]
    out, gsd = scalar(3.0), scalar(MSE_GSV)
    call("falnet_mse3_fwd_bwd", P3(*[t.data_ptr() for t in av]), P3(*[t.data_ptr() for t in bv]), L3(*numels), F3(*MSE3_SCALE_OUT), L.ptr(out),
         F3(*MSE3_SCALE_GRAD), L.ptr(gsd), P3(*[t.data_ptr() for t in gas]), L.dtype_code(dtype))
    eq(out, 3.0 + units * MSE3_SCALE_OUT[0], "mse3_fwd_bwd value")
    for k in range(3):
        same(gas[k], ds[k] * (2 * MSE3_SCALE_GRAD[k] * MSE_GSV), f"mse3_fwd_bwd gradient of tensor {k}")
    torch.cuda.synchronize()
    return begin, loops


SM_SCALE, SM_GSV = 2.0 ** -20, 4.0


def smooth_exact(B, H, W, x0, x1, seed=4):
    """falnet_smooth_fwd / _bwd (accumulate 0 and 1) / _fwd_bwd with gamma = 0 on integer disparities with plateaus."""
    disp = R.plateau_disp(B, H, W, seed)
    img = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed + 1)) - 0.43
    count, adj = R.smooth_gamma0_int(disp, x0, x1)
    assert 2 * count + 3 * (1 << 20) < (1 << 24) and (adj == 0).any() and (adj != 0).any()
    adj = torch.from_numpy(adj).float()
    im, dp = dev(img), dev(disp)
    out = scalar(NAN)
    call("falnet_smooth_fwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, 0.0, SM_SCALE, L.ptr(out), 0)
    eq(out, count * SM_SCALE, "smooth_fwd")
    call("falnet_smooth_fwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, 0.0, SM_SCALE, L.ptr(out), 1)
    eq(out, 2 * count * SM_SCALE, "smooth_fwd accumulate")
    gd = filled(B * H * W, NAN)
    call("falnet_smooth_bwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, 0.0, SM_SCALE, L.ptr(None), L.ptr(gd), 0)
    same(gd, adj * SM_SCALE, "smooth_bwd (columns outside the window must be 0.0)")
    gsd = scalar(SM_GSV)
    gd = filled(B * H * W, 5.0)
    call("falnet_smooth_bwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, 0.0, SM_SCALE, L.ptr(gsd), L.ptr(gd), 1)
    same(gd, 5.0 + adj * (SM_SCALE * SM_GSV), "smooth_bwd accumulate")
    out.fill_(3.0)
    gd = filled(B * H * W, NAN)
    call("falnet_smooth_fwd_bwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, 0.0, SM_SCALE, L.ptr(out), L.ptr(gsd), L.ptr(gd))
    eq(out, 3.0 + count * SM_SCALE, "smooth_fwd_bwd value")
    same(gd, adj * (SM_SCALE * SM_GSV), "smooth_fwd_bwd gradient")
    torch.cuda.synchronize()
    return smooth_tiles(B, H, W, x0, x1)


# ------------------------------------------------------------------------------------------ random-data cases: figures against float64
def smooth_random(B, H, W, x0, x1, gamma, seed=11):
    img, disp = R.random_smooth_inputs(B, H, W, seed)
    v, g = R.smoothness(img, disp, x0, x1, gamma)
    sc = 1.0 / (B * H * (x1 - x0))
    im, dp = dev(img), dev(disp)
    out, out2, gsd = scalar(NAN), scalar(0.0), scalar(3.0)
    gd, gd2 = filled(B * H * W, NAN), filled(B * H * W, NAN)
    call("falnet_smooth_fwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, gamma, sc, L.ptr(out), 0)
    call("falnet_smooth_bwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, gamma, sc, L.ptr(None), L.ptr(gd), 0)
    call("falnet_smooth_fwd_bwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, gamma, sc, L.ptr(out2), L.ptr(gsd), L.ptr(gd2))
    return {"value": R.relscalar(out, v), "grad": R.relerr(gd, g.reshape(-1)), "fused_value": R.relscalar(out2, v),
            "fused_grad": R.relerr(gd2, 3.0 * g.reshape(-1))}


def l1_random(shape, masked, seed=12):
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    m = torch.rand(B, 1, H, W, generator=g) if masked else None
    v, gr = R.l1(a, b, m)
    sc = 1.0 / a.numel()
    ad, bd, md = dev(a), dev(b), (dev(m) if masked else None)
    out, gsd, ga = scalar(NAN), scalar(0.5), filled(a.numel(), NAN)
    call("falnet_l1_fwd", L.ptr(ad), L.ptr(bd), L.ptr(md), B, Cc, H * W, sc, L.ptr(out), 0)
    call("falnet_l1_bwd", L.ptr(ad), L.ptr(bd), L.ptr(md), B, Cc, H * W, sc, L.ptr(gsd), L.ptr(ga), 0)
    fig = {"value": R.relscalar(out, v), "grad": R.relerr(ga, 0.5 * gr.reshape(-1))}
    if not masked:
        out2, ga2 = scalar(0.0), filled(a.numel(), NAN)
        call("falnet_l1_fwd_bwd", L.ptr(ad), L.ptr(bd), B, Cc, H * W, sc, L.ptr(out2), L.ptr(gsd), L.ptr(ga2))
        fig.update(fused_value=R.relscalar(out2, v), fused_grad=R.relerr(ga2, 0.5 * gr.reshape(-1)))
    return fig


F32_CHAIN = 4 * 2.0 ** -24  # the f32 roundings in front of the 16-bit one (the difference, two products of the scales, one with d)


def mse_random(dtype, n, seed=13):
    """16-bit: `grad` is the worst element's |got - ref| over its allowance (half an ulp of the type at that element, R.half_ulp, + the
    f32 chain in front of it), so <= 1 passes; f32: max-abs over max-abs.  The gradient scale keeps 16-bit gradients in the type's normal range, as the loss
    scale does in training."""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    sc, sg, gsv = 1.0 / n, 2.0 ** -7, 0.5
    v, _ = R.mse(a, b, dtype, sc)
    _, gr = R.mse(a, b, dtype, sg * gsv)
    cpad = 8 if n % 8 == 0 else 1
    ad, bd, code = dev(a, dtype), dev(b, dtype), L.dtype_code(dtype)
    out, out2, gsd = scalar(NAN), scalar(0.0), scalar(gsv)
    ga, ga2 = filled(n, NAN, dtype), filled(n, NAN, dtype)
    call("falnet_mse_fwd", L.ptr(ad), L.ptr(bd), n // cpad, cpad, sc, L.ptr(out), 0, code)
    call("falnet_mse_bwd", L.ptr(ad), L.ptr(bd), n // cpad, cpad, sg, L.ptr(gsd), L.ptr(ga), code)
    call("falnet_mse_fwd_bwd", L.ptr(ad), L.ptr(bd), n // cpad, cpad, sc, L.ptr(out2), sg, L.ptr(gsd), L.ptr(ga2), code)

    def gerr(got):
        if dtype == torch.float32:
            return R.relerr(got, gr)
        allow = R.half_ulp(gr, dtype) + F32_CHAIN * gr.abs()
        return float(((got.double().cpu() - gr).abs() / allow).max())
    return {"value": R.relscalar(out, v), "grad": gerr(ga), "fused_value": R.relscalar(out2, v), "fused_grad": gerr(ga2)}


# ------------------------------------------------------------------------------------------ the case lists
L1_EXACT = [((2, 3, 12, 40), 0, 0), ((8, 3, 256, 512), 0, 0), ((8, 3, 256, 512), 1, 0), ((8, 3, 256, 512), 0, 1), ((1, 3, 75, 250), 0, 0),
            ((1, 3, 75, 250), 0, 1)]
MSE_BELOW_CAP = 8 * 100003                # one group per thread, the last workgroup partly idle
MSE_UNROLL_EDGE = 8 * (3 * CAP + 5)       # just above 3 x 131 072 groups: five threads take ONE unrolled trip, the others three remainder trips
MSE_BOTH_LOOPS = 8 * (6 * CAP + 37)       # an unrolled trip AND remainder trips in the same thread, ragged end
MSE_SCALAR = 320003                       # total % 8 != 0: the element-wise form, more than one sweep
MSE_UNALIGNED = (1 << 20) + 8             # a multiple of 8 at a base pointer off by one element: the element-wise form again
MSE_EXACT = [(MSE_BELOW_CAP, 0), (MSE_UNROLL_EDGE, 0), (MSE_BOTH_LOOPS, 0), (MSE_SCALAR, 0), (MSE_UNALIGNED, 1)]
BENCH_SLICES = (8 * 256 * 512 * 64, 8 * 128 * 256 * 128, 8 * 64 * 128 * 256)  # the three VGG maps of the benchmark's perceptual term
MSE3_TODAY = (2 * 64 * 32 * 64, 2 * 128 * 16 * 32, 1 * 64 * 2 * 4)            # the sizes of test_gpu_ops.py::test_losses
MSE3_SMALLEST_FIRST = (1 * 64 * 2 * 4, 2 * 64 * 32 * 64, 2 * 128 * 16 * 32)
SMOOTH_EXACT = [(B, H, W, x0, x1) for B, H, W, wins in R.SMOOTH_CASES for x0, x1 in wins]
ROWMAX_REM = 131072 + 6000


# ------------------------------------------------------------------------------------------ coverage arithmetic
def check_coverage():
    """The table in the docstring of tests/test_gpu_losses.py, computed."""
    cap = CAP
    big, odd = 8 * 3 * 256 * 512, 3 * 75 * 250
    v = l1_launch(big)
    assert v["vec"] and v["trips"] >= 2
    s = l1_launch(big, aligned=False)
    assert not s["vec"] and s["trips"] >= 2
    assert not l1_launch(odd)["vec"] and odd % 4 != 0
    assert l1_launch(2 * 3 * 12 * 40)["trips"] == 1  # (today's size: one trip, which is the gap)
    m = mse_launch(MSE_BELOW_CAP)
    assert m["vec"] and m["unrolled"] == 0 and m["remainder"] == 1 and m["items"] < cap and m["items"] % RED_THREADS != 0
    m = mse_launch(MSE_UNROLL_EDGE)
    assert m["vec"] and m["unrolled"] == 1 and m["remainder"] == 3 and m["both"] == 0 and m["items"] - 3 * m["stride"] == 5
    m = mse_launch(MSE_BOTH_LOOPS)
    assert m["vec"] and m["unrolled"] == 1 and m["remainder"] == 3 and m["both"] == m["stride"] and m["items"] % m["stride"] == 37
    m = mse_launch(BENCH_SLICES[0])
    assert m["vec"] and m["unrolled"] >= 2 and m["remainder"] == 0
    for n, aligned in ((MSE_SCALAR, True), (MSE_UNALIGNED, False)):
        m = mse_launch(n, aligned)
        assert not m["vec"] and m["trips"] >= 2
    b = mse3_begin(MSE3_TODAY)
    assert (b[1] - b[0]) * RED_THREADS > MSE3_TODAY[0] // 8  # idle workgroups, unrolled loop never runs
    b = mse3_begin(BENCH_SLICES)
    for k in range(3):
        stride = (b[k + 1] - b[k]) * RED_THREADS
        u, r, both = unrolled_loops(BENCH_SLICES[k] // 8, stride)
        assert u >= 2, (k, u)
    u, r, both = unrolled_loops(BENCH_SLICES[0] // 8, (b[1] - b[0]) * RED_THREADS)
    assert r >= 1 and both > 0 and (BENCH_SLICES[0] // 8) % (4 * (b[1] - b[0]) * RED_THREADS) != 0  # ragged tail
    b = mse3_begin(MSE3_SMALLEST_FIRST)
    assert int(MSE3_SMALLEST_FIRST[0] / sum(MSE3_SMALLEST_FIRST) * RED_BLOCKS) < K["MSE3_FLOOR"] and b[1] - b[0] == K["MSE3_FLOOR"]
    r = rowmax_launch(131072)
    assert r["vec"] and r["unrolled"] >= 2 and r["remainder"] == 0
    r = rowmax_launch(ROWMAX_REM)
    assert r["vec"] and r["unrolled"] >= 2 and r["remainder"] == 2
    assert not rowmax_launch(75 * 250)["vec"] and rowmax_launch(480)["unrolled"] == 0
    for x0, x1 in ((102, 512), (0, 409), (0, 512)):
        t = smooth_tiles(8, 256, 512, x0, x1)
        assert t["fwd_tiles"] > t["fwd_grid"] and t["bwd_tiles"] > t["fused_grid"] and t["tiles_y"] >= 2 and t["fwd_tiles_x"] >= 2
    assert smooth_tiles(8, 256, 512, 0, 512)["bwd_tiles"] == 1024
    assert smooth_tiles(3, 37, 131, 70, 90)["empty_tiles_x"] == 2 and smooth_tiles(3, 37, 131, 77, 78)["empty_tiles_x"] == 2
    for B, H, W, x0, x1 in ((3, 37, 131, 63, 129), (3, 37, 131, 70, 90), (8, 256, 512, 102, 512), (8, 256, 512, 0, 409)):
        assert smooth_tiles(B, H, W, x0, x1)["edge_inside_tile"]
    assert not smooth_tiles(3, 37, 131, 64, 128)["edge_inside_tile"] and 63 % SM_TX != 0 and 102 % SM_TX != 0
    assert smooth_tiles(1, 16, 64, 0, 64)["bwd_tiles"] == 1  # (test_smoothness_column_window's size: one tile, which is the gap)
    assert smooth_tiles(2, 17, 130, 0, 130)["tiles_y"] == 2 and smooth_tiles(2, 1, 200, 0, 200)["tiles_y"] == 1
