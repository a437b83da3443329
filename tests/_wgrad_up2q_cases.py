"""Cases, integer operands, float64 reference and the C-ABI launch for tests/test_gpu_wgrad_up2q.py: the `deconv` weight gradient (nearest x2, then
3x3 / pad 1) with all four parity classes per low-resolution row step (falnet_wgrad_t::up2 = 2, wgrad3x3_up2q_kernel).

Operands are small integers (input in [-3, 4], upstream gradient in [-4, 4]), exact in bf16 and f16; the largest case sums 20 x 140 positions, so
every partial sum stays below 2800 * 16 < 2^24 and the f32 result does not depend on the order of summation: `==` against the reference."""
import ctypes as C
import functools
import types

import torch

F32, F64 = torch.float32, torch.float64
X_RANGE, G_RANGE = (-3, 4), (-4, 4)
GUARD_FLOATS = 1024

# name, B, cin, cout, low-res H, W: the smallest shapes at which this form can go wrong
CASES = [
    dict(name="9x33", B=2, cin=64, cout=64, H=9, W=33),       # odd row count (a half step), one-column second strip, ranges straddling a sample
    dict(name="10x70_c96_49", B=1, cin=96, cout=49, H=10, W=70),  # half-empty second input tile, gout padded 49 -> 64 (stride gC)
    dict(name="8x24_c128", B=2, cin=128, cout=64, H=8, W=24),  # two input-channel tiles sharing a range
]
BY_NAME = {c["name"]: c for c in CASES}


def pad32(c):
    return (c + 31) // 32 * 32


def units(case):
    """(sample, 32-column strip, low-resolution row) units of the launch: what the splits cut."""
    return case["B"] * ((case["W"] + 31) // 32) * case["H"]


def split_counts(case):
    """1, 3, 5 and a count above the units (so above the row pairs too): some splits are then empty and must write slabs of zeros."""
    return [1, 3, 5, units(case) + 3]


def assert_exact(case):
    n = case["B"] * 4 * case["H"] * case["W"]
    assert n * max(map(abs, X_RANGE)) * max(map(abs, G_RANGE)) < 2 ** 24


@functools.lru_cache(maxsize=None)
def operands(name):
    """(x NHWC [B][H][W][cin_pad], g NHWC [B][2H][2W][gC]) as f32 CPU tensors of integers; padding channels of x zero, every channel of g filled."""
    c = BY_NAME[name]
    gen = torch.Generator().manual_seed(1000 * c["H"] + c["W"] + c["cin"])
    x = torch.randint(X_RANGE[0], X_RANGE[1] + 1, (c["B"], c["H"], c["W"], pad32(c["cin"])), generator=gen).to(F32)
    x[..., c["cin"]:] = 0
    g = torch.randint(G_RANGE[0], G_RANGE[1] + 1, (c["B"], 2 * c["H"], 2 * c["W"], pad32(c["cout"])), generator=gen).to(F32)
    return x, g


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 on the CPU: nearest x2, then the 3x3 / pad-1 weight gradient [cout][cin][3][3] and the bias gradient [cout]."""
    c = BY_NAME[name]
    x, g = operands(name)
    cin, cout, H2, W2 = c["cin"], c["cout"], 2 * c["H"], 2 * c["W"]
    up = x[..., :cin].to(F64).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    up = torch.nn.functional.pad(up, (0, 0, 1, 1, 1, 1))
    gd = g[..., :cout].to(F64)
    dw = torch.empty(cout, cin, 3, 3, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum("bhwo,bhwi->oi", gd, up[:, ky:ky + H2, kx:kx + W2])
    return dw, gd.sum(dim=(0, 1, 2))


def launch(case, dtype, nsplit, up2, bias, device="cuda"):
    """One falnet_wgrad launch (variant 7) of the case in the form `up2` (2, 1, or 0 = the high-resolution form over the same operands) with
    `nsplit` slabs, then falnet_wgrad_reduce.  Returns (gradient [cout][cin][3][3] f64, bias gradient [cout] f64 or None, guard intact)."""
    from fal_net_amd import _lib as L
    from fal_net_amd import ops
    lib = L.lib()
    x, g = operands(case["name"])
    x_t, g_t = x.to(dtype).to(device).contiguous(), g.to(dtype).to(device).contiguous()
    cin, cout, cin_pad, gC = case["cin"], case["cout"], pad32(case["cin"]), pad32(case["cout"])
    h, w = (case["H"], case["W"]) if up2 else (2 * case["H"], 2 * case["W"])
    d = L.Wgrad()
    pc = types.SimpleNamespace(cout=cout, cin_pad=cin_pad)
    ops._fill_wgrad(d, dtype, [ops.nhwc_src(x_t)], h, w, g_t, [(dy, dx, 0) for dy, dx, _ in ops.fwd_taps(3)], 1, case["B"], h, w, pc)
    d.variant, d.nsplit, d.up2 = 7, nsplit, up2
    nfl = nsplit * 9 * gC * cin_pad
    assert int(lib.falnet_wgrad_workspace_bytes(C.byref(d))) == 4 * nfl
    ws = torch.full((nfl + GUARD_FLOATS,), float("nan"), dtype=F32, device=device)
    d.partial = ws.data_ptr()
    db = None
    if bias:
        assert int(lib.falnet_wgrad_fuses_bias(C.byref(d))) == 1
        db = torch.zeros(gC + 32, dtype=F32, device=device)
        db[cout:] = 7.0
        d.bias_grad = db.data_ptr()
    what = f"{case['name']} up2={up2} nsplit={nsplit}"
    L.check(lib.falnet_wgrad(C.byref(d), L.stream_ptr()), what)
    gw = torch.full((cout, cin, 9), float("nan"), dtype=F32, device=device)
    L.check(lib.falnet_wgrad_reduce(L.ptr(ws), nsplit, 9, gC, cin_pad, L.ptr(gw), cout, cin, cin, cin_pad, 0, L.stream_ptr()), what + " reduce")
    guard = bool(torch.isnan(ws[nfl:]).all()) and (db is None or bool((db[cout:] == 7.0).all()))
    keep = (x_t, g_t)  # the operands outlive the launches
    torch.cuda.synchronize()
    del keep
    return gw.view(cout, cin, 3, 3).to(F64).cpu(), None if db is None else db[:cout].to(F64).cpu(), guard
