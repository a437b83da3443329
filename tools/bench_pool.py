#!/usr/bin/env python3
"""falnet_maxpool2_bwd_codes against falnet_maxpool2_bwd, back to back in one process, at the three pool shapes of the Stage-1 benchmark
(B = 8, 256 x 512 input: 64 ch @ 256 x 512, 128 ch @ 128 x 256, 256 ch @ 64 x 128; bf16).  Each launch is timed alone between two events, with
a 512 MiB fill in front of it so that neither kernel finds its operands in the last-level cache; medians of 21.  Bytes moved per pooled
element: (4 + 1 + 4) x 2 with the full-resolution map, (0.25 + 1 + 4) x 2 with the codes -- ratio 0.58.  Tuning tool."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from fal_net_amd import _lib as L
lib, DEV, B, dt = L.lib(), "cuda", 8, torch.bfloat16
code = L.dtype_code(dt)
flush = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)


def timed(fn, n=21):
    ts = []
    for _ in range(n + 2):
        flush.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts[2:])[n // 2]


def codes_of(y):
    """The codes the fused pool would write for the stored map y (B, H, W, C): first maximum in row-major order, none when it is not > 0."""
    Bq, H, W, C = y.shape
    win = y.float().view(Bq, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(Bq, H // 2, W // 2, C, 4)
    mx = win.max(-1).values
    first = (win == mx[..., None]).float().argmax(-1)
    nib = torch.where(mx > 0, 1 << first, torch.zeros_like(first)).view(Bq, H // 2, W // 2, C // 2, 2)
    return (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8).contiguous()


for h, w, c in ((256, 512, 64), (128, 256, 128), (64, 128, 256)):
    y = torch.relu(torch.randn(B, h, w, c, device=DEV)).to(dt)
    gy = torch.randn(B, h // 2, w // 2, c, device=DEV).to(dt)
    codes = codes_of(y)
    gx0, gx1 = torch.empty_like(y), torch.empty_like(y)
    st = L.stream_ptr()
    t_old = timed(lambda: L.check(lib.falnet_maxpool2_bwd(L.ptr(y), L.ptr(gy), L.ptr(gy), L.ptr(gx0), B, h, w, c, code, st)))
    t_new = timed(lambda: L.check(lib.falnet_maxpool2_bwd_codes(L.ptr(codes), L.ptr(gy), L.ptr(gx1), B, h, w, c, code, st)))
    assert torch.equal(gx0.view(torch.int16), gx1.view(torch.int16))
    pooled = gy.numel() * 2
    print(f"{B}x{h}x{w}x{c}: maxpool2_bwd {t_old:6.1f} us ({9 * pooled / t_old / 1e6:5.2f} TB/s)   maxpool2_bwd_codes {t_new:6.1f} us "
          f"({5.25 * pooled / t_new / 1e6:5.2f} TB/s)   ratio {t_new / t_old:.3f}")
