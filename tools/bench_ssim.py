#!/usr/bin/env python3
"""Times of the SSIM kernels (csrc/ssim.hip) by HIP events: the metric on one KITTI frame (3 x 375 x 1242) and the loss forward + backward in one
launch at the training size (8 x 3 x 256 x 512), each beside the L1 loss kernel on the same tensors and beside its byte floor (the bytes the call
must move over HBM at the 6.3 TB/s a float4 copy reaches on this chip).  Tuning tool; profiles/ssim_timing.txt is its output."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from fal_net_amd import _lib as L
from fal_net_amd import metrics as M
lib, DEV = L.lib(), "cuda"
HBM = 6.3e12  # bytes / s, measured copy rate
MEAN = M.MEAN
def timeit(fn, n=200):
    for _ in range(10): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
def line(name, t, nbytes):
    floor = nbytes / HBM * 1e6
    print(f"{name:44s} {t:7.1f} us   {nbytes / 1e6:6.1f} MB   floor {floor:5.1f} us   {nbytes / t / 1e6:5.2f} TB/s")
S, seed = torch.zeros(2, device=DEV), torch.ones(1, device=DEV)
# ---- the metric: one frame -------------------------------------------------------------------------------------------------------------
B, H, W = 1, 375, 1242
p, r = torch.rand(B, 3, H, W, device=DEV) - 0.43, torch.rand(B, 3, H, W, device=DEV) - 0.43
table = M.MetricTable(1)
row = table.row(0)
ws = table.ssim_workspace(lib.falnet_ssim_workspace_bytes(B, 3, H, W, 5))
n = p.numel()
t = timeit(lambda: L.check(lib.falnet_ssim_metric(L.ptr(p), L.ptr(r), *MEAN, B, H, W, L.ptr(row.tensor), L.ptr(ws), L.stream_ptr())))
print(f"metric, {B} x 3 x {H} x {W} (kernel + finaliser; f64 window sums, 11 x 11):")
line("falnet_ssim_metric", t, 2 * n * 4)
t = timeit(lambda: L.check(lib.falnet_view_errors(L.ptr(p), L.ptr(r), *MEAN, B, H, W, L.ptr(row.tensor), L.ptr(table.workspace), L.stream_ptr())))
line("falnet_view_errors (per-pixel, same frame)", t, 2 * n * 4)
# ---- the loss: forward + backward at the training size ---------------------------------------------------------------------------------
B, C, H, W = 8, 3, 256, 512
a, b, g = (torch.rand(B, C, H, W, device=DEV) - 0.43 for _ in range(3))
n = a.numel()
wl = torch.zeros(int(lib.falnet_ssim_workspace_bytes(B, C, H, W, 1)) // 8, dtype=torch.float64, device=DEV)
nw = B * C * (H - 2) * (W - 2)
print(f"loss, {B} x {C} x {H} x {W} (3 x 3 box, f32):")
t_l1 = timeit(lambda: L.check(lib.falnet_l1_fwd_bwd(L.ptr(a), L.ptr(b), B, C, H * W, 1.0 / n, L.ptr(S), L.ptr(seed), L.ptr(g), L.stream_ptr())))
line("falnet_l1_fwd_bwd (writes the gradient)", t_l1, 3 * n * 4)
t_add = timeit(lambda: L.check(lib.falnet_ssim_loss_fwd_bwd(L.ptr(a), L.ptr(b), *MEAN, B, C, H, W, 1, 0.15 / nw, L.ptr(S), 1.0 / nw, L.ptr(seed), L.ptr(g), 1,
                                                            L.ptr(wl), L.stream_ptr())))
line("falnet_ssim_loss_fwd_bwd (adds to the gradient)", t_add, 4 * n * 4)
t = timeit(lambda: L.check(lib.falnet_ssim_loss_fwd_bwd(L.ptr(a), L.ptr(b), *MEAN, B, C, H, W, 1, 0.15 / nw, L.ptr(S), 1.0 / nw, L.ptr(seed), L.ptr(g), 0,
                                                        L.ptr(wl), L.stream_ptr())))
line("falnet_ssim_loss_fwd_bwd (assigns the gradient)", t, 3 * n * 4)
t = timeit(lambda: L.check(lib.falnet_ssim_loss_fwd(L.ptr(a), L.ptr(b), *MEAN, B, C, H, W, 1, 1.0 / nw, L.ptr(S), 1, L.ptr(wl), L.stream_ptr())))
line("falnet_ssim_loss_fwd", t, 2 * n * 4)
t = timeit(lambda: L.check(lib.falnet_ssim_loss_bwd(L.ptr(a), L.ptr(b), *MEAN, B, C, H, W, 1, 1.0 / nw, L.ptr(seed), L.ptr(g), 0, L.stream_ptr())))
line("falnet_ssim_loss_bwd", t, 3 * n * 4)
print(f"the step's SSIM term (fwd_bwd, add) is {t_add / t_l1:.2f} x the L1 kernel and {t_add / 5200 * 100:.2f} % of a 5.2 ms step")
