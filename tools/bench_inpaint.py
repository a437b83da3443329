#!/usr/bin/env python3
"""Time of the background-biased pull-push hole filling (csrc/inpaint.hip, falnet_inpaint_fwd) at C = 4, I = 8, beta = 4: 375 x 1242 and 256 x 512,
on the outputs of a falnet_med_pose_fwd call of 8 poses on an orbit (B = 1, N = 49), which is timed too, for scale.  Against it: a chain of
torch operations that implements the same definition on the same device (torch_fill below; its index tables are built outside the timed
region), and the byte floor (2 C + 2) H W 4 I -- values, weight and guide read once, out written once -- as a rate.  HIP events around INNER
back-to-back calls, the candidates in alternating order within every round, median (min .. max) over ROUNDS.  The working set at 375 x 1242 (inputs
and out 149 MB, workspace 30 MB) is about the size of the 256 MB Infinity Cache and is re-used from call to call: warm-cache figures, stated as such.
usage: python tools/bench_inpaint.py [out.txt]   (on an MI355X; profiles/inpaint_timing.txt)"""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import freeview as FV  # noqa: E402
from fal_net_amd import inpaint as IP  # noqa: E402

ROUNDS, INNER, WARM = 15, 5, 3
BETA, FLOOR = 4.0, 2.0 ** -10


def tent_tables(nf, nc, dev):
    i = torch.arange(nf, device=dev)
    odd = (i % 2) == 1
    t0 = torch.where(odd, (i - 1) // 2, i // 2 - 1)
    w0 = torch.where(odd, 0.75, 0.25).to(torch.float32)
    return t0.clamp(0, nc - 1), (t0 + 1).clamp(0, nc - 1), w0, 1.0 - w0


def div(n, d):
    return torch.where(d > 0, n / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(n))


class TorchFill:
    """The definition of include/falnet_hip.h (falnet_inpaint_fwd) as a chain of torch operations: what the kernels are measured against."""

    def __init__(self, H, W, dev):
        self.sizes = [(H, W)]
        while self.sizes[-1] != (1, 1):
            h, w = self.sizes[-1]
            self.sizes.append(((h + 1) // 2, (w + 1) // 2))
        self.tents = [(tent_tables(hf, hc, dev), tent_tables(wf, wc, dev)) for (hf, wf), (hc, wc) in zip(self.sizes, self.sizes[1:])]

    def up(self, x, l):
        (y0, y1, wy0, wy1), (x0, x1, wx0, wx1) = self.tents[l]
        r0, r1 = x[..., y0, :], x[..., y1, :]
        r0 = wx0 * r0[..., x0] + wx1 * r0[..., x1]
        r1 = wx0 * r1[..., x0] + wx1 * r1[..., x1]
        return wy0[:, None] * r0 + wy1[:, None] * r1

    def __call__(self, values, weight, guide, scale, beta, floor):
        C = values.shape[1]
        keep = weight >= floor
        w0 = torch.where(keep, weight, torch.zeros_like(weight))
        c0 = torch.where(keep, values, torch.zeros_like(values))
        g = torch.where(keep, torch.exp(-beta * (guide / scale.view(-1, 1, 1, 1))), torch.ones_like(weight))
        pyr = [torch.cat([c0 * g, w0 * g, w0], 1)]
        for h, w in self.sizes[:-1]:
            p = TF.pad(pyr[-1], (0, w % 2, 0, h % 2))
            s = (p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2])
            a = s[:, -1:]
            pyr.append(s * torch.where(a > 1, 1.0 / a, torch.ones_like(a)))
        top = pyr[-1]
        F, G = div(top[:, :C], top[:, C:C + 1]), div(top[:, C:C + 1], top[:, C + 1:])
        for l in range(len(pyr) - 2, -1, -1):
            UG = self.up(G, l)
            U = div(self.up(F * G, l), UG)
            if l == 0:
                return c0 + (1.0 - w0) * U
            t = pyr[l]
            a = t[:, C + 1:]
            F = a * div(t[:, :C], t[:, C:C + 1]) + (1.0 - a) * U
            G = a * div(t[:, C:C + 1], a) + (1.0 - a) * UG
        return c0 + (1.0 - w0) * F


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "inpaint_timing.txt"), "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
    lib = L.lib()
    emit(f"{torch.cuda.get_device_name(0)}; microseconds per call, HIP events around {INNER} back-to-back calls, median (min .. max) over {ROUNDS} rounds "
         f"after {WARM} warm-up rounds, candidates alternating within a round; warm caches (the working set is re-used from call to call)")
    for N, H, W in ((49, 375, 1242), (49, 256, 512)):
        B, V, C = 1, 8, 4
        I = B * V
        g = torch.Generator().manual_seed(3)
        d0 = (torch.randn(B, N, H, W, generator=g) * 2).cuda()
        left = torch.rand(B, 3, H, W, generator=g).cuda()
        mx = torch.full((B,), 300.0).cuda()
        mn = mx * 2 / 300
        K = FV.camera(H, W)
        rec = np.ascontiguousarray(np.stack([FV.pose(K, **kw) for kw in FV.paths.orbit(V, 0.5, 0.25, yaw=3.0)]).astype(np.float64))
        rp = rec.ctypes.data_as(ctypes.c_void_p)
        views, disps, cover = torch.empty(B, V, 3, H, W, device="cuda"), torch.empty(B, V, 1, H, W, device="cuda"), torch.empty(B, V, 1, H, W, device="cuda")
        st = L.stream_ptr()

        def pose():
            L.check(lib.falnet_med_pose_fwd(L.ptr(d0), L.ptr(left), L.ptr(mn), L.ptr(mx), rp, V, L.ptr(views), L.ptr(disps), L.ptr(cover), B, N, H, W, st))
        pose()
        values = torch.cat([views, disps * cover], 2).view(I, C, H, W).contiguous()
        weight, guide = cover.view(I, 1, H, W), disps.view(I, 1, H, W)
        scale = mx.view(B, 1).expand(B, V).contiguous().view(I)
        filled = torch.empty_like(values)
        ws = torch.empty(IP.workspace_bytes(C, H, W, I) // 4, device="cuda")

        def kernels():
            L.check(lib.falnet_inpaint_fwd(L.ptr(values), L.ptr(weight), L.ptr(guide), L.ptr(scale), BETA, FLOOR, L.ptr(filled), L.ptr(ws), ws.numel() * 4, I, C, H, W, st))
        chain = TorchFill(H, W, values.device)
        kernels()
        ref = chain(values, weight, guide, scale, BETA, FLOOR)
        torch.cuda.synchronize()
        holes = float((weight < FLOOR).float().mean())
        emit(f"C = {C}, I = {I} (1 sample x 8 orbit poses, N = {N}), {H} x {W}, L = {IP.levels(H, W)}, beta = {BETA:g}; {100 * holes:.1f} % of the pixels are empty; "
             f"kernels vs torch chain: max |difference| {float((filled - ref).abs().max()):.3g} on colours up to {float(ref.abs().max()):.3g}")
        cands = [("falnet_inpaint_fwd", kernels), ("torch chain of the same definition", lambda: chain(values, weight, guide, scale, BETA, FLOOR)),
                 ("falnet_med_pose_fwd, the render it follows (8 poses)", pose)]
        times = {name: [] for name, _ in cands}
        for r in range(WARM + ROUNDS):
            for name, fn in (cands if r % 2 == 0 else cands[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(INNER):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r >= WARM:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / INNER)
        med = {}
        for name, _ in cands:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            emit(f"  {name:54s} {med[name]:9.1f} ({t[0]:8.1f} .. {t[-1]:8.1f}) us")
        floor_bytes = (2 * C + 2) * H * W * 4 * I
        k = med["falnet_inpaint_fwd"]
        emit(f"  byte floor (2 C + 2) H W 4 I = {floor_bytes / 1e6:.1f} MB -> {floor_bytes / k / 1e6:.2f} TB/s achieved on it; torch chain / kernels "
             f"{med[cands[1][0]] / k:.1f}; kernels / render {k / med[cands[2][0]]:.2f}")


if __name__ == "__main__":
    main()
