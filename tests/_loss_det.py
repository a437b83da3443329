"""Helper of tests/test_gpu_losses.py::test_deterministic_reductions_child (run as a subprocess with FALNET_DETERMINISTIC=1: the switch
is read when the library is loaded).  With the ORDERED tail of red_finish on:
  * the exact cases of tests/_loss_cases.py give the same integers (they assert themselves), accumulate = 1 forms included;
  * random-data scalars are bit-identical on two calls, on another stream, and on a further call (the ticket is back at zero), and
    within the bound of the float64 reference."""
import json
import os
import struct
import sys

os.environ["FALNET_DETERMINISTIC"] = "1"
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch  # noqa: E402

from fal_net_amd import _lib as L  # noqa: E402

import _loss_cases as K  # noqa: E402
import _loss_ref as R  # noqa: E402
from _loss_cases import NAN, call, dev, filled, scalar  # noqa: E402


def bits(t):
    return struct.pack("<f", float(t)).hex()


def exact_cases():
    n = 0
    for shape, off_a, off_all in K.L1_EXACT:
        K.l1_exact(shape, off_a, off_all)
        n += 1
    for total, off in K.MSE_EXACT:
        K.mse_exact(torch.float32, total, off)
        n += 1
    for dtype in (torch.bfloat16, torch.float16):
        K.mse_exact(dtype, K.MSE_BOTH_LOOPS, 0)
        n += 1
    K.mse3_exact(torch.float32, K.MSE3_SMALLEST_FIRST)
    K.mse3_exact(torch.float16, K.MSE3_TODAY)
    K.mse3_exact(torch.bfloat16, K.BENCH_SLICES, seed=6)  # all 512 workgroups publish, the last arriver adds them in order
    n += 3
    for B, H, W, x0, x1 in K.SMOOTH_EXACT:
        K.smooth_exact(B, H, W, x0, x1)
        n += 1
    return n


class RandomScalars:
    """Fixed device inputs; run() launches every reduction once and returns the bit patterns of the scalars."""

    def __init__(self):
        g = torch.Generator().manual_seed(21)
        self.shape = (8, 3, 256, 512)
        a, b = torch.randn(*self.shape, generator=g), torch.randn(*self.shape, generator=g)
        m = torch.rand(8, 1, 256, 512, generator=g)
        self.a, self.b, self.m = dev(a), dev(b), dev(m)
        self.n = K.MSE_BOTH_LOOPS
        x, y = torch.randn(self.n, generator=g), torch.randn(self.n, generator=g)
        self.xy = {dt: (dev(x, dt), dev(y, dt)) for dt in (torch.float32, torch.bfloat16, torch.float16)}
        self.x3 = [(dev(torch.randn(n, generator=g), torch.bfloat16), dev(torch.randn(n, generator=g), torch.bfloat16)) for n in K.MSE3_TODAY]
        self.sm = []
        for B, H, W, x0, x1 in ((8, 256, 512, 102, 512), (3, 37, 131, 63, 129)):
            img, disp = R.random_smooth_inputs(B, H, W, 11)
            self.sm.append((B, H, W, x0, x1, dev(img), dev(disp), R.smoothness(img, disp, x0, x1, 2.0)[0]))
        self.ref = {"l1": R.l1(a, b)[0], "l1_masked": R.l1(a, b, m)[0], "mse_f32": R.mse(x, y)[0], "mse_bf16": R.mse(x, y, torch.bfloat16)[0],
                    "mse_f16": R.mse(x, y, torch.float16)[0]}
        self.figures = {}

    def run(self):
        out, vals = scalar(NAN), []
        B, Cc, H, W = self.shape
        sc = 1.0 / self.a.numel()

        def take(name=None):
            torch.cuda.current_stream().synchronize()
            vals.append(bits(out))
            if name is not None:
                self.figures[name] = max(self.figures.get(name, 0.0), R.relscalar(out, self.ref[name]))
        call("falnet_l1_fwd", L.ptr(self.a), L.ptr(self.b), L.ptr(None), B, Cc, H * W, sc, L.ptr(out), 0)
        take("l1")
        call("falnet_l1_fwd", L.ptr(self.a), L.ptr(self.b), L.ptr(self.m), B, Cc, H * W, sc, L.ptr(out), 0)
        take("l1_masked")
        out.fill_(1.5)
        call("falnet_l1_fwd", L.ptr(self.a), L.ptr(self.b), L.ptr(None), B, Cc, H * W, sc, L.ptr(out), 1)  # accumulate onto a non-zero scalar
        take()
        assert abs(float(out) - 1.5 - float(self.ref["l1"])) < 1e-5
        ga = filled(self.a.numel(), NAN)
        out.fill_(0.25)
        call("falnet_l1_fwd_bwd", L.ptr(self.a), L.ptr(self.b), B, Cc, H * W, sc, L.ptr(out), L.ptr(None), L.ptr(ga))
        take()
        for dt, nm in ((torch.float32, "mse_f32"), (torch.bfloat16, "mse_bf16"), (torch.float16, "mse_f16")):
            x, y = self.xy[dt]
            call("falnet_mse_fwd", L.ptr(x), L.ptr(y), self.n // 8, 8, 1.0 / self.n, L.ptr(out), 0, L.dtype_code(dt))
            take(nm)
            call("falnet_mse_fwd", L.ptr(x), L.ptr(y), self.n // 8, 8, 1.0 / self.n, L.ptr(out), 1, L.dtype_code(dt))
            take()
            gx = filled(self.n, NAN, dt)
            out.fill_(0.0)
            call("falnet_mse_fwd_bwd", L.ptr(x), L.ptr(y), self.n // 8, 8, 1.0 / self.n, L.ptr(out), 2.0 ** -7, L.ptr(None), L.ptr(gx), L.dtype_code(dt))
            take(nm)
        g3 = [filled(n, NAN, torch.bfloat16) for n in K.MSE3_TODAY]
        out.fill_(0.0)
        call("falnet_mse3_fwd_bwd", K.P3(*[t[0].data_ptr() for t in self.x3]), K.P3(*[t[1].data_ptr() for t in self.x3]), K.L3(*K.MSE3_TODAY),
             K.F3(*[1.0 / n for n in K.MSE3_TODAY]), L.ptr(out), K.F3(*[2.0 ** -7] * 3), L.ptr(None), K.P3(*[t.data_ptr() for t in g3]),
             L.dtype_code(torch.bfloat16))
        take()
        for i, (B, H, W, x0, x1, im, dp, ref) in enumerate(self.sm):
            sc = 1.0 / (B * H * (x1 - x0))
            self.ref[f"smooth{i}"] = ref
            call("falnet_smooth_fwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, 2.0, sc, L.ptr(out), 0)
            take(f"smooth{i}")
            call("falnet_smooth_fwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, 2.0, sc, L.ptr(out), 1)
            take()
            gd = filled(B * H * W, NAN)
            out.fill_(0.0)
            call("falnet_smooth_fwd_bwd", L.ptr(im), L.ptr(dp), B, H, W, x0, x1, 2.0, sc, L.ptr(out), L.ptr(None), L.ptr(gd))
            take(f"smooth{i}")
        return vals


def main():
    assert L.lib().falnet_get_deterministic() == 1
    n_exact = exact_cases()
    rs = RandomScalars()
    runs = [rs.run(), rs.run()]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        runs.append(rs.run())
    side.synchronize()
    runs.append(rs.run())
    print(json.dumps({"deterministic": 1, "exact_cases": n_exact, "scalars": runs, "figures": rs.figures}), flush=True)


if __name__ == "__main__":
    main()
