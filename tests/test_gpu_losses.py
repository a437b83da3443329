"""The loss and loss-scale kernels of csrc/losses.hip through the C-ABI, at the sizes they run at, against exact integers and against the
float64 references of tests/_loss_ref.py (the case runners and the launch arithmetic are in tests/_loss_cases.py).

a. exact cases, compared with ==: a - b in {0, +-1, +-2}, power-of-two scales, integer disparities with gamma = 0.  Any dropped, doubled
   or misplaced element moves the answer by a whole unit; every gradient buffer starts as NaN.
b. random data against float64: bounds from profiles/loss_kernels_vs_f64.txt (BOUND below).
c. grad_guard, loss_scale_update, loss_seeds, step_scalars, the guarded Adam.
d. the same with deterministic (ordered) reductions, in a child process (tests/_loss_det.py).
e. the Python surface of fal_net_amd/loss_functions.py at 8 x 256 x 512.

Which case reaches which loop (test_every_named_loop_is_reached computes this table from the constants parsed out of losses.hip, so a
change of RED_BLOCKS / RED_THREADS / SM_TX / SM_TY cannot silently un-cover a loop; CAP = RED_BLOCKS x RED_THREADS = 131 072):

  kernel                 loop / branch                      case                               arithmetic
  l1_fwd_kernel          float4 path, 2nd grid-stride trip  L1 8x3x256x512 aligned             n4 = 786 432 > CAP: 6 trips
  l1_fwd_kernel          scalar path, 2nd trip              L1 8x3x256x512, base off by 1 f32  total = 3 145 728 > CAP: 24 trips
  l1_fwd_kernel          scalar path by total % 4 != 0      L1 1x3x75x250                      total = 56 250, % 4 = 2
  l1_fwd_kernel          gadd                               every L1 case (l1_fwd_bwd_add)
  mse_fwd_kernel<T,true> one group per thread, no loop 2    MSE_BELOW_CAP                      n8 = 100 003 < CAP
  mse_fwd_kernel<T,true> unrolled loop, edge                MSE_UNROLL_EDGE                    n8 = 3 CAP + 5: 5 threads x 1 unrolled trip
  mse_fwd_kernel<T,true> unrolled + remainder, same thread  MSE_BOTH_LOOPS                     n8 = 6 CAP + 37: 1 unrolled + 2..3 remainder trips
  mse_fwd_kernel<T,true> unrolled only (the benchmark)      BENCH_SLICES[0], bf16              n8 = 64 CAP: 16 unrolled trips, no remainder
  mse_fwd_kernel<T,false> element-wise, 2nd trip            MSE_SCALAR, MSE_UNALIGNED          total = 320 003 / 1 048 584 > CAP
  mse3_fwd_bwd_kernel    stride > n8: idle workgroups       MSE3_TODAY                         tensor 0: stride 87 040 > n8 32 768
  mse3_fwd_bwd_kernel    unrolled + ragged remainder        BENCH_SLICES, bf16                 tensor 0: 292 blocks, n8 = 8 388 608 = 28 x 4 stride + 16 384
  mse3_fwd_bwd_kernel    16-workgroup floor on tensor 0     MSE3_SMALLEST_FIRST                int(512 x 512 / 393 728) = 0 -> 16
  rowmax_kernel          4x loop, all four lanes            rowmax n = 131 072                 n4 = 32 768 = 8 x 4096: 8 unrolled trips, NO remainder
  rowmax_kernel          remainder after the 4x loop        rowmax n = 131 072 + 6 000         n4 = 34 268: 8 unrolled + 2 remainder trips
  rowmax_kernel          scalar path                        rowmax n = 18 750                  n % 4 = 2
  smooth_fwd_kernel      grid-stride over tiles             smooth 8x256x512, every window     896 / 896 / 1 024 tiles > 512 workgroups
  smooth_bwd_kernel      grid-stride over tiles (fused)     smooth 8x256x512                   1 024 tiles > 512 workgroups
  smooth_*_kernel        halo across seams, both directions every multi-tile shape             e.g. 8x256x512: 16 x 8 tiles per sample
  smooth_fwd vs _bwd     tiles from x0 vs from column 0     windows (102,512), (63,129), ...   x0 % 64 != 0
  smooth_*_kernel        window edge inside a tile          (0,409), (70,90), (63,129)         x1 % 64 != 0 / x0 % 64 != 0
  smooth_bwd_kernel      any == false tiles write zeros     3x37x131 (70,90), (77,78)          tiles 0 and 2 of 3 miss the window
  grad_guard_kernel      last partial sweep, lanes != 0     the flat gradient of FAL_netB N=49 n4 over 1 024 x 256 threads: see test_grad_guard

(The issue's n = 131 072 for rowmax has an EMPTY remainder loop, as the arithmetic above shows, so the planted-in-the-remainder case
uses n = 137 072 beside it.  The MSE ABI has no untouched padding: padded channels are ordinary elements with a = b = 0 whose gradient
must come back as 0; the L1 ABI has no padding at all.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402

import _loss_cases as K  # noqa: E402
import _loss_ref as R  # noqa: E402
from _loss_cases import DEV, NAN, call, dev, eq, filled, same, scalar  # noqa: E402

# profiles/loss_kernels_vs_f64.txt: every reference-side deviation is below the 1e-5 that test_losses already uses, so the bound of
# every random-data case is 4 x 1e-5 (tests/test_loss_ref.py checks the file against this constant)
BOUND = R.bound(R.FLOOR)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_ID = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def _report(name, fig, bounds=None):
    print(f"{name}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()), flush=True)
    for k, v in fig.items():
        b = (bounds or {}).get(k, BOUND)
        assert v <= b, f"{name}: {k} = {v:.3e} > {b:.3e}"


# ------------------------------------------------------------------------------------------ coverage arithmetic
def test_every_named_loop_is_reached():
    K.check_coverage()


# ------------------------------------------------------------------------------------------ a. exact cases
@pytest.mark.parametrize("shape,off_a,off_all", K.L1_EXACT, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_l1_exact(shape, off_a, off_all):
    launch = K.l1_exact(shape, off_a, off_all)
    assert launch["vec"] == (off_a == 0 and off_all == 0 and (shape[0] * shape[1] * shape[2] * shape[3]) % 4 == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("total,off", K.MSE_EXACT)
def test_mse_exact(total, off, dtype):
    K.mse_exact(dtype, total, off)


def test_mse_exact_benchmark_slice1_bf16():
    """8 x 256 x 512 x 64 in bf16, once: the unrolled loop is the whole kernel."""
    launch = K.mse_exact(torch.bfloat16, K.BENCH_SLICES[0], 0, seed=5, max_sum=1 << 20)
    assert launch["unrolled"] == 16 and launch["remainder"] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("numels", [K.MSE3_TODAY, K.MSE3_SMALLEST_FIRST], ids=["today", "smallest_first"])
def test_mse3_exact(numels, dtype):
    K.mse3_exact(dtype, numels)


def test_mse3_exact_benchmark_slices_bf16():
    K.mse3_exact(torch.bfloat16, K.BENCH_SLICES, seed=6)


@pytest.mark.parametrize("B,H,W,x0,x1", K.SMOOTH_EXACT)
def test_smooth_exact_gamma0(B, H, W, x0, x1):
    K.smooth_exact(B, H, W, x0, x1)


@pytest.mark.parametrize("n", [131072, K.ROWMAX_REM, 75 * 250])
def test_rowmax(n):
    """The maximum planted, sample by sample, in each lane of the 4x unrolled loop, in its remainder (where there is one), in the last
    element; one sample with negative values only; B = 8."""
    B, th = 8, K.K["ROWMAX_THREADS"]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, n, generator=g).clamp_(-3.0, 3.0)
    launch = K.rowmax_launch(n)
    if launch["vec"]:
        spots = [4 * (5 + u * th) + u for u in range(4)]                   # float4 i, i + 1024, i + 2048, i + 3072 of thread 5, one component each
        spots += [4 * (5 + 4 * th + u * th) + 3 - u for u in range(4)]     # ... and of its second unrolled trip
        if launch["remainder"]:
            n4u = launch["unrolled"] * 4 * th
            spots[6:8] = [4 * (n4u + 7) + 2, 4 * (n4u + th + 3) + 1]        # first and second remainder trip
            assert spots[7] < n
    else:
        spots = [0, 1, th - 1, th, 3 * th + 17, n - th - 1, n - 2, n - 1]
    for s, p in enumerate(spots[:7]):
        x[s, p] = 5.0 + s
    x[7] = -x[7].abs() - 1.0   # negative only: the identity of the maximum must not be 0
    x[7, spots[7]] = -0.5
    xd, out = dev(x), filled(B, NAN)
    call("falnet_rowmax", L.ptr(xd), L.ptr(out), B, n)
    want = R.rowmax(x)
    assert [float(v) for v in want[:7]] == [5.0 + s for s in range(7)] and float(want[7]) == -0.5
    same(out, want, "rowmax")
    if n % 4 == 0:  # a base pointer off by one float: the scalar path on the same data
        xo = dev(x, off=1)
        out.fill_(NAN)
        call("falnet_rowmax", L.ptr(xo), L.ptr(out), 1, n)  # (B = 1: with B > 1 the samples' alignment alternates, which is the next call)
        assert float(out[0]) == float(want[0]) and torch.isnan(out[1:]).all()
    xo = dev(x[:, :n - 1].contiguous())  # n - 1 elements per sample: samples start at every alignment
    out.fill_(NAN)
    call("falnet_rowmax", L.ptr(xo), L.ptr(out), B, n - 1)
    same(out, R.rowmax(x[:, :n - 1]), "rowmax at n - 1")


@pytest.mark.parametrize("B,Cc,H,W", [(8, 3, 256, 512), (2, 3, 75, 250)])
def test_hflip_and_mask_mix(B, Cc, H, W):
    g = torch.Generator().manual_seed(8)
    a, b = torch.randn(B, Cc, H, W, generator=g), torch.randn(B, Cc, H, W, generator=g)
    ad, bd = dev(a), dev(b)
    out = filled(a.numel(), NAN)
    call("falnet_hflip", L.ptr(ad), L.ptr(out), B * Cc * H, W)
    same(out, R.hflip(a), "hflip")
    assert L.lib().falnet_hflip(L.ptr(ad), L.ptr(ad), B * Cc * H, W, L.stream_ptr()) != 0  # in place is rejected
    # exact inputs: small integers mixed with weights in {0, 1/4, 1/2, 1} -- every product and the sum are exact, fused or not
    ai, bi = torch.randint(-4, 5, (B, Cc, H, W), generator=g).float(), torch.randint(-4, 5, (B, Cc, H, W), generator=g).float()
    m = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, 1, H, W), generator=g)]
    out.fill_(NAN)
    aid, bid, mid = dev(ai), dev(bi), dev(m)
    call("falnet_mask_mix", L.ptr(aid), L.ptr(bid), L.ptr(mid), L.ptr(out), B, Cc, H * W)
    torch.cuda.synchronize()
    same(out, R.mask_mix(ai, bi, m), "mask_mix (exact inputs)")
    mr = torch.rand(B, 1, H, W, generator=g)
    md = dev(mr)
    out.fill_(NAN)
    call("falnet_mask_mix", L.ptr(ad), L.ptr(bd), L.ptr(md), L.ptr(out), B, Cc, H * W)
    _report("mask_mix random", {"rel": R.relerr(out, R.mask_mix(a, b, mr).reshape(-1))}, {"rel": 1e-6})  # (the bound of test_losses for this op)


@pytest.mark.parametrize("B,H,W", [(8, 256, 512), (2, 75, 250)])
def test_occlusion_mask_and_mirror_weight(B, H, W):
    g = torch.Generator().manual_seed(9)
    # exact inputs: masks in {0, 1/2, 1}, per-sample maxima that are powers of two
    a = torch.tensor([0.0, 0.5, 1.0])[torch.randint(0, 3, (B, 1, H, W), generator=g)]
    b = torch.tensor([0.0, 0.5, 1.0])[torch.randint(0, 3, (B, 1, H, W), generator=g)]
    rmax = torch.tensor([2.0 ** (k % 5 + 1) for k in range(B)])
    ad, bd, rd = dev(a), dev(b), dev(rmax)
    c2, c8 = int(0.2 * W), int(0.8 * W)
    for x0, x1 in ((0, c2), (c8, W), (0, W), (c2, c2), (W, W), (0, 0)):  # the training windows, the full width, empty windows
        occ = filled(B * H * W, NAN)
        call("falnet_occlusion_mask", L.ptr(ad), L.ptr(bd), L.ptr(occ), B, H, W, x0, x1)
        want = R.occlusion_mask(a, b, x0, x1)
        same(occ, want, f"occlusion_mask [{x0}, {x1})")
        w = filled(B * H * W, NAN)
        call("falnet_mirror_weight", L.ptr(occ), L.ptr(rd), L.ptr(w), B, H, W, x0, x1)
        same(w, R.mirror_weight(want, rmax, x0, x1), f"mirror_weight [{x0}, {x1})")
    for x0, x1 in ((c2, W), (0, c8)):  # the mirror loss's own windows, on a mask made for the other one
        w = filled(B * H * W, NAN)
        call("falnet_mirror_weight", L.ptr(ad), L.ptr(rd), L.ptr(w), B, H, W, x0, x1)
        same(w, R.mirror_weight(a, rmax, x0, x1), f"mirror_weight [{x0}, {x1})")
    lib, st = L.lib(), L.stream_ptr()
    assert lib.falnet_occlusion_mask(L.ptr(ad), L.ptr(bd), L.ptr(ad), B, H, W, 5, 4, st) != 0   # x0 > x1
    assert lib.falnet_mirror_weight(L.ptr(ad), L.ptr(rd), L.ptr(bd), B, H, W, 0, W + 1, st) != 0  # x1 > W


# ------------------------------------------------------------------------------------------ b. random data against float64
@pytest.mark.parametrize("gamma", [1.0, 2.0])
@pytest.mark.parametrize("B,H,W,x0,x1", K.SMOOTH_EXACT)
def test_smooth_random_vs_f64(B, H, W, x0, x1, gamma):
    _report(f"smooth {B}x{H}x{W} [{x0},{x1}) gamma={gamma:g}", K.smooth_random(B, H, W, x0, x1, gamma))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape", R.L1_RANDOM, ids=lambda s: "x".join(map(str, s)))
def test_l1_random_vs_f64(shape, masked):
    _report(f"l1 {shape} masked={masked}", K.l1_random(shape, masked))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("n", R.MSE_RANDOM)
def test_mse_random_vs_f64(n, dtype):
    """16-bit gradients: the reference uses the rounded operands, so what is left is the output rounding of the gradient: half an ulp of
    the type at the element's own binade (R.half_ulp; `grad` is the worst element over that allowance, <= 1)."""
    one = {"grad": 1.0, "fused_grad": 1.0} if dtype != torch.float32 else None
    _report(f"mse {_ID[dtype]} n={n}", K.mse_random(dtype, n), one)


# ------------------------------------------------------------------------------------------ c. loss-scale path
def _flat_gradient_numel():
    from fal_net_amd import synthetic
    from fal_net_amd.models import FAL_netB
    m = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(49)}, no_levels=49, compute_dtype=torch.float16).to(DEV)
    m.ensure_flat(torch.device(DEV))
    return m.flat_gradients().numel()


def test_grad_guard():
    n = _flat_gradient_numel()
    blocks, th = K.K["GUARD_BLOCKS"], K.RED_THREADS
    sweep, n4 = blocks * th, n // 4
    assert n % 4 == 0 and n > 16_000_000 and n4 % sweep != 0 and n4 > 2 * sweep, (n, n4, sweep)  # several sweeps and a partial last one
    last_sweep = n4 // sweep * sweep
    g = torch.Generator().manual_seed(10)
    x = torch.randn(n, generator=g)
    fmax = float(np.finfo(np.float32).max)
    x[1::1001] = fmax
    x[2::1003] = -fmax
    x[3::1007] = 1e-45      # denormals
    x[4::1009] = -1e-40
    x[5::1013] = -0.0
    x[n - 4:] = torch.tensor([fmax, -fmax, 1e-45, -0.0])
    xd = dev(x)
    lib, st = L.lib(), L.stream_ptr()
    base = [1024.0, 5.0, 0.0, 2.0]
    state = torch.tensor(base, device=DEV)
    call("falnet_grad_guard", L.ptr(xd), n, L.ptr(state))
    assert state.tolist() == base, "finite values (FLT_MAX, denormals, -0.0) must not raise the flag"
    spots = {"element 0": 0, "last element": n - 1, "last partial sweep": 4 * (last_sweep + (n4 - last_sweep) // 2) + 1,
             "lane 37 of a wave, third sweep": 4 * (2 * sweep + 64 * 1000 + 37) + 2, "last float4, first component": n - 4}
    assert spots["last partial sweep"] < n and (spots["lane 37 of a wave, third sweep"] // 4) % 64 == 37
    for where, p in spots.items():
        for bad in (float("inf"), float("-inf"), NAN):
            keep = float(xd[p])
            xd[p] = bad
            state.copy_(torch.tensor(base))
            call("falnet_grad_guard", L.ptr(xd), n, L.ptr(state))
            assert state.tolist() == [1024.0, 5.0, 1.0, 2.0], f"{bad} at {where} (element {p}): state {state.tolist()}"
            xd[p] = keep
    state.copy_(torch.tensor(base))
    call("falnet_grad_guard", L.ptr(xd), n, L.ptr(state))
    assert state.tolist() == base  # restored: clean again
    state[2] = 1.0
    call("falnet_grad_guard", L.ptr(xd), n, L.ptr(state))
    assert state.tolist() == [1024.0, 5.0, 1.0, 2.0]  # the guard only ever raises the flag
    assert lib.falnet_grad_guard(L.ptr(xd), n - 2, L.ptr(state), st) != 0        # n % 4 != 0
    assert lib.falnet_grad_guard(L.ptr(xd[1:]), n - 4, L.ptr(state), st) != 0    # base off by one float
    assert lib.falnet_grad_guard(L.ptr(xd), 0, L.ptr(state), st) != 0


def test_loss_scale_update_follows_the_state_machine():
    args, want = R.SCALE_ARGS, list(R.SCALE_START)
    state = torch.tensor(want, device=DEV)
    inf4 = torch.tensor([0.0, float("inf"), 0.0, 0.0], device=DEV)
    seen = []
    for i, (flag, _) in enumerate(R.SCALE_SCRIPT):
        if flag:
            if i % 2:
                call("falnet_grad_guard", L.ptr(inf4), 4, L.ptr(state))  # the way the flag is raised in training
            else:
                state[2] = 1.0
            want[2] = 1.0
        call("falnet_loss_scale_update", L.ptr(state), *args)
        want = R.loss_scale_update(want, *args)
        got = state.tolist()
        assert got == want, f"step {i}: device {got}, state machine {want}"
        seen.append(got)
    # milestones, by hand (tests/test_loss_ref.py holds the state machine itself to the same list)
    assert seen[1][:2] == [16384.0, 2.0] and seen[2][:2] == [32768.0, 0.0] and seen[5][0] == 65536.0 and seen[8][:2] == [65536.0, 0.0]
    assert seen[9] == [32768.0, 0.0, 0.0, 1.0] and seen[24] == [1.0, 0.0, 0.0, 16.0], "arriving at the floor is not yet the -1 mark"
    assert seen[25] == [1.0, -1.0, 0.0, 17.0] and seen[26] == [1.0, -1.0, 0.0, 18.0] and seen[27] == [1.0, 1.0, 0.0, 18.0]
    assert seen[29] == [2.0, 0.0, 0.0, 18.0] and seen[30] == [1.0, 0.0, 0.0, 19.0]
    lib, st = L.lib(), L.stream_ptr()
    assert lib.falnet_loss_scale_update(L.ptr(state), 0.5, 0.5, 3, 1.0, 2.0, st) != 0 and lib.falnet_loss_scale_update(L.ptr(state), 2.0, 0.5, 0, 1.0, 2.0, st) != 0
    assert state.tolist() == seen[-1]


@pytest.mark.parametrize("n", [3, 64, 100])
def test_loss_seeds(n):
    g = torch.Generator().manual_seed(n)
    coef = torch.randn(n, generator=g)
    state = torch.tensor([8192.0 * 1.25, 7.0, 0.0, 3.0], device=DEV)
    out = filled(n + 8, NAN)
    cd = dev(coef)
    call("falnet_loss_seeds", L.ptr(state), L.ptr(cd), L.ptr(out), n)
    same(out[:n], torch.from_numpy(coef.numpy() * np.float32(8192.0 * 1.25)), "loss_seeds")  # one f32 product: correctly rounded, so ==
    assert torch.isnan(out[n:]).all() and state.tolist() == [10240.0, 7.0, 0.0, 3.0]
    assert (n > K.K["SEEDS_THREADS"]) == (n == 100)  # 100 needs a second trip of the one 64-thread workgroup


def test_step_scalars():
    S, out = torch.tensor([3.25, 1.5], device=DEV), filled(3, NAN)
    call("falnet_step_scalars", L.ptr(S), 0.5, L.ptr(out))
    want, zero = R.step_scalars([3.25, 1.5], 0.5)
    assert out.tolist() == want == [4.0, 3.25, 1.5] and S.tolist() == zero  # exact operands: ==, fused multiply-add or not
    s0, s1, a = 0.7134, 123.456, 0.2 * 2 / 512
    S = torch.tensor([s0, s1], device=DEV)
    f = np.float32
    call("falnet_step_scalars", L.ptr(S), a, L.ptr(out))
    got = out.tolist()
    ref = float(f(s0)) + float(f(a)) * float(f(s1))  # float64 on the stored operands
    assert abs(got[0] - ref) <= 2.0 ** -23 * abs(ref) and got[1:] == [float(f(s0)), float(f(s1))] and S.tolist() == [0.0, 0.0]


def test_adam_step_guarded_skips_or_equals_the_plain_step():
    n = 1 << 20
    g = torch.Generator().manual_seed(11)
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1024.0
    m0, v0 = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    hyper = (0.5, 0.999, 1e-8)
    grd = dev(gr)

    def run(flag, guarded):
        p, m, v = dev(p0), dev(m0), dev(v0)
        st = torch.tensor([1e-4, 3.0], device=DEV)
        if guarded:
            sc = torch.tensor([1024.0, 4.0, float(flag), 1.0], device=DEV)
            call("falnet_adam_step_guarded", L.ptr(p), L.ptr(grd), L.ptr(m), L.ptr(v), n, L.ptr(st), *hyper, 0.5, L.ptr(sc))
            assert sc.tolist() == [1024.0, 4.0, float(flag), 1.0]  # the step reads the scaler state, it does not write it
        else:
            call("falnet_adam_step_dev", L.ptr(p), L.ptr(grd), L.ptr(m), L.ptr(v), n, L.ptr(st), *hyper, 0.5 / 1024.0)
        return p, m, v, st.tolist()
    p, m, v, st = run(1, True)
    assert torch.equal(p.cpu(), p0) and torch.equal(m.cpu(), m0) and torch.equal(v.cpu(), v0) and st[1] == 3.0, "a flagged step must change nothing"
    pg, mg, vg, stg = run(0, True)
    pd, md, vd, std = run(0, False)
    assert torch.equal(pg, pd) and torch.equal(mg, md) and torch.equal(vg, vd) and stg == std and stg[1] == 4.0
    assert not torch.equal(pg.cpu(), p0)
    assert L.lib().falnet_adam_step_guarded(L.ptr(pg), L.ptr(grd), L.ptr(mg), L.ptr(vg), n, L.ptr(torch.zeros(2, device=DEV)), *hyper, 1.0, L.ptr(None),
                                            L.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------ d. ordered reductions
def test_deterministic_reductions_child():
    """FALNET_DETERMINISTIC=1 in a child process (the switch is read when the library loads): the exact cases of (a) give the same
    integers through the ordered tail of red_finish, the accumulate forms still add onto a non-zero scalar, and the random cases of (b)
    give bit-identical scalars on two calls, on another stream, and on a further call (the ticket is back at zero)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_loss_det.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["deterministic"] == 1 and res["exact_cases"] >= 20
    runs = res["scalars"]
    assert len(runs) == 4 and all(len(x) == len(runs[0]) and len(x) >= 10 for x in runs)
    for name, x in zip(("second call", "other stream", "third call"), runs[1:]):
        assert x == runs[0], (name, [(a, b) for a, b in zip(runs[0], x) if a != b])
    for k, v in res["figures"].items():
        assert v <= BOUND, (k, v)


# ------------------------------------------------------------------------------------------ e. the Python surface
def test_loss_functions_surface_at_benchmark_size():
    from fal_net_amd import loss_functions as LF
    B, H, W = 8, 256, 512
    g = torch.Generator().manual_seed(12)
    synth, label = torch.randn(B, 3, H, W, generator=g), torch.randn(B, 3, H, W, generator=g)
    mask = torch.rand(B, 1, H, W, generator=g)
    ld = label.to(DEV)
    for name, mk, ref_mask, a_p in (("mask 1", 1, None, 0.0), ("tensor mask", mask.to(DEV), mask, 0.0), ("scalar mask 0.5", 0.5, torch.full((B, 1, H, W), 0.5), 0.0),
                                    ("a_p without label features", 1, None, 0.01)):
        s = synth.clone().to(DEV).requires_grad_(True)
        loss = LF.rec_loss_fnc(mk, s, ld, None, a_p)
        (loss * 3.0).backward()
        v, gr = R.l1(synth, label, ref_mask)
        _report(f"rec_loss_fnc {name}", {"value": R.relscalar(loss, v), "grad": R.relerr(s.grad, 3.0 * gr)})
    img, disp = R.random_smooth_inputs(B, H, W, 13)
    imd = img.to(DEV)
    for x0, x1 in ((int(0.2 * W), W), (0, int(0.8 * W)), (0, W)):
        d = disp.clone().to(DEV).requires_grad_(True)
        loss = LF.smoothness(imd[:, :, :, x0:x1], d[:, :, :, x0:x1], gamma=2)
        (loss * 0.5).backward()
        v, gr = R.smoothness(img, disp, x0, x1, 2.0)
        assert d.grad.shape == (B, 1, H, W)  # the gradient lands in the uncropped parent
        _report(f"smoothness view [{x0},{x1})", {"value": R.relscalar(loss, v), "grad": R.relerr(d.grad, 0.5 * gr)})
    # mirror loss: occlusion mask, per-sample maximum, weight, masked L1
    a, b = torch.rand(B, 1, H, W, generator=g), torch.rand(B, 1, H, W, generator=g)
    tdisp = torch.rand(B, 1, H, W, generator=g) * 60
    c2, c8 = int(0.2 * W), int(0.8 * W)
    for (o0, o1), (x0, x1) in (((0, c2), (c2, W)), ((c8, W), (0, c8))):
        occ = LF.occlusion_mask(a.to(DEV), b.to(DEV), o0, o1)
        occ_ref = R.occlusion_mask(a.float(), b.float(), o0, o1)
        assert R.relerr(occ, occ_ref) <= 2.0 ** -24  # one f32 product
        d = disp.clone().to(DEV).requires_grad_(True)
        loss = LF.mirror_loss_fnc(d, tdisp.to(DEV), occ, x0, x1)
        loss.backward()
        w = R.mirror_weight(occ.cpu(), R.rowmax(tdisp), x0, x1)
        v, gr = R.l1(disp, tdisp, w, 1.0 / (B * H * (x1 - x0)))
        _report(f"mirror_loss_fnc [{x0},{x1})", {"value": R.relscalar(loss, v), "grad": R.relerr(d.grad, gr)})
