"""CPU: the float64 references of the loss kernels (tests/_loss_ref.py) against torch autograd in f64, against the oracle's smoothness,
and against the closed forms of the exact cases of tests/test_gpu_losses.py -- so that the reference cannot be wrong unnoticed.  Also the
launch arithmetic of tests/_loss_cases.py (which loop each GPU case reaches) and profiles/loss_kernels_vs_f64.txt against the constants
the GPU module takes from it."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import falnet_oracle as O

import _loss_cases as K
import _loss_ref as R

f64 = torch.float64
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=f64), torch.as_tensor(b, dtype=f64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, rtol=tol, atol=tol), float((a - b).abs().max())


SMALL_SMOOTH = [(2, 5, 9, 0, 9), (2, 5, 9, 2, 9), (2, 5, 9, 0, 6), (1, 1, 7, 0, 7), (1, 1, 7, 3, 4), (3, 4, 6, 5, 6), (2, 17, 70, 3, 67), (1, 6, 1, 0, 1)]


@pytest.mark.parametrize("gamma", [1.0, 2.0, 0.0])
@pytest.mark.parametrize("B,H,W,x0,x1", SMALL_SMOOTH)
def test_smoothness_reference_vs_oracle_and_autograd(B, H, W, x0, x1, gamma):
    """Value against O.smoothness on the cropped tensors in f64; gradient against autograd THROUGH the crop, so it lands in the parent."""
    g = _g(B * 100 + H * 10 + W)
    img = torch.rand(B, 3, H, W, generator=g, dtype=f64) - 0.43
    disp = (torch.rand(B, 1, H, W, generator=g, dtype=f64) * 30 + 2).requires_grad_(True)
    want = O.smoothness(img[:, :, :, x0:x1], disp[:, :, :, x0:x1], gamma)
    want.backward()
    v, gr = R.smoothness(img, disp, x0, x1, gamma)
    _close(v, want.detach())
    _close(gr, disp.grad)
    assert gr.shape == (B, 1, H, W) and float(gr[..., :x0].abs().sum()) == 0.0 and float(gr[..., x1:].abs().sum()) == 0.0
    v2, gr2 = R.smoothness(img, disp, x0, x1, gamma, scale=0.125)  # an explicit scale replaces the mean
    _close(v2, want.detach() * 0.125 * B * H * (x1 - x0))
    _close(gr2, disp.grad * 0.125 * B * H * (x1 - x0))


def test_smoothness_reference_uses_the_kernel_constants():
    """gray_at of losses.hip: 0.299 (r + 0.411) + 0.587 (g + 0.432) + 0.114 (b + 0.45), zero OUTSIDE the window (not the gray of a zero image)."""
    src = open(os.path.join(ROOT, "fal_net_amd", "csrc", "losses.hip")).read()
    assert "0.299f * (im[o] + 0.411f) + 0.587f * (im[HW + o] + 0.432f) + 0.114f * (im[2 * HW + o] + 0.45f)" in src
    assert R.GRAY == (0.299, 0.587, 0.114) and R.MEAN == (0.411, 0.432, 0.45)
    # one bright column in a constant image, window of that column only: its neighbours are PADDING (0), so |dx| = 2 gray
    img = torch.zeros(1, 3, 1, 5, dtype=f64)
    disp = torch.tensor([[[[7.0, 7.0, 3.0, 7.0, 7.0]]]], dtype=f64)
    gray = 0.299 * 0.411 + 0.587 * 0.432 + 0.114 * 0.45
    v, gr = R.smoothness(img, disp, 2, 3, 1.0, scale=1.0)
    _close(v, 4 * 3.0 * np.exp(-2 * gray))  # four neighbours, all padding: |3 - 0| each; wx = wy = exp(-|2 gray|)
    _close(gr[0, 0, 0], torch.tensor([0.0, 0.0, 4 * np.exp(-2 * gray), 0.0, 0.0], dtype=f64))


@pytest.mark.parametrize("masked", [False, True])
def test_l1_reference_vs_autograd(masked):
    g = _g(3)
    a = torch.randn(2, 3, 5, 7, generator=g, dtype=f64).requires_grad_(True)
    b = torch.randn(2, 3, 5, 7, generator=g, dtype=f64)
    b[0, 0, 0, :3] = a.detach()[0, 0, 0, :3]  # exact ties: sign(0) = 0
    m = torch.rand(2, 1, 5, 7, generator=g, dtype=f64) if masked else None
    want = torch.mean((1 if m is None else m) * (a - b).abs())
    want.backward()
    v, gr = R.l1(a, b, m)
    _close(v, want.detach())
    _close(gr, a.grad)
    assert float(gr[0, 0, 0, :3].abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_mse_reference_rounds_first(dtype):
    g = _g(4)
    a, b = torch.randn(3, 40, generator=g), torch.randn(3, 40, generator=g)
    ar = a.to(dtype).to(f64).requires_grad_(True)
    br = b.to(dtype).to(f64)
    want = ((ar - br) ** 2).mean()
    want.backward()
    v, gr = R.mse(a, b, dtype)
    _close(v, want.detach())
    _close(gr, ar.grad)
    if dtype != torch.float32:
        assert not torch.allclose(gr, 2.0 / a.numel() * (a.to(f64) - b.to(f64)), rtol=1e-6, atol=0)  # the rounding is in there


def test_stage2_helpers_vs_torch():
    g = _g(5)
    B, H, W = 3, 9, 40
    a, b = torch.rand(B, 1, H, W, generator=g, dtype=f64), torch.rand(B, 1, H, W, generator=g, dtype=f64)
    c2, c8 = int(0.2 * W), int(0.8 * W)
    ref = a * b
    ref[:, :, :, 0:c2] = 1
    _close(R.occlusion_mask(a, b, 0, c2), ref)
    _close(R.occlusion_mask(a, b, 7, 7), a * b)  # empty window
    t = torch.rand(B, 1, H, W, generator=g, dtype=f64) * 60
    _close(R.rowmax(t), F.max_pool2d(t, kernel_size=(H, W)).reshape(B))
    _close(R.rowmax(-t - 1.0), -(t + 1.0).reshape(B, -1).min(1).values)  # negative only
    w = R.mirror_weight(ref, R.rowmax(t), c2, W)
    want = (1 / F.max_pool2d(t, kernel_size=(H, W))) * (1 - ref)
    _close(w[..., c2:], want[..., c2:])
    assert float(w[..., :c2].abs().sum()) == 0.0 and float(R.mirror_weight(ref, R.rowmax(t), 5, 5).abs().sum()) == 0.0
    x, y = torch.randn(B, 3, H, W, generator=g, dtype=f64), torch.randn(B, 3, H, W, generator=g, dtype=f64)
    _close(R.mask_mix(x, y, a), a * x + (1 - a) * y)
    _close(R.hflip(x), torch.flip(x, [3]))
    # the mirror loss of the training script (mean over the window of w |d - t|) is the masked L1 at scale 1 / (B H Wc)
    d = (torch.rand(B, 1, H, W, generator=g, dtype=f64) * 50).requires_grad_(True)
    loss = torch.mean(want[..., c2:] * torch.abs(d - t)[..., c2:])
    loss.backward()
    v, gr = R.l1(d, t, w, 1.0 / (B * H * (W - c2)))
    _close(v, loss.detach())
    _close(gr, d.grad)


def test_loss_scale_state_machine_milestones():
    """The scripted sequence of test_gpu_losses.py, by hand: growth after exactly `interval` clean steps, the cap, back-off, arriving at
    the floor without the -1 mark, a further overflow at the floor with it, recovery, the skipped counter."""
    args = R.SCALE_ARGS
    st, seen = list(R.SCALE_START), []
    for flag, _ in R.SCALE_SCRIPT:
        st = R.loss_scale_update(st[:2] + [float(flag)] + st[3:], *args)
        assert st[2] == 0.0
        seen.append(st)
    assert [s[:2] for s in seen[:3]] == [[16384.0, 1.0], [16384.0, 2.0], [32768.0, 0.0]]
    assert seen[5][:2] == [65536.0, 0.0] and seen[8] == [65536.0, 0.0, 0.0, 0.0]                      # capped
    assert [s[0] for s in seen[9:25]] == [2.0 ** k for k in range(15, -1, -1)] and all(s[1] == 0.0 for s in seen[9:25])
    assert seen[24] == [1.0, 0.0, 0.0, 16.0] and seen[25] == [1.0, -1.0, 0.0, 17.0] and seen[26] == [1.0, -1.0, 0.0, 18.0]
    assert seen[27] == [1.0, 1.0, 0.0, 18.0] and seen[28] == [1.0, 2.0, 0.0, 18.0] and seen[29] == [2.0, 0.0, 0.0, 18.0]
    assert seen[30] == [1.0, 0.0, 0.0, 19.0] and len(seen) == 31
    # a floor above 1 and a back-off that would undershoot it
    assert R.loss_scale_update([6.0, 4.0, 1.0, 0.0], 2.0, 0.5, 3, 4.0, 64.0) == [4.0, 0.0, 0.0, 1.0]
    assert R.step_scalars([3.25, 1.5], 0.5) == ([4.0, 3.25, 1.5], [0.0, 0.0])


def test_exact_case_generators_and_closed_forms():
    """The inputs of the exact GPU cases: small integers, counts below 2^24, and the references reproduce the closed forms to the unit."""
    a, b, d = R.exact_diff(100003, 1)
    assert torch.equal(a - b, d) and int(d.abs().max()) == 2 and int(a.min()) >= -2 and int(a.max()) <= 5 and (d == 0).float().mean() > 0.5
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert torch.equal(a.to(dt).to(torch.int8), a)  # stored exactly
    R.plant(a, b, d, [0, 100002, 200000], value=-2)
    assert torch.equal(a - b, d) and int(d[0]) == -2 and int(d[-1]) == -2
    s1, s2 = R.exact_counts(d)
    v, gr = R.l1(a.reshape(1, 1, 1, -1), b.reshape(1, 1, 1, -1), None, 2.0 ** -12)
    assert float(v) == s1 * 2.0 ** -12 and torch.equal(gr.reshape(-1), 2.0 ** -12 * torch.sign(d.double()))
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        v, gr = R.mse(a, b, dt, 2.0 ** -12)
        assert float(v) == s2 * 2.0 ** -12 and torch.equal(gr, 2.0 ** -11 * d.double())
    with pytest.raises(AssertionError):
        R.exact_counts(torch.full((1 << 23,), 2, dtype=torch.int8))  # sum d^2 = 2^25: not exact in f32 any more
    _, _, big = R.exact_diff(8 * 256 * 512 * 64, 5, 1 << 20)        # the benchmark's slice 1 stays far below 2^24
    assert R.exact_counts(big)[1] <= 1 << 20


@pytest.mark.parametrize("B,H,W,x0,x1", K.SMOOTH_EXACT)
def test_smoothness_gamma0_closed_form(B, H, W, x0, x1):
    """gamma = 0 on integer disparities: the float64 reference equals the int64 count and adjoint exactly, and the case is one the
    GPU test can hold to == (count below the f32-exact range after the accumulate forms have doubled it; plateaus present)."""
    disp = R.plateau_disp(B, H, W, 4)
    assert torch.equal(disp, disp.round()) and float(disp.min()) >= 0 and float(disp.max()) <= 3
    img = torch.rand(B, 3, H, W, generator=_g(5)) - 0.43
    count, adj = R.smooth_gamma0_int(disp, x0, x1)
    v, gr = R.smoothness(img, disp, x0, x1, 0.0, scale=2.0 ** -20)
    assert float(v) == count * 2.0 ** -20
    assert torch.equal(gr, torch.from_numpy(adj).double() * 2.0 ** -20)
    assert 2 * count + 3 * (1 << 20) < (1 << 24) and (adj == 0).any() and (adj != 0).any() and np.abs(adj).max() <= 8
    win = disp[:, 0, :, x0:x1]
    if x1 - x0 > 1:
        assert (win[:, :, 1:] == win[:, :, :-1]).any(), "no plateau: sgn(0) would go unexercised"
    assert not adj[..., :x0].any() and not adj[..., x1:].any()


def test_launch_arithmetic_reaches_every_loop():
    """tests/_loss_cases.py restates the launch code of losses.hip from the constants it parses out of the source; this is the table in
    the docstring of tests/test_gpu_losses.py, computed -- on the CPU too, so a change of RED_BLOCKS or SM_TX fails here first."""
    assert K.CAP == 131072 and K.K["GUARD_BLOCKS"] == 1024
    K.check_coverage()
    assert K.mse3_begin(K.BENCH_SLICES) == [0, 292, 438, 512] and K.mse3_begin(K.MSE3_SMALLEST_FIRST)[:2] == [0, 16]
    assert K.unrolled_loops(3 * K.CAP, K.CAP) == (0, 3, 0) and K.unrolled_loops(4 * K.CAP, K.CAP) == (1, 0, 0)


def test_profile_file_matches_the_bounds():
    """profiles/loss_kernels_vs_f64.txt: one line per random-data case, bound = 4 x max(deviation, 1e-5), and no deviation above the floor
    (which is what lets tests/test_gpu_losses.py use the single constant BOUND = 4e-5).  One case is re-measured here."""
    lines = [l.split() for l in open(os.path.join(ROOT, "profiles", "loss_kernels_vs_f64.txt")) if l.strip() and not l.startswith("#")]
    names = {l[0] for l in lines}
    for B, H, W, wins in R.SMOOTH_CASES:
        for x0, x1 in wins:
            for gamma in (1, 2):
                assert f"smooth_{B}x{H}x{W}_win{x0}-{x1}_gamma{gamma}" in names
    for shape in R.L1_RANDOM:
        for kind in ("plain", "masked"):
            assert f"l1_{'x'.join(map(str, shape))}_{kind}" in names
    for n in R.MSE_RANDOM:
        assert f"mse_f32_n{n}" in names
    for name, ds, dg, bs, bg in lines:
        assert float(ds) <= R.FLOOR and float(dg) <= R.FLOOR, name
        assert float(bs) == pytest.approx(R.bound(float(ds))) and float(bg) == pytest.approx(R.bound(float(dg))), name
        assert float(bs) == pytest.approx(4e-5) and float(bg) == pytest.approx(4e-5)
    ds, dg = R.f32_smooth_deviation(3, 37, 131, 63, 129, 2.0)
    rec = next(l for l in lines if l[0] == "smooth_3x37x131_win63-129_gamma2")
    assert ds == pytest.approx(float(rec[1]), rel=0.5, abs=2e-8) and dg == pytest.approx(float(rec[2]), rel=0.5, abs=2e-8)


def test_half_ulp_is_the_spacing_of_the_type():
    """R.half_ulp against torch's own rounding: the worst rounding error of x -> dtype over a dense sweep equals half the spacing and never
    exceeds it; relative to the element it lies between 2^-9 and 2^-8 (bf16) / 2^-12 and 2^-11 (f16), subnormals aside."""
    x = torch.linspace(0.011, 7.9, 400001, dtype=f64).float().double()  # f32 values: ONE rounding on the way to the 16-bit type
    for dt, lo in ((torch.bfloat16, 2.0 ** -9), (torch.float16, 2.0 ** -12)):
        assert torch.finfo(dt).eps == 2.0 ** (1 - R.SIG_BITS[dt])
        err, h = (x.float().to(dt).to(f64) - x).abs(), R.half_ulp(x, dt)
        assert bool((err <= h).all()) and float((err / h).max()) > 0.99
        assert float((h / x).min()) > lo and float((h / x).max()) <= 2 * lo and float((err / x).max()) > 1.5 * lo
    tiny = torch.tensor([1e-6, 3e-8, 6.0e-5], dtype=f64).float().double()  # f16 subnormals: multiples of 2^-24
    assert bool(((tiny.float().to(torch.float16).to(f64) - tiny).abs() <= R.half_ulp(tiny, torch.float16)).all())
    assert R.half_ulp(tiny, torch.float16)[:2].tolist() == [2.0 ** -25, 2.0 ** -25]
