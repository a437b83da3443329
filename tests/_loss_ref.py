"""Float64 references of the loss and loss-scale kernels of csrc/losses.hip: plain torch / numpy on the CPU, one function per operation.

Used by tests/test_loss_ref.py (CPU: the references against torch autograd in f64, against the oracle and against closed forms) and by
tests/test_gpu_losses.py / tests/_loss_cases.py (GPU: the kernels against the references).  Nothing here imports the library.

Conventions: every function takes CPU tensors of any float dtype, promotes to float64 and returns float64 (value as a 0-d tensor).
`scale` multiplies the SUM (the kernels take 1 / numel for a mean); gradients are d value / d first operand for an upstream gradient of 1.
The smoothness reference is written as explicit shifted slices with a hand-written SCATTER adjoint (each |d_p - d_q| term hands its
sign to p and, when q lies inside the window, minus its sign to q); the kernel uses the gather form and the oracle uses autograd, so the
three share no code.

`python tests/_loss_ref.py` prints the lines of profiles/loss_kernels_vs_f64.txt (reference-side f32 deviations and the bounds derived
from them, see BOUND below).
"""
import numpy as np
import torch

f64 = torch.float64


def _d(t):
    return t.detach().to(f64)


# ------------------------------------------------------------------------------------------ L1 / MSE
def l1(a, b, mask=None, scale=None):
    """value = scale * sum(mask * |a - b|), grad = scale * mask * sign(a - b).  a, b: (B, C, H, W); mask: (B, 1, H, W) or None."""
    a, b = _d(a), _d(b)
    scale = 1.0 / a.numel() if scale is None else scale
    d = a - b
    m = torch.ones((), dtype=f64) if mask is None else _d(mask)
    return scale * (m * d.abs()).sum(), scale * m * torch.sign(d)


def stored(t, dtype):
    """The values a kernel reads: rounded to the operand type, then promoted."""
    return t.detach().to(dtype).to(f64)


def mse(a, b, dtype=torch.float32, scale=None):
    """value = scale * sum((a - b)^2), grad = 2 * scale * (a - b), on the values AS STORED in `dtype` (any shape)."""
    a, b = stored(a, dtype), stored(b, dtype)
    scale = 1.0 / a.numel() if scale is None else scale
    d = a - b
    return scale * (d * d).sum(), 2.0 * scale * d


# ------------------------------------------------------------------------------------------ edge-aware smoothness
GRAY = (0.299, 0.587, 0.114)
MEAN = (0.411, 0.432, 0.45)


def _shift(t, dy, dx):
    """t[y + dy, x + dx] with zeros outside (last two dims), for dy, dx in {-1, 0, 1}."""
    H, W = t.shape[-2:]
    p = torch.zeros(t.shape[:-2] + (H + 2, W + 2), dtype=t.dtype)
    p[..., 1:H + 1, 1:W + 1] = t
    return p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def smoothness(img, disp, x0, x1, gamma, scale=None):
    """Edge-aware smoothness on the column window [x0, x1) of img (B, 3, H, W) and disp (B, 1, H, W): zero padding is applied AFTER the
    crop (the window's neighbours outside it count as 0, gray value and disparity alike).  Returns (value, d value / d disp) with the
    gradient in the UNCROPPED (B, 1, H, W) parent: zero outside the window.  scale defaults to 1 / (B * H * (x1 - x0)) (the mean)."""
    B, _, H, W = disp.shape
    assert 0 <= x0 < x1 <= W
    im, d = _d(img)[:, :, :, x0:x1], _d(disp)[:, 0, :, x0:x1]
    scale = 1.0 / (B * H * (x1 - x0)) if scale is None else scale
    g = sum(GRAY[c] * (im[:, c] + MEAN[c]) for c in range(3))
    wx = torch.exp(-gamma * (-_shift(g, 0, -1) + 2 * g - _shift(g, 0, 1)).abs())
    wy = torch.exp(-gamma * (-_shift(g, -1, 0) + 2 * g - _shift(g, 1, 0)).abs())
    Wc = x1 - x0
    value = torch.zeros((), dtype=f64)
    gp = torch.zeros(B, H + 2, Wc + 2, dtype=f64)  # padded accumulator: what lands in the rim belongs to the padding and is dropped
    for dy, dx, w in ((0, 1, wx), (0, -1, wx), (-1, 0, wy), (1, 0, wy)):
        diff = d - _shift(d, dy, dx)
        value = value + (w * diff.abs()).sum()
        s = w * torch.sign(diff)
        gp[:, 1:H + 1, 1:Wc + 1] += s                          # to the pixel itself
        gp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + Wc] -= s      # to the neighbour it was compared with
    grad = torch.zeros(B, 1, H, W, dtype=f64)
    grad[:, 0, :, x0:x1] = gp[:, 1:H + 1, 1:Wc + 1]
    return scale * value, scale * grad


def smooth_gamma0_int(disp, x0, x1):
    """Closed form of the gamma = 0 case on INTEGER disparities (every weight is exp(-0) = 1): the integer sum of the four absolute
    differences and the integer adjoint, in int64 numpy.  disp: (B, 1, H, W) integer-valued.  Returns (count, adjoint (B, 1, H, W) int64)."""
    d = np.asarray(disp.detach().cpu().numpy()).astype(np.int64)[:, 0, :, x0:x1]
    B, H, Wc = d.shape
    p = np.pad(d, ((0, 0), (1, 1), (1, 1)))
    c = p[:, 1:-1, 1:-1]
    nb = (p[:, 1:-1, 2:], p[:, 1:-1, :-2], p[:, :-2, 1:-1], p[:, 2:, 1:-1])  # right, left, up, down
    count = int(sum(np.abs(c - n).sum() for n in nb))
    inside = np.pad(np.ones_like(d), ((0, 0), (1, 1), (1, 1)))
    ins = (inside[:, 1:-1, 2:], inside[:, 1:-1, :-2], inside[:, :-2, 1:-1], inside[:, 2:, 1:-1])
    # own four terms + the term each in-window neighbour holds on this pixel: d|n - c| / dc = -sign(n - c) = sign(c - n)
    adj = sum(np.sign(c - n) * (1 + i) for n, i in zip(nb, ins))
    out = np.zeros((B, 1, H, disp.shape[3]), dtype=np.int64)
    out[:, 0, :, x0:x1] = adj
    return count, out


# ------------------------------------------------------------------------------------------ Stage-2 helpers
def mask_mix(a, b, m):
    """m * a + (1 - m) * b; m: (B, 1, H, W) broadcast over the channels."""
    a, b, m = _d(a), _d(b), _d(m)
    return m * a + (1.0 - m) * b


def occlusion_mask(a, b, x0, x1):
    """a * b, forced to 1 in the column window [x0, x1)."""
    out = _d(a) * _d(b)
    out[..., x0:x1] = 1.0
    return out


def rowmax(t):
    """Per-sample maximum over everything but the first dim."""
    return _d(t).reshape(t.shape[0], -1).max(dim=1).values


def mirror_weight(occ, rmax, x0, x1):
    """(1 - occ) / rmax[b] inside [x0, x1), 0 outside.  occ: (B, 1, H, W), rmax: (B,)."""
    w = (1.0 - _d(occ)) / _d(rmax).reshape(-1, 1, 1, 1)
    out = torch.zeros_like(w)
    out[..., x0:x1] = w[..., x0:x1]
    return out


def hflip(t):
    """Mirror along the last dim."""
    idx = torch.arange(t.shape[-1] - 1, -1, -1)
    return _d(t).index_select(t.dim() - 1, idx)


# ------------------------------------------------------------------------------------------ dynamic loss scale
def loss_scale_update(state, growth, backoff, interval, min_scale, max_scale):
    """One step of the GradScaler-style state machine over state = [scale, good_steps, overflow_flag, skipped_steps] (float32 values).
    Overflow: the scale backs off (never below min_scale), the step counts as skipped, and good_steps becomes -1 when the scale was
    ALREADY at its floor (the run is diverging), else 0.  Clean: good_steps (a -1 mark counts as 0) grows by one; at `interval` the scale
    grows (never above max_scale) and the count restarts.  The flag is cleared either way."""
    f = np.float32
    scale, good, flag, skipped = (f(x) for x in state)
    if flag != 0:
        at_floor = scale <= f(min_scale)
        scale = max(f(scale * f(backoff)), f(min_scale))
        good = f(-1) if at_floor else f(0)
        skipped = f(skipped + f(1))
    else:
        good = f(max(good, f(0)) + f(1))
        if good >= f(interval):
            scale = min(f(scale * f(growth)), f(max_scale))
            good = f(0)
    return [float(scale), float(good), 0.0, float(skipped)]


# The scripted sequence of the loss-scale tests: (overflow flag of the step, what the step is there to show), with growth 2, back-off 1/2,
# interval 3, floor 1, cap 65536, starting at 16384.
SCALE_ARGS = (2.0, 0.5, 3, 1.0, 65536.0)
SCALE_START = [16384.0, 0.0, 0.0, 0.0]
SCALE_SCRIPT = [(0, ""), (0, ""), (0, "growth after exactly 3 clean steps"), (0, ""), (0, ""), (0, "65536"), (0, ""), (0, ""), (0, "capped")] + \
               [(1, "back-off")] * 16 + [(1, "overflow AT the floor: -1"), (1, "again"), (0, "recovery"), (0, ""), (0, "grows off the floor"), (1, "")]


def step_scalars(S, a):
    """out = {S0 + a * S1, S0, S1}; S is zero afterwards."""
    s0, s1 = float(S[0]), float(S[1])
    return [s0 + float(a) * s1, s0, s1], [0.0, 0.0]


# ------------------------------------------------------------------------------------------ exact-arithmetic inputs
def exact_diff(n, seed, max_sum=1 << 21):
    """Integer differences d in {0, +-1, +-2} (int8, flat, n elements) whose density keeps sum|d| and sum d^2 far below 2^24, plus a base
    b in {0..3}: a = b + d and b are small integers, exact in f32, bf16 and f16.  Returns (a, b, d) as int8 tensors."""
    g = torch.Generator().manual_seed(seed)
    k = max(1, min(n // 4, max_sum // 4))  # every non-zero adds at most 4 to sum d^2
    d = torch.zeros(n, dtype=torch.int8)
    idx = torch.randint(0, n, (k,), generator=g)
    vals = torch.tensor([-2, -1, 1, 2], dtype=torch.int8)[torch.randint(0, 4, (k,), generator=g)]
    d[idx] = vals
    b = torch.randint(0, 4, (n,), generator=g, dtype=torch.int8)
    return b + d, b, d


def plant(a, b, d, positions, value=2):
    """Impulses of `value` at flat `positions` (a = b + d kept consistent)."""
    for p in positions:
        if 0 <= p < d.numel():
            d[p] = value
            a[p] = b[p] + value
    return a, b, d


def exact_counts(d):
    """(sum |d|, sum d^2) of an integer difference tensor as Python ints; asserts both stay below 2^24 (exact in f32 in ANY order)."""
    d64 = d.to(torch.int64)
    s1, s2 = int(d64.abs().sum()), int((d64 * d64).sum())
    assert s1 < (1 << 24) and s2 < (1 << 24), (s1, s2)
    return s1, s2


def plateau_disp(B, H, W, seed):
    """Integer disparities in {0..3} with plateaus (3 x 3 blocks of a coarse random grid, then one third of the pixels re-drawn)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, 4, (B, 1, (H + 2) // 3, (W + 2) // 3), generator=g)
    d = coarse.repeat_interleave(3, dim=2).repeat_interleave(3, dim=3)[:, :, :H, :W].clone()
    redraw = torch.rand(B, 1, H, W, generator=g) < (1.0 / 3.0)
    d[redraw] = torch.randint(0, 4, (int(redraw.sum()),), generator=g)
    return d.to(torch.float32)


# ------------------------------------------------------------------------------------------ bounds of the random-data cases
# profiles/loss_kernels_vs_f64.txt: on the SAME inputs, how far the f32 CPU expression (the oracle's smoothness, torch's f32 L1 / MSE) is
# from these float64 references.  The bound of a case is MARGIN * max(that deviation, FLOOR): FLOOR is the project's existing bound for
# these ops (tests/test_gpu_ops.py::test_losses, 1e-5), MARGIN = 4 covers __expf and the kernels' different summation order.
FLOOR = 1e-5
MARGIN = 4.0


def bound(dev):
    return MARGIN * max(float(dev), FLOOR)


# 16-bit MSE gradients: the reference uses the operands as stored, so what is left is the rounding of the gradient itself to the
# type: HALF AN ULP of the type at that element.  bf16 carries 8 significant bits, f16 11: the spacing in the binade [2^e, 2^(e+1)) is
# 2^(e - 7) / 2^(e - 10), half of it 2^(e - 8) / 2^(e - 11) -- relative to the element between 2^-9 (top of the binade) and 2^-8
# (bottom) for bf16, 2^-12 .. 2^-11 for f16.  A bound of 2^-9 / 2^-12 times the ELEMENT cannot be met by any correctly rounding
# kernel (a value just above 1 + 2^-8 rounds to 1 or 1 + 2^-7 in bf16: 2^-8 off); the spacing is taken at the element's own binade.
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}  # below 2^MIN_EXP the spacing stays that of the lowest normal binade (subnormals)


def half_ulp(ref, dtype):
    """Half the spacing of `dtype` at every element of the float64 tensor `ref`."""
    _, e = torch.frexp(ref.abs())  # ref = m * 2^e with m in [0.5, 1): the binade is [2^(e - 1), 2^e)
    e = torch.clamp(e.to(f64) - 1.0, min=float(MIN_EXP[dtype]))
    return torch.pow(torch.tensor(2.0, dtype=f64), e - SIG_BITS[dtype])


def relerr(got, ref):
    """max |got - ref| / max |ref| (the `rel` of tests/test_gpu_ops.py)."""
    got, ref = _d(got).cpu(), _d(ref).cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _f(x):
    return float(x.detach()) if torch.is_tensor(x) else float(x)


def relscalar(got, ref):
    return abs(_f(got) - _f(ref)) / max(abs(_f(ref)), 1e-300)


SMOOTH_CASES = [  # (B, H, W, [(x0, x1), ...]): shared by the exact (gamma = 0) and the random (gamma = 1, 2) smoothness cases
    (8, 256, 512, [(102, 512), (0, 409), (0, 512)]),   # int(0.2 W), int(0.8 W): the training scripts' windows at that width
    (2, 75, 250, [(50, 250), (0, 200), (0, 250)]),
    (3, 37, 131, [(63, 129), (70, 90), (64, 128), (0, 131), (77, 78)]),  # ... and a one-column window
    (2, 1, 200, [(0, 200), (40, 200)]),
    (2, 17, 130, [(0, 130), (26, 130)]),
]
L1_RANDOM = [(2, 3, 12, 40), (8, 3, 256, 512), (1, 3, 75, 250)]
MSE_RANDOM = [(6 * 131072 + 37) * 8, 320003]  # both MSE loops of the vector form; the scalar form


def random_smooth_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, H, W, generator=g) - 0.43
    disp = torch.rand(B, 1, H, W, generator=g) * 30 + 2
    return img, disp


def f32_smooth_deviation(B, H, W, x0, x1, gamma, seed=11):
    """(scalar deviation, gradient deviation) of the f32 CPU oracle from the float64 reference on random_smooth_inputs."""
    import os
    import sys
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    from oracle import falnet_oracle as O
    img, disp = random_smooth_inputs(B, H, W, seed)
    dsp = disp.clone().requires_grad_(True)
    v32 = O.smoothness(img[:, :, :, x0:x1], dsp[:, :, :, x0:x1], gamma)
    v32.backward()
    v, g = smoothness(img, disp, x0, x1, gamma)
    return relscalar(v32, v), relerr(dsp.grad, g)


def f32_l1_deviation(shape, masked, seed=12):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    m = torch.rand(shape[0], 1, shape[2], shape[3], generator=g) if masked else None
    a32 = a.clone().requires_grad_(True)
    v32 = ((1 if m is None else m) * (a32 - b).abs()).mean()
    v32.backward()
    v, gr = l1(a, b, m)
    return relscalar(v32, v), relerr(a32.grad, gr)


def f32_mse_deviation(n, seed=13):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    a32 = a.clone().requires_grad_(True)
    v32 = ((a32 - b) ** 2).mean()
    v32.backward()
    v, gr = mse(a, b)
    return relscalar(v32, v), relerr(a32.grad, gr)


def profile_lines():
    out = ["# Reference-side deviations of the loss kernels' random-data cases (tests/test_gpu_losses.py, section b).",
           "# dev_*  : the f32 CPU expression (oracle smoothness, torch f32 L1 / MSE) against the float64 reference of tests/_loss_ref.py on the",
           "#          test's own inputs: scalar relative, gradient max-abs over max-abs.",
           f"# bound_*: {MARGIN:g} x max(dev, {FLOOR:g}).  {FLOOR:g} is the existing bound of these ops in tests/test_gpu_ops.py::test_losses; the",
           f"#          factor {MARGIN:g} is the margin for __expf and for the kernels' summation order (grid-stride partial sums, wave shuffles,",
           "#          one atomic per workgroup), so every bound here is 4e-5 where test_losses has 1e-5: the cases are up to 2^15 times larger and",
           "#          every deviation below is under the floor, i.e. the floor, not a measurement of the kernels, sets the bound.",
           "# 16-bit MSE gradients: the reference uses the rounded operands, what remains is the output rounding: half an ulp of the type at the",
           "#          element's own binade (8 significant bits bf16, 11 f16; relative to the element that is 2^-9 .. 2^-8 and 2^-12 .. 2^-11) --",
           "#          reasoned, not measured; see half_ulp in tests/_loss_ref.py.",
           "# case dev_scalar dev_grad bound_scalar bound_grad"]
    for B, H, W, wins in SMOOTH_CASES:
        for x0, x1 in wins:
            for gamma in (1.0, 2.0):
                ds, dg = f32_smooth_deviation(B, H, W, x0, x1, gamma)
                out.append(f"smooth_{B}x{H}x{W}_win{x0}-{x1}_gamma{gamma:g} {ds:.3e} {dg:.3e} {bound(ds):.3e} {bound(dg):.3e}")
    for shape in L1_RANDOM:
        for masked in (False, True):
            ds, dg = f32_l1_deviation(shape, masked)
            out.append(f"l1_{'x'.join(map(str, shape))}_{'masked' if masked else 'plain'} {ds:.3e} {dg:.3e} {bound(ds):.3e} {bound(dg):.3e}")
    for n in MSE_RANDOM:
        ds, dg = f32_mse_deviation(n)
        out.append(f"mse_f32_n{n} {ds:.3e} {dg:.3e} {bound(ds):.3e} {bound(dg):.3e}")
    return out


if __name__ == "__main__":
    print("\n".join(profile_lines()))
