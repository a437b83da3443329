"""Float64 reference of the MED head (csrc/med_head.hip, med_head2.hip) for element-wise tests, and the comparator they use.

The reference IS oracle.falnet_oracle.med_head run on the float64 image of the stored float32 inputs (the oracle follows its inputs'
dtype): disp, p_im0, maskL, maskR in both maskr_align_corners settings from its forward pass, grad_dlog0 from float64 autograd of
sum(disp * gd) + sum(p_im0 * gp) and of each term alone.  No formula of the head is restated here for a VALUE.

What is added is a per-element MAGNITUDE for every output (the spirit of tests/_conv_ref.py: mag): the same sums with every term replaced
by its absolute value AND every two-tap interpolation (1 - a) t0 + a t1 replaced by |t0| + |t1|.  The second part matters: the kernels
take a = s - floor(s) from a float32 expf / logf table, so a carries an ABSOLUTE error of about ulp(s); relative to a |t1| (a may be
5e-4) that is unbounded, relative to |t0| + |t1| it is ulp(s).  The magnitudes are built from the oracle's own pieces (plane_disparities,
shift_planes with INTEGER shifts, which select single taps, torch.softmax and the oracle's Dprob); test_head_ref.py checks mag >= |ref|.

Bound of an element:   |got - ref| <= u |ref| + c mag + eta
  u    unit roundoff of the stored type (round to nearest, p significant bits: 2^-24 f32, 2^-8 bf16, 2^-11 f16);
  c    the measured coefficient COEF[output][class] below;
  eta  underflow floor of the formats, not of the kernel: the float32 exponentials of planes more than 87 below the maximum are 0 (or
       subnormal), each such term is at most 2^-126 x |gradient| x max disparity (300 < 2^9) x N (<= 2^7) -- 2^-100 is generous and
       thirty orders of magnitude below any value the tests distinguish; an f16 store has subnormal spacing 2^-24.

Precondition, not an exclusion: k_n = floor(s_n) is discontinuous, and a float64 reference disagrees with a float32 table wholesale when
some s_n sits on an integer.  assert_integer_margin() therefore requires every float64 s_n of a case to lie >= MARGIN = 5e-4 from an
integer (the float32 table moves s by about 1e-4 at s = 300); it skips no element and no plane -- a case that fails it is replaced.

COEF was measured on an MI355X against this reference: worst (|got - ref| - u |ref| - eta) / mag over ALL_CASES, their logit families and
seeds 0, 1, 2, times 4, rounded up to a power of two (the inputs are seeded and the kernels have no atomics, so a run repeats; the factor
is for other seeds and another compiler's fast-exp schedule).  FALNET_HEAD_REPORT=<path> makes tests/test_gpu_head.py append its figures
as JSON lines.
"""
import functools
import json
import math
import os

import torch

from oracle import falnet_oracle as O

f64 = torch.float64
MARGIN = 5e-4
U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ETA = {torch.float32: 2.0 ** -100, torch.bfloat16: 2.0 ** -100, torch.float16: 2.0 ** -24}

# (B, N, H, W, maxd); mx_b = maxd (1 - 0.07 b), mn = mx 2 / 300.  OLD_CASES = HEAD_CASES of tests/test_gpu_ops.py.
OLD_CASES = [(2, 7, 6, 40, 30.0), (2, 49, 4, 128, 300.0), (1, 49, 3, 512, 300.0), (1, 96, 2, 320, 300.0), (2, 33, 5, 77, 120.0),
             (1, 96, 2, 1280, 300.0), (1, 49, 2, 1242, 300.0), (1, 7, 1, 2100, 300.0)]
# added: N = 2 and N = HEAD_MAXN = 128 (the ends check_head admits), N = 8 (exactly one chunk), N = 9 (a one-plane tail).
# Kernels they take (falnet_med_head_kernel_name; forward / NHWC backward, the planar backward has one kernel):
#   (1,   2, 2, 40,  30)  med_head_fwd_lds2_kernel / med_head_bwd_lds2_kernel   (six masked planes in the only chunk)
#   (1,   8, 2, 40,  30)  med_head_fwd_lds2_kernel / med_head_bwd_lds2_kernel
#   (1,   9, 2, 40,  30)  med_head_fwd_lds2_kernel / med_head_bwd_lds2_kernel
#   (1, 128, 2, 64, 300)  med_head_fwd_lds_kernel  / med_head_bwd_lds_kernel    (N + 8 > 128: the register plane table does not apply)
NEW_CASES = [(1, 2, 2, 40, 30.0), (1, 8, 2, 40, 30.0), (1, 9, 2, 40, 30.0), (1, 128, 2, 64, 300.0)]
NEW_CASE_KERNELS = {
    (1, 2, 2, 40, 30.0): ("med_head_fwd_lds2_kernel", "med_head_bwd_lds2_kernel"),
    (1, 8, 2, 40, 30.0): ("med_head_fwd_lds2_kernel", "med_head_bwd_lds2_kernel"),
    (1, 9, 2, 40, 30.0): ("med_head_fwd_lds2_kernel", "med_head_bwd_lds2_kernel"),
    (1, 128, 2, 64, 300.0): ("med_head_fwd_lds_kernel", "med_head_bwd_lds_kernel"),
}
ALL_CASES = OLD_CASES + NEW_CASES
SMALL_CASES = [OLD_CASES[0]] + NEW_CASES[:3]
# logit families: a randn * 2; b rising 3 per plane + randn (a new running maximum in every chunk); c all equal; d one plane 100 above the rest
ALL_FAMILIES = ("a", "b", "c", "d")


def families(case):
    """All four on the added cases and the two smallest old ones, (a) and (b) on the wide old ones."""
    return ALL_FAMILIES if case in NEW_CASES or case in OLD_CASES[:2] else ("a", "b")


def disp_class(case):
    """'d30': ulp(s) ~ 2e-6, the float32 table's error is negligible; 'wide' (maxd >= 120): a term ~ ulp(s) |t1 - t0| is not."""
    return "d30" if case[4] <= 30.0 else "wide"


# COEF[output][class]: 4 x the worst observed coefficient, rounded up to a power of two.  Observed worst (MI355X, seeds 0-2) and the
# case, family, seed and output that produced it beside each.  The 'wide' coefficients of p_im0, the masks and the gradient are the float32
# plane table: expf(logf(mx / mn) (c - 1)) carries a relative error of about 1e-6, which is 3e-4 pixels at s = 300, times logit
# differences of about 3 between neighbouring columns in family b.  The d30 ones are __expf at arguments of -100 (family d).
COEF = {
    "disp": {"d30": 2.0 ** -19,    # 4.60e-07  (2, 7, 6, 40, 30) a seed 1, disp
             "wide": 2.0 ** -18},  # 8.23e-07  (1, 96, 2, 320, 300) a seed 0, disp
    "p_im0": {"d30": 2.0 ** -15,   # 6.99e-06  (2, 7, 6, 40, 30) d seed 2, p_im0
              "wide": 2.0 ** -7},  # 1.01e-03  (1, 49, 3, 512, 300) b seed 0, p_im0
    "mask": {"d30": 2.0 ** -14,    # 7.68e-06  (2, 7, 6, 40, 30) d seed 0, maskL
             "wide": 2.0 ** -9},   # 3.10e-04  (2, 33, 5, 77, 120) b seed 0, maskL
    "grad": {"d30": 2.0 ** -14,    # 1.33e-05  (2, 7, 6, 40, 30) d seed 1, planar gradient with both upstream gradients
             "wide": 2.0 ** -7},   # 1.27e-03  (1, 96, 2, 320, 300) b seed 0, planar gradient with both upstream gradients
}


def coef(output, case):
    c = COEF[output][disp_class(case)]
    assert c is not None, f"COEF[{output!r}] has not been measured"
    return c


def round_up_coef(worst):
    """4 x worst, rounded up to a power of two."""
    return 2.0 ** math.ceil(math.log2(4.0 * worst))


# ------------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(case, family="a", seed=0):
    """Stored float32 inputs of one case (CPU): dlog0, left, mn, mx, gd, gp."""
    B, N, H, W, maxd = case
    g = torch.Generator().manual_seed(seed * 100003 + N * 1000 + W)
    base = torch.randn(B, N, H, W, generator=g)
    if family == "a":
        dlog0 = base * 2.0
    elif family == "b":
        dlog0 = base + 3.0 * torch.arange(N, dtype=torch.float32).view(1, N, 1, 1)
    elif family == "c":
        dlog0 = torch.full((B, N, H, W), 0.75)
    elif family == "d":
        dlog0 = base * 2.0
        dlog0[:, N // 3] = dlog0.amax(1) + 100.0
    else:
        raise ValueError(family)
    left = torch.rand(B, 3, H, W, generator=g) - 0.43
    mx = torch.full((B,), maxd) * (1 - 0.07 * torch.arange(B))
    mn = mx * 2 / 300
    gd = torch.randn(B, 1, H, W, generator=g)
    gp = torch.randn(B, 3, H, W, generator=g)
    return {"dlog0": dlog0, "left": left, "mn": mn, "mx": mx, "gd": gd, "gp": gp, "case": case, "family": family, "seed": seed}


def plane_shifts(mn, mx, N, W):
    """float64 s_n = d_n (W - 1) / W of the stored mn, mx -> (B, N)."""
    return O.plane_disparities(mn.to(f64), mx.to(f64), N) * (W - 1) / W


def integer_margin(mn, mx, N, W):
    s = plane_shifts(mn, mx, N, W)
    return float((s - torch.round(s)).abs().min())


def assert_integer_margin(mn, mx, N, W):
    m = integer_margin(mn, mx, N, W)
    assert m >= MARGIN, (f"some float64 plane shift s_n lies {m:.3g} from an integer (< {MARGIN}): floor(s_n) of a float32 table may differ "
                         f"from the reference's -- replace the case (N={N}, W={W}, mx={mx.tolist()}, mn={mn.tolist()})")
    return m


# ------------------------------------------------------------------------------------------------------------------- reference
def _two(t, k):
    """|t| at the two taps of a shift whose integer part is k (per sample and plane): shift_planes with integer shifts selects single taps."""
    t = t.abs()
    return O.shift_planes(t, k) + O.shift_planes(t, k + 1)


def _acfalse_taps(sm, d, weighted):
    """Sum over planes of the four taps FAL_netA's right mask reads (oracle._maskr_align_corners_false: pixel (x, y) reads
    (x W / (W - 1) + d_n - 0.5, y H / (H - 1) - 0.5), zero padding): with the bilinear weights (test_head_ref.py compares that with the
    oracle's grid_sample, so the tap positions are right) or with weight 1 (the magnitude)."""
    B, N, H, W = sm.shape
    ix = torch.arange(W, dtype=f64).view(1, 1, W) * W / (W - 1) + d.view(B, N, 1) - 0.5
    iy = torch.arange(H, dtype=f64) * H / (H - 1) - 0.5 if H > 1 else torch.zeros(1, dtype=f64)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    smp = torch.nn.functional.pad(sm, (1, 1, 1, 1))  # index -1 and W (H) map to the zero border
    acc = 0
    for dy in (0, 1):
        yi = (y0.long() + dy).clamp(-1, H) + 1
        rows = smp[:, :, yi, :]
        wy = (wy1 if dy else 1 - wy1).view(1, 1, H, 1)
        for dx in (0, 1):
            xi = (x0.long() + dx).clamp(-1, W) + 1
            v = torch.gather(rows, 3, xi.view(B, N, 1, W).expand(B, N, H, W))
            wx = (wx1 if dx else 1 - wx1).view(B, N, 1, W)
            acc = acc + (v * wy * wx if weighted else v)
    return acc.sum(1, keepdim=True)


def reference(inp, n_planes=None, check_margin=True):
    """Float64 outputs and magnitudes of one case.  n_planes < N: the reference of the first n_planes planes only (a mutation).
    Keys: disp, p_im0, maskL, maskR, maskR_acfalse, grad_both, grad_disp, grad_pan and mag_<key> for each."""
    dlog0 = inp["dlog0"].to(f64)
    if n_planes is not None:
        dlog0 = dlog0[:, :n_planes].contiguous()
    left, mn, mx = inp["left"].to(f64), inp["mn"].to(f64), inp["mx"].to(f64)
    gd, gp = inp["gd"].to(f64), inp["gp"].to(f64)
    B, N, H, W = dlog0.shape
    if check_margin:
        assert_integer_margin(inp["mn"], inp["mx"], N, W)
    dlog0.requires_grad_(True)
    mnv, mxv = mn.view(B, 1, 1), mx.view(B, 1, 1)
    out = O.med_head(dlog0, left, mnv, mxv, True, True, True)
    r = {"disp": out["disp"].detach(), "p_im0": out["p_im0"].detach(), "maskL": out["maskL"], "maskR": out["maskR"]}
    with torch.no_grad():
        r["maskR_acfalse"] = O.med_head(dlog0.detach(), left, mnv, mxv, True, True, False, maskr_align_corners=False)["maskR"]
    ld, lp = (out["disp"] * gd).sum(), (out["p_im0"] * gp).sum()
    r["grad_disp"] = torch.autograd.grad(ld, dlog0, retain_graph=True)[0]
    r["grad_pan"] = torch.autograd.grad(lp, dlog0, retain_graph=True)[0]
    r["grad_both"] = torch.autograd.grad(ld + lp, dlog0)[0]

    with torch.no_grad():
        d = O.plane_disparities(mnv, mxv, N)
        k = torch.floor(d * (W - 1) / W)
        sm = torch.softmax(dlog0.detach(), 1)
        dprob = out["Dprob"].detach()
        r["mag_disp"] = (d.view(B, N, 1, 1) * sm).sum(1, keepdim=True)
        left2 = torch.stack([_two(left, k[:, n:n + 1].expand(B, 3)) for n in range(N)], 1)  # (B, N, 3, H, W)
        r["mag_p_im0"] = (left2 * dprob.unsqueeze(2)).sum(1)
        r["mag_maskR"] = _two(sm, k).sum(1, keepdim=True)
        r["mag_maskL"] = _two(dprob, -k - 1).sum(1, keepdim=True)
        r["mag_maskR_acfalse"] = _acfalse_taps(sm, d, weighted=False)
        r["mag_grad_disp"] = gd.abs() * sm * (d.view(B, N, 1, 1) + r["disp"])
        src = dprob * (gp.abs().unsqueeze(1) * (left2 + r["mag_p_im0"].unsqueeze(1))).sum(2)  # at the source pixel
        r["mag_grad_pan"] = _two(src, -k - 1)
        r["mag_grad_both"] = r["mag_grad_disp"] + r["mag_grad_pan"]
    return r


@functools.lru_cache(maxsize=None)
def cached(case, family, seed=0):
    """(inputs, reference) of a listed case, computed once per process; callers must not modify either."""
    inp = make_inputs(case, family, seed)
    return inp, reference(inp)


# ------------------------------------------------------------------------------------------------------------------- comparator
def compare(got, ref, mag, dtype, c):
    """Element-wise |got - ref| <= u |ref| + c mag + eta.  Returns dict(bad, worst_ratio, maxnorm, coef): the count of elements over the
    bound (a non-finite `got` counts), the worst |err| / bound, the max-norm error, and the coefficient the worst element would need."""
    got = got.detach().to("cpu").to(f64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    u, eta = U[dtype], ETA[dtype]
    err = (got - ref).abs()
    finite = torch.isfinite(got)
    inf = torch.full_like(err, float("inf"))
    err = torch.where(finite, err, inf)
    bound = u * ref.abs() + c * mag + eta
    excess = err - u * ref.abs() - eta
    need = torch.where(excess > 0, excess / mag.clamp_min(1e-300), torch.zeros_like(err))
    return {"bad": int((~(err <= bound)).sum()), "worst_ratio": float((err / bound).max()), "maxnorm": float(err.max()),
            "coef": float(need.max()), "n": err.numel()}


def report(record):
    path = os.environ.get("FALNET_HEAD_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")
