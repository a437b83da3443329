"""Float64 reference of the per-pixel statistics of the MED distribution (csrc/med_stats.hip, fal_net_amd/confidence.py) for element-wise
tests, a float32 restatement of the same formulas, and the numpy reference of the ordered compaction (csrc/compact.hip).

The reference is assembled from oracle.falnet_oracle.plane_disparities and torch.softmax only, on the float64 image of the stored float32
inputs (a = first index of the largest STORED float32 logit, win = {n : |n - a| <= 1} within [0, N - 1]):

    p = softmax(dlog0, 1)      d = plane_disparities(mn, mx, N)
    mean    sum p_n d_n                         (IS O.med_head's disp: the same expression)
    std     sqrt(sum p_n (d_n - mean)^2)
    entropy -sum p_n ln p_n / ln N
    arg     a                                   conf  sum_win p_n            peak  sum_win p_n d_n / sum_win p_n

Inputs are _head_ref.make_inputs' families a, b, c, d and one family added here, e: family b reversed along the plane axis (falling 3 per
plane), which puts the arg-max at plane 0 and clips the window on the low side; family b clips it at N - 1.

Comparator, unit roundoffs and eta are _head_ref's:  |got - ref| <= u |ref| + c mag + eta.  Magnitudes and coefficients are derived, not fitted
to the kernel (c_disp = _head_ref.coef("disp", case)):

    mean     mag = ref                                    c = c_disp    the same arithmetic as the head's disp: may not be worse
    std      mag = mean_ref + std_ref                     c = 4 c_disp  d(var) <= 2 std d(mean) + c var, so d(std) <= d(mean) + c std / 2; the
                                                                        factor 4 covers the second reduction and the square root
    conf     mag = ref                                    c = 4 c_disp  a sum of positive terms, then one quotient
    peak     mag = ref                                    c = 4 c_disp  a sum of positive terms, then one quotient
    entropy  mag = (ln S + sum p_n |l_n - m|) / ln N      c = 4 c_disp  computed as (ln S - sum p_n (l_n - m)) / ln N, m = l_a, S = sum exp(l_n - m)
                                                                        (ln S as log1p(S - 1), S - 1 summed without plane a's exact 1: at a peaked
                                                                        pixel S = 1 + eps, and log(S) of the ROUNDED S loses eps -- relative to this
                                                                        magnitude, which is of the order of eps there, that form misses any fixed
                                                                        coefficient: float32 torch needed 2.4e-5 with it on the listed cases)
    arg      torch.equal with the first-index arg-max of the stored logits: no tolerance; family c gives 0 everywhere

None of the derived coefficients had to be replaced: the float32 restatement below (f32_eval: plain float32 torch on the CPU) meets every one
of them on every listed case (tests/test_stats_host.py), and so does the kernel (profiles/med_stats_vs_f64.txt, tools/measure_med_stats.py).

Kernel forms: med_stats_kernel<8> (N <= 8), <64> (N <= 64), <128> (N <= 128) and nothing else -- the kernel has no path that depends on W, H or
alignment -- so the listed cases (N = 2, 7 | 9, 49 | 128) reach every form and none is added.
"""
import functools

import numpy as np
import torch

import _head_ref as R
from oracle import falnet_oracle as O

f64 = torch.float64
KINDS = ("mean", "std", "entropy", "arg", "conf", "peak")  # bit k of `which`
ALL = 0b111111

# (B, N, H, W, maxd); inputs are _head_ref.make_inputs' (mx_b = maxd (1 - 0.07 b), mn = mx 2 / 300)
CASES = [
    (1, 2, 2, 40, 30.0),      # smallest N: the window covers both planes
    (2, 7, 3, 40, 30.0),      # B > 1 with per-sample max_disp
    (1, 9, 2, 77, 120.0),     # odd W, one-plane tail
    (2, 49, 2, 128, 300.0),   # the benchmark's N
    (1, 128, 2, 64, 300.0),   # N = HEAD_MAXN
    (1, 49, 2, 1242, 300.0),  # W % 4 != 0, several column blocks
    (1, 7, 1, 2100, 300.0),   # W > 2048
]
SMALL = CASES[:2]
ALL_FAMILIES = ("a", "b", "c", "d", "e")


def families(case):
    """a - e on the first two cases; a, b, e on the rest."""
    return ALL_FAMILIES if case in SMALL else ("a", "b", "e")


def listed():
    return [(c, f) for c in CASES for f in families(c)]


def make_inputs(case, family="a", seed=0):
    """_head_ref.make_inputs, plus family e: family b reversed along the plane axis."""
    if family == "e":
        inp = dict(R.make_inputs(case, "b", seed))
        inp["dlog0"] = inp["dlog0"].flip(1).contiguous()
        inp["family"] = "e"
        return inp
    return R.make_inputs(case, family, seed)


def coef(kind, case):
    c = R.coef("disp", case)
    return c if kind == "mean" else 4.0 * c


def first_argmax(dlog0, last=False):
    """(B, 1, H, W) int64: the first (last: a mutation) index of the largest stored logit along the plane axis."""
    N = dlog0.shape[1]
    idx = torch.arange(N).view(1, N, 1, 1).expand_as(dlog0)
    top = dlog0 == dlog0.amax(1, keepdim=True)
    if last:
        return torch.where(top, idx, torch.full_like(idx, -1)).amax(1, keepdim=True)
    return torch.where(top, idx, torch.full_like(idx, N)).amin(1, keepdim=True)


def _evaluate(dlog0, mn, mx, a, window, dtype, std_form="centred"):
    """The formulas in `dtype` from softmax and plane_disparities; a: the arg-max (B, 1, H, W)."""
    B, N, H, W = dlog0.shape
    l = dlog0.to(dtype)
    d = O.plane_disparities(mn.to(dtype).view(B, 1, 1), mx.to(dtype).view(B, 1, 1), N).view(B, N, 1, 1)
    p = torch.softmax(l, 1)
    idx = torch.arange(N).view(1, N, 1, 1)
    win = ((idx - a).abs() <= window).to(dtype)
    mean = (d * p).sum(1, keepdim=True)
    if std_form == "centred":
        std = (p * (d - mean) ** 2).sum(1, keepdim=True).sqrt()
    else:  # E[d^2] - mean^2: what the bound has to reject
        std = ((p * d * d).sum(1, keepdim=True) - mean * mean).clamp_min(0).sqrt()
    m = l.amax(1, keepdim=True)
    lnN = torch.log(torch.tensor(float(N), dtype=dtype))
    r = {"mean": mean, "std": std, "arg": a.to(dtype)}
    if dtype == f64:
        r["entropy"] = -(p * torch.log(p)).sum(1, keepdim=True) / lnN
        lnS = -torch.log(p.amax(1, keepdim=True))  # S = sum exp(l - m) = 1 / max p
        r["mag_entropy"] = (lnS + (p * (l - m).abs()).sum(1, keepdim=True)) / lnN
    else:  # the form the kernel computes: ln S = log1p(S - 1), S - 1 summed without the arg-max plane's exact 1
        e = torch.exp(l - m)
        lnS = torch.log1p((e * (idx != a).to(dtype)).sum(1, keepdim=True))
        r["entropy"] = (lnS - (e * (l - m)).sum(1, keepdim=True) / e.sum(1, keepdim=True)) / lnN
    conf = (p * win).sum(1, keepdim=True)
    r["conf"] = conf
    r["peak"] = (p * d * win).sum(1, keepdim=True) / conf
    return r


def reference(inp, n_planes=None, window=1, last_tie=False):
    """Float64 outputs and magnitudes of one case: mean, std, entropy, arg, conf, peak and mag_<name>.  Mutations: n_planes < N (the reference
    of the first n_planes planes only), window (planes on either side of the arg-max), last_tie (last-index tie-breaking)."""
    dlog0 = inp["dlog0"] if n_planes is None else inp["dlog0"][:, :n_planes].contiguous()
    a = first_argmax(dlog0, last=last_tie)
    r = _evaluate(dlog0, inp["mn"], inp["mx"], a, window, f64)
    r["mag_mean"], r["mag_conf"], r["mag_peak"] = r["mean"], r["conf"], r["peak"]
    r["mag_std"] = r["mean"] + r["std"]
    return r


def f32_eval(inp, std_form="centred"):
    """The same formulas in plain float32 torch on the CPU (entropy in the kernel's form): shows that the bounds are achievable."""
    return _evaluate(inp["dlog0"], inp["mn"], inp["mx"], first_argmax(inp["dlog0"]), 1, torch.float32, std_form)


@functools.lru_cache(maxsize=None)
def cached(case, family, seed=0):
    """(inputs, reference) of a listed comparison, computed once per process; callers must not modify either."""
    inp = make_inputs(case, family, seed)
    return inp, reference(inp)


def compare_all(case, got, ref, kinds=KINDS):
    """{name: comparator result} of the outputs in `got` ({name: (B, 1, H, W)}) against `ref`; arg is exact: bad = the count of unequal elements."""
    out = {}
    for k in kinds:
        g = got[k].detach().cpu()
        if k == "arg":
            bad = int((g.to(f64) != ref["arg"]).sum())
            out[k] = {"bad": bad, "worst_ratio": float(bad > 0), "maxnorm": float((g.to(f64) - ref["arg"]).abs().max()), "coef": 0.0, "n": g.numel()}
        else:
            out[k] = R.compare(g, ref[k], ref["mag_" + k], torch.float32, coef(k, case))
    return out


# ------------------------------------------------------------------------------------------------------------------- compaction
def compact_ref(records, score, threshold):
    """numpy: the records (n, ...) whose score is >= threshold, in index order; a NaN score compares false and is dropped."""
    with np.errstate(invalid="ignore"):
        keep = np.asarray(score) >= np.float32(threshold)
    return np.asarray(records)[keep]


def make_scores(n, kind, seed=0, threshold=0.5):
    """n float32 scores against `threshold`: 'none' (all below or NaN), 'all' (all at or above, some exactly AT the threshold) or 'half' (about
    half kept, NaNs present)."""
    rng = np.random.default_rng(seed * 7919 + n)
    s = rng.random(n).astype(np.float32)
    if kind == "none":
        s = s * np.float32(0.49)
        s[::5] = np.nan
    elif kind == "all":
        s = np.float32(threshold) + s * np.float32(0.4)
        s[::3] = np.float32(threshold)
    elif kind == "half":
        s[::7] = np.nan
    else:
        raise ValueError(kind)
    return s


def make_records(n, rec_bytes, seed=0):
    """n records: (n,) float32 for 4 bytes, (n, 15) uint8 for 15."""
    rng = np.random.default_rng(seed * 104729 + n + rec_bytes)
    if rec_bytes == 4:
        return rng.standard_normal(n).astype(np.float32)
    return rng.integers(0, 256, (n, rec_bytes), dtype=np.uint8)
