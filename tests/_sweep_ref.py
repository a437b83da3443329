"""Float64 reference of the baseline sweep (csrc/med_sweep.hip, fal_net_amd/views.py) for element-wise tests.

The reference is assembled from the oracle's own pieces only (oracle.falnet_oracle.plane_disparities, shift_planes, torch.softmax) on the
float64 image of the stored float32 inputs; for the view at baseline fraction t

    s     = plane_shifts * float(t)                                  (B, N), plane_shifts = d_n (W - 1) / W as _head_ref.plane_shifts
    dprob = softmax(O.shift_planes(dlog0, s), 1)
    view  = sum_n O.shift_planes(left, s[:, n]) * dprob[:, n]        summed in the oracle's order (p = 0; p = p + ...)
    disp  = sum_n d_n dprob_n                                        full-baseline pixels, not scaled by t

so that t = 1 IS O.med_head's p_im0 (difference exactly 0.0) and t = 0 gives `left` to 1e-16 and the forward's `disp` exactly
(tests/test_sweep_host.py).  Magnitudes follow _head_ref: the view's is the two-tap form sum_n (|l[x+k]| + |l[x+k+1]|) dprob_n, k = floor(s)
(the kernel's a = s - floor(s) comes from a float32 table and carries an absolute error of about ulp(s)); disp's magnitude is its own value
(every term is positive).  Comparator, unit roundoffs and eta are _head_ref's:  |got - ref| <= u |ref| + c mag + eta.

Precondition, scaled from _head_ref's: for every view with t != 0, every float64 t s_n must lie at least MARGIN max(1, |t|) from an integer
(the float32 table's error in t s_n grows with |t|).  A (case, set) that fails it is replaced, never masked: (1, 7, 1, 2100, 300) fails it
with set B, which is why that pair is not listed.

Coefficients: the t = 1 VIEW is the head's p_im0 arithmetic and is held to _head_ref.COEF["p_im0"].  For the other views and for the
disparities COEF below was measured on an MI355X against this reference: worst (|got - ref| - u |ref| - eta) / mag over every (case, set)
of CASES, its logit families and seeds 0, 1, 2 (raw figures: profiles/sweep_vs_f64.txt, written by tools/measure_sweep.py), then
_head_ref.round_up_coef: times 4, rounded up to a power of two.
"""
import functools

import torch

import _head_ref as R
from oracle import falnet_oracle as O

f64 = torch.float64
MARGIN = R.MARGIN

SETS = {
    "A": (1.0,),
    "B": (-1.0, -0.5, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0),  # a full launch of 8
    "C": (0.37, -1.63, 1.9),
    "Z": (0.0,),
}
# (B, N, H, W, maxd) -> baseline sets; inputs are _head_ref.make_inputs' (mx_b = maxd (1 - 0.07 b), mn = mx 2 / 300)
CASES = {
    (1, 2, 2, 40, 30.0): "ABCZ",      # smallest N
    (2, 7, 3, 40, 30.0): "ABCZ",      # B > 1 with per-sample mx
    (1, 9, 2, 77, 120.0): "ABCZ",     # odd width, one-plane tail chunk
    (2, 49, 2, 128, 300.0): "ABCZ",   # the benchmark's N
    (1, 128, 2, 64, 300.0): "ABZ",    # N = HEAD_MAXN, shifts far wider than the row: whole planes out of range on both sides
    (1, 49, 2, 1242, 300.0): "ABZ",   # three column blocks, scalar staging (W % 4 != 0)
    (1, 96, 1, 1280, 300.0): "ABCZ",  # 16-byte staging at the deepest prefetch
    (1, 7, 1, 2100, 300.0): "ACZ",    # W > 2048: the global-tap kernel
    # added to the issue's list: the paths of med_sweep.hip none of the above takes
    (1, 7, 1, 1024, 300.0): "ABCZ",   # 16-byte staging at the middle prefetch depth (759 < W <= 1271), two column blocks
    (1, 7, 1, 2048, 300.0): "ACZ",    # the widest staged row: more than 64 KiB of LDS per workgroup
}
SMALL = list(CASES)[:2]


def families(case):
    """a and b everywhere, all four on the first two cases."""
    return R.ALL_FAMILIES if case in SMALL else ("a", "b")


def listed():
    """[(case, set name, family)] of every comparison."""
    return [(c, s, f) for c, sets in CASES.items() for s in sets for f in families(c)]


# COEF[output][class of _head_ref.disp_class]: 4 x the worst observed coefficient, rounded up to a power of two; the observed worst (MI355X,
# seeds 0-2) with the case, set, family and seed that produced it beside each.  "view": the views with t != 1; "disp": every view's disparity.
COEF = {
    "view": {"d30": 2.0 ** -13,   # 2.385e-05  (2, 7, 3, 40, 30) C d seed 0, t = 1.9
             "wide": 2.0 ** -6},  # 3.467e-03  (1, 96, 1, 1280, 300) C b seed 1, t = 1.9
    "disp": {"d30": 2.0 ** -12,   # 3.830e-05  (2, 7, 3, 40, 30) C d seed 2, t = 1.9
             "wide": 2.0 ** -9},  # 2.594e-04  (1, 49, 2, 1242, 300) B a seed 0, t = 1.5
}
# (the t = 1 views, held to _head_ref.COEF["p_im0"] = 2^-15 / 2^-7: observed worst 4.340e-06 (2, 7, 3, 40, 30) A d seed 0 and 4.668e-04
# (1, 128, 2, 64, 300) A b seed 0.  The disparity's coefficient is far above the head's own disp: it is the expectation over the WARPED softmax,
# whose logits carry the float32 table's error in a = t s_n - floor(t s_n) times the logit difference of neighbouring columns, as p_im0 does.)


def coef(output, case, t=None):
    if output == "view" and t == 1.0:
        return R.coef("p_im0", case)  # the same arithmetic as the head's right view: may not be worse
    c = COEF[output][R.disp_class(case)]
    assert c is not None, f"COEF[{output!r}] has not been measured"
    return c


# ------------------------------------------------------------------------------------------------------------------- precondition
def sweep_margin(mn, mx, N, W, ts):
    """min over the views with t != 0 of (distance of the float64 t s_n from an integer) / max(1, |t|); inf when every t is 0."""
    s = R.plane_shifts(mn, mx, N, W)
    worst = float("inf")
    for t in ts:
        if float(t) != 0.0:
            st = s * float(t)
            worst = min(worst, float((st - torch.round(st)).abs().min()) / max(1.0, abs(float(t))))
    return worst


def assert_sweep_margin(mn, mx, N, W, ts):
    m = sweep_margin(mn, mx, N, W, ts)
    assert m >= MARGIN, (f"some float64 t s_n lies {m:.3g} max(1, |t|) from an integer (< {MARGIN}): floor() of a float32 table may differ from the "
                         f"reference's -- replace the case (N={N}, W={W}, mx={mx.tolist()}, t={list(ts)})")
    return m


# ------------------------------------------------------------------------------------------------------------------- reference
def reference(inp, ts, check_margin=True):
    """Float64 views (B, V, 3, H, W), disps (B, V, 1, H, W) and their magnitudes for the baseline fractions `ts`: dict(view, disp, mag_view,
    mag_disp)."""
    dlog0, left, mn, mx = inp["dlog0"].to(f64), inp["left"].to(f64), inp["mn"].to(f64), inp["mx"].to(f64)
    B, N, H, W = dlog0.shape
    if check_margin:
        assert_sweep_margin(inp["mn"], inp["mx"], N, W, ts)
    d = O.plane_disparities(mn.view(B, 1, 1), mx.view(B, 1, 1), N)  # (B, N)
    shifts = R.plane_shifts(inp["mn"], inp["mx"], N, W)
    views, disps, mags = [], [], []
    for t in ts:
        s = shifts * float(t)
        dprob = torch.softmax(O.shift_planes(dlog0, s), 1)
        k = torch.floor(s)
        p, mag = 0, 0
        for n in range(N):
            p = p + O.shift_planes(left, s[:, n:n + 1].expand(B, 3)) * dprob[:, n:n + 1]
            mag = mag + R._two(left, k[:, n:n + 1].expand(B, 3)) * dprob[:, n:n + 1]
        views.append(p)
        mags.append(mag)
        disps.append((d.view(B, N, 1, 1) * dprob).sum(1, keepdim=True))
    disp = torch.stack(disps, 1)
    return {"view": torch.stack(views, 1), "disp": disp, "mag_view": torch.stack(mags, 1), "mag_disp": disp}


def forward_disp(inp):
    """The forward's float64 disparity (B, 1, H, W): what the t = 0 disparity is held to."""
    B = inp["dlog0"].shape[0]
    return O.med_head(inp["dlog0"].to(f64), inp["left"].to(f64), inp["mn"].to(f64).view(B, 1, 1), inp["mx"].to(f64).view(B, 1, 1), True, False, False)["disp"]


@functools.lru_cache(maxsize=None)
def cached(case, set_name, family, seed=0):
    """(inputs, reference) of a listed comparison, computed once per process; callers must not modify either."""
    inp, _ = cached_inputs(case, family, seed)
    return inp, reference(inp, SETS[set_name])


@functools.lru_cache(maxsize=None)
def cached_inputs(case, family, seed=0):
    inp = R.make_inputs(case, family, seed)
    return inp, forward_disp(inp)


def compare_views(case, ts, got_views, got_disps, ref):
    """[(output, view index, t, comparator result)] of every view and disparity of one launch against `ref`."""
    out = []
    for v, t in enumerate(ts):
        if got_views is not None:
            out.append(("view", v, t, R.compare(got_views[:, v], ref["view"][:, v], ref["mag_view"][:, v], torch.float32, coef("view", case, float(t)))))
        if got_disps is not None:
            out.append(("disp", v, t, R.compare(got_disps[:, v], ref["disp"][:, v], ref["mag_disp"][:, v], torch.float32, coef("disp", case))))
    return out
