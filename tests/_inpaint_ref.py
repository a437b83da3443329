"""Float64 reference of the background-biased pull-push hole filling (csrc/inpaint.hip, fal_net_amd/inpaint.py) for element-wise tests.

The definition (include/falnet_hip.h, falnet_inpaint_fwd), per image:
  level 0   keep = weight >= floor; w0 = keep ? weight : 0; c0 = keep ? values : 0 (selects); g = exp(-beta guide / guide_scale), 1 when beta = 0
            (guide is not read then); stored triple (cg, wg, a) = (c0 g, w0 g, w0)
  pull      l -> l + 1, sizes (H + 1) // 2, (W + 1) // 2, until 1 x 1: a coarse cell sums its existing fine cells of all C + 2 channels, then all
            channels times 1 / a_sum where a_sum > 1
  apex      div(n, d) = d > 0 ? n / d : 0;  F_L = div(cg, wg), G_L = div(wg, a)
  push      up() = the 2x tent filter (1/4, 3/4; taps clamped; separable);  UG = up(G'), U = div(up(F' G'), UG)
            l >= 1: F = a div(cg, wg) + (1 - a) U, G = a div(wg, a) + (1 - a) UG;   l = 0: out = c0 + (1 - w0) U;   L = 0: out = c0 + (1 - w0) F_0
Inputs are taken as they are (f32 tensors of a test are converted exactly), beta, floor and guide_scale as the f32 values the library receives,
so `keep` is decided identically on both sides.

The bound of the GPU tests:  |got - ref| <= K (L + 1) 2^-24 M,  M = the largest |c0| / w0 over the kept pixels of the image (magnitude()).
K counts, to first order, the f32 roundings of one level in the kernel's order of operations, each in units of u M (u = 2^-24).  Every colour the
algorithm forms is a convex combination of the kept colours, so a rounding of relative size u in a colour-like quantity moves it by at most u M,
and one in a weight-like quantity (wg, G, a, 1 - a: the weights of such a combination) moves the combination by at most 2 u M (the weights'
change times the spread of the colours, at most 2 M).  The contributions of the levels enter `out` through the factors a_l prod_{j<l} (1 - a_j),
which sum to at most 1 over the pull side and add up level by level over the push side, hence the factor (L + 1).
  pull, one level:   cg: 2 additions + the scaling = 3;  wg: the same 3, a weight: 6;  a: 2 additions + the reciprocal + the scaling = 4, a
                     weight: 8                                                                                                       -> 17
  push, one level:   P = F G: 1;  up(P): 2 per pass (two products, one sum; fewer where they contract) = 4;  up(G): 4, a weight: 8;  the division
                     U: 1;  F: div, times a, times U, the sum = 4, and 1 - a, a weight: 2;  G: div, times a, times UG, the sum = 4, a weight: 8 -> 28
  level 0, once:     g: the quotient guide / guide_scale and its product with -beta move the exponent by 2 u |x|, |x| <= 8 PROVIDED 0 <= guide <=
                     guide_scale (the tests keep to that), expf adds at most 2 u: 18 u on a weight = 36; the products c0 g and w0 g: 1 + 2.  With
                     L >= 1 that is at most 39 / 2 per level of (L + 1); with L = 0 there is one pixel, g cancels in div(cg, wg), and 3 remain -> 20
K = 17 + 28 + 20 = 65, written as 64 + 1; it is derived, not fitted: the ratios the kernels reach are recorded in profiles/inpaint_vs_f64.txt."""
import numpy as np

K = 65
U32 = 2.0 ** -24
FLOOR = 2.0 ** -10


def level_sizes(H, W):
    """[(H_l, W_l)] for l = 0..L."""
    out = [(int(H), int(W))]
    while out[-1] != (1, 1):
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def levels(H, W):
    return len(level_sizes(H, W)) - 1


def workspace_floats(C, H, W, images):
    return images * (C + 2) * sum(h * w for h, w in level_sizes(H, W)[1:])


def div(n, d):
    d = np.broadcast_to(d, n.shape)
    out = np.zeros_like(n)
    np.divide(n, d, out=out, where=d > 0)
    return out


def level0(values, weight, guide, guide_scale, beta, floor):
    """(c0 (C, H, W), w0 (H, W), triple (C + 2, H, W)) in float64."""
    values, weight = np.asarray(values, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    keep = weight >= floor
    w0 = np.where(keep, weight, 0.0)
    c0 = np.where(keep[None], values, 0.0)
    if beta == 0:
        g = np.ones_like(w0)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            g = np.where(keep, np.exp(-beta * np.asarray(guide, dtype=np.float64) / guide_scale), 1.0)
    return c0, w0, np.concatenate([np.where(keep[None], c0 * g, 0.0), (w0 * g)[None], w0[None]])


def pull(t):
    """(C + 2, H, W) -> (C + 2, (H + 1) // 2, (W + 1) // 2)."""
    _, h, w = t.shape
    p = np.zeros((t.shape[0], h + h % 2, w + w % 2))
    p[:, :h, :w] = t
    s = (p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) + (p[:, 1::2, 0::2] + p[:, 1::2, 1::2])
    a = s[-1]
    big = a > 1
    return s * np.where(big, 1.0 / np.where(big, a, 1.0), 1.0)


def tent(nf, nc):
    """Taps and weights of the fine indices 0..nf-1 in a coarse level of nc cells."""
    i = np.arange(nf)
    odd = (i % 2) == 1
    t0 = np.where(odd, (i - 1) // 2, i // 2 - 1)
    t1 = t0 + 1
    w0 = np.where(odd, 0.75, 0.25)
    return np.clip(t0, 0, nc - 1), np.clip(t1, 0, nc - 1), w0, 1.0 - w0


def up(x, hf, wf):
    """(..., Hc, Wc) -> (..., hf, wf)."""
    y0, y1, wy0, wy1 = tent(hf, x.shape[-2])
    x0, x1, wx0, wx1 = tent(wf, x.shape[-1])
    r0 = wx0 * x[..., y0[:, None], x0[None, :]] + wx1 * x[..., y0[:, None], x1[None, :]]
    r1 = wx0 * x[..., y1[:, None], x0[None, :]] + wx1 * x[..., y1[:, None], x1[None, :]]
    return wy0[:, None] * r0 + wy1[:, None] * r1


def fill(values, weight, guide=None, guide_scale=None, beta=0.0, floor=FLOOR, bias_in_push=True):
    """One image: values (C, H, W), weight (H, W), guide (H, W) or None -> out (C, H, W) float64.  bias_in_push=False is the variant whose
    bias lives in the pull alone (G = 1 in the push): what the definition is NOT, for the host test of the bias figures."""
    beta, floor = float(np.float32(beta)), float(np.float32(floor))
    if beta != 0:
        guide_scale = float(np.float32(guide_scale))
    c0, w0, t = level0(values, weight, guide, guide_scale, beta, floor)
    C = c0.shape[0]
    pyr = [t]
    while pyr[-1].shape[1:] != (1, 1):
        pyr.append(pull(pyr[-1]))
    top = pyr[-1]
    F, G = div(top[:C], top[C]), div(top[C:C + 1], top[C + 1])
    if not bias_in_push:
        G = np.ones_like(G)
    if len(pyr) == 1:
        return c0 + (1.0 - w0) * F
    for l in range(len(pyr) - 2, -1, -1):
        t = pyr[l]
        hf, wf = t.shape[1:]
        UG = up(G, hf, wf)
        U = div(up(F * G, hf, wf), UG)
        if l == 0:
            return c0 + (1.0 - w0) * U
        a = t[C + 1]
        F = a * div(t[:C], t[C]) + (1.0 - a) * U
        G = a * div(t[C:C + 1], a) + (1.0 - a) * UG if bias_in_push else np.ones_like(UG)


def plain_fill(values, weight, floor=FLOOR):
    """The plain two-channel pull-push (colour, weight; no guide, no G), written on its own: what beta = 0 must equal exactly."""
    values, weight = np.asarray(values, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    keep = weight >= float(np.float32(floor))
    w0 = np.where(keep, weight, 0.0)
    c0 = np.where(keep[None], values, 0.0)
    cs, ws = [c0], [w0]
    while ws[-1].shape != (1, 1):
        both = pull(np.concatenate([cs[-1], ws[-1][None], ws[-1][None]]))
        cs.append(both[:-2])
        ws.append(both[-1])
    F = div(cs[-1], ws[-1])
    if len(ws) == 1:
        return c0 + (1.0 - w0) * F
    for l in range(len(ws) - 2, 0, -1):
        F = ws[l] * div(cs[l], ws[l]) + (1.0 - ws[l]) * up(F, *ws[l].shape)
    return c0 + (1.0 - w0) * up(F, *w0.shape)


def magnitude(values, weight, floor=FLOOR):
    """M: the largest |c0| / w0 over the kept pixels (0 when none is kept)."""
    values, weight = np.asarray(values, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    keep = weight >= float(np.float32(floor))
    if not keep.any():
        return 0.0
    return float((np.abs(values[:, keep]) / weight[keep]).max())


def bound(H, W, M):
    return K * (levels(H, W) + 1) * U32 * M


def step_scene(edge, H=32, W=64, hole=16):
    """The step scene of the bias figures: colour 1 at disparity 100 left of `edge`, colour 0 at disparity 5 right of it, a hole of `hole`
    columns centred on the edge.  -> (values (1, H, W), weight, guide, guide_scale = 100, the hole's mask)."""
    x = np.arange(W)
    colour = np.broadcast_to(np.where(x < edge, 1.0, 0.0), (H, W))
    guide = np.broadcast_to(np.where(x < edge, 100.0, 5.0), (H, W)).copy()
    mask = np.broadcast_to((x >= edge - hole // 2) & (x < edge + hole // 2), (H, W))
    weight = np.where(mask, 0.0, 1.0)
    return (colour * weight)[None], weight, guide, 100.0, mask


# ---- the cases of the GPU tests: shapes, weight families, seeded inputs (f32, so that both sides read the same numbers)
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (7, 9), (64, 64), (65, 63), (129, 200), (37, 124), (75, 250)]
FULL = (375, 1242)
FAMILIES = ("ones", "zero", "one_pixel", "sparse", "dense", "wedge", "floor")


def weights(family, H, W, rng, floor=FLOOR):
    f = np.float32(floor)
    if family == "ones":
        return np.ones((H, W), np.float32)
    if family == "zero":
        return np.zeros((H, W), np.float32)
    if family == "one_pixel":
        w = np.zeros((H, W), np.float32)
        w[rng.integers(H), rng.integers(W)] = 0.625
        return w
    if family == "sparse":
        return np.where(rng.random((H, W)) < 0.05, rng.random((H, W)), 0.0).astype(np.float32)
    if family == "dense":
        return np.where(rng.random((H, W)) < 0.2, 1.0, rng.random((H, W))).astype(np.float32)
    if family == "wedge":  # like a real cover map: full inside, a ramp to 0 over a few columns towards a slanted border, a band of 0 at the top
        y, x = np.mgrid[0:H, 0:W]
        edge = 0.15 * W + 0.2 * y
        w = np.clip((x - edge) / 3.0 + 0.5, 0.0, 1.0)
        w[: max(H // 10, 0)] = 0.0
        return w.astype(np.float32)
    if family == "floor":  # at the floor and at its f32 neighbours, among zeros and ones
        pick = rng.integers(0, 5, (H, W))
        table = np.array([0.0, np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(1)), 1.0], np.float32)
        return table[pick]
    raise ValueError(family)


def inputs(H, W, C, I, family, seed):
    """Seeded f32 inputs of one case: values (I, C, H, W) premultiplied colours in [-1, 1], weight (I, 1, H, W), guide (I, 1, H, W) in
    [0, guide_scale], guide_scale (I,)."""
    rng = np.random.default_rng([seed, H, W, C, I, FAMILIES.index(family)])
    w = np.stack([weights(family, H, W, rng) for _ in range(I)])[:, None]
    colour = rng.uniform(-1.0, 1.0, (I, C, H, W)).astype(np.float32)
    scale = rng.uniform(50.0, 300.0, I).astype(np.float32)
    guide = (rng.random((I, 1, H, W)).astype(np.float32) * scale[:, None, None, None]).astype(np.float32)
    guide = np.minimum(guide, scale[:, None, None, None])
    return {"values": (colour * w).astype(np.float32), "weight": w.astype(np.float32), "guide": guide, "guide_scale": scale}


def reference(inp, beta, floor=FLOOR):
    """-> (out (I, C, H, W) float64, M per image)."""
    I = inp["values"].shape[0]
    outs = [fill(inp["values"][i], inp["weight"][i, 0], inp["guide"][i, 0], inp["guide_scale"][i], beta, floor) for i in range(I)]
    return np.stack(outs), [magnitude(inp["values"][i], inp["weight"][i, 0], floor) for i in range(I)]


_CACHE = {}


def cached(H, W, C, I, family, seed, beta):
    """The inputs and the reference of one case, computed once per process and left unchanged."""
    key = (H, W, C, I, family, seed, float(beta))
    if key not in _CACHE:
        ikey = key[:-1]
        if ikey not in _CACHE:
            _CACHE[ikey] = inputs(H, W, C, I, family, seed)
        _CACHE[key] = (_CACHE[ikey],) + reference(_CACHE[ikey], beta)
    return _CACHE[key]
