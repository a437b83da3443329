"""The numpy definition of the connected components of a depth or disparity map (include/falnet_hip.h: falnet_components), restated
from that text for tests/test_components_host.py and tests/test_gpu_components.py, and the input families both use.

  valid   lo < v && v <= hi, and with a score map score >= threshold; every comparison with a NaN is false
  edge    right and down 4-neighbours, both valid, max(vp, vq) <= min(vp, vq) * ratio with f32 operands and an np.float32 product,
          ratio = np.float32(1.0 + max_jump): the double sum rounded once
  label   the smallest pixel index of the component, -1 for an invalid pixel; size: the component's pixel count, 0 for an invalid pixel
  info    (components, valid pixels, the largest component's size)

A plain union-find over the two edge arrays: nothing here is shared with the device code."""
import functools
import zlib

import numpy as np

FAMILIES = ("plane", "checker", "rows", "columns", "tie", "spiral", "two-spirals", "serpentine", "comb", "percolation", "walk", "score", "bad", "inf-jump")
VALIDITY_ONLY = ("plane", "spiral", "serpentine", "comb", "percolation", "inf-jump")  # their edges depend on validity alone
LO_V, HI_V = 2.0 ** -20, 2.0 ** 20  # every finite positive value lies in here: no subnormal is probed


def edges(m, max_jump=0.05, lo=0.0, hi=np.inf, score=None, threshold=None):
    """(valid (H, W), right (H, W - 1), down (H - 1, W)) boolean arrays of the definition."""
    m = np.asarray(m, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (np.float32(lo) < m) & (m <= np.float32(hi))
        if score is not None:
            valid &= np.asarray(score, np.float32) >= np.float32(threshold)
        ratio = np.float32(1.0 + float(max_jump))

        def joined(p, q, vp, vq):
            prod = (np.minimum(p, q) * ratio).astype(np.float32)
            return vp & vq & (np.maximum(p, q) <= prod)

        right = joined(m[:, :-1], m[:, 1:], valid[:, :-1], valid[:, 1:])
        down = joined(m[:-1], m[1:], valid[:-1], valid[1:])
    return valid, right, down


def label_ref(m, max_jump=0.05, lo=0.0, hi=np.inf, score=None, threshold=None):
    """(labels (H, W) int32, sizes (H, W) int32, (components, valid, largest))."""
    m = np.asarray(m, np.float32)
    H, W = m.shape
    valid, right, down = edges(m, max_jump, lo, hi, score, threshold)
    parent = list(range(H * W))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    idx = np.arange(H * W).reshape(H, W)
    pairs = [(idx[:, :-1][right], idx[:, 1:][right]), (idx[:-1][down], idx[1:][down])]
    for ps, qs in pairs:
        for p, q in zip(ps.tolist(), qs.tolist()):
            a, b = find(p), find(q)
            if a != b:  # the smaller root stays the root: a root is the smallest index of its set
                parent[max(a, b)] = min(a, b)
    roots = np.array([find(x) for x in range(H * W)], np.int64).reshape(H, W)
    labels = np.where(valid, roots, -1).astype(np.int32)
    counts = np.bincount(labels[valid].astype(np.int64), minlength=H * W)
    sizes = np.where(valid, counts[np.maximum(labels, 0)], 0).astype(np.int32)
    n_comp = int((labels.reshape(-1) == np.arange(H * W)).sum())
    return labels, sizes, (n_comp, int(valid.sum()), int(sizes.max()) if valid.any() else 0)


# ---- input families ---------------------------------------------------------------------------------------------------------------------------------
def _rng(name, H, W):
    return np.random.default_rng(zlib.crc32("{}-{}-{}".format(name, H, W).encode()))


def spiral_path(H, W):
    """A boolean (H, W) mask: one simple path from (0, 0) that winds inwards with one wall pixel between its turns -- a pixel is added only when none
    of its 4-neighbours but the one it comes from is on the path, so the path has no shortcut and is ONE component of its own length."""
    on = np.zeros((H, W), bool)
    on[0, 0] = True
    i, j, d = 0, 0, 0
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(a, b, fi, fj):
        if not (0 <= a < H and 0 <= b < W) or on[a, b]:
            return False
        for di, dj in step:
            c, e = a + di, b + dj
            if (c, e) != (fi, fj) and 0 <= c < H and 0 <= e < W and on[c, e]:
                return False
        return True

    while True:
        for turn in (0, 1):
            nd = (d + turn) % 4
            a, b = i + step[nd][0], j + step[nd][1]
            if free(a, b, i, j):
                on[a, b] = True
                i, j, d = a, b, nd
                break
        else:
            return on


def _walk(rng, H, W, sigma=0.04):
    """A smooth positive map whose neighbour ratios scatter around 1.05: the exponential of a random walk along the rows on one down the first column."""
    steps = rng.normal(0.0, sigma, (H, W))
    steps[:, 0] = np.cumsum(rng.normal(0.0, sigma, H))
    return np.clip(np.exp(np.cumsum(steps, axis=1)) * 4.0, LO_V, HI_V).astype(np.float32)


@functools.lru_cache(maxsize=None)
def family(name, H, W):
    """{"map": (H, W) f32, "kw": the keywords of label_ref / components.label besides the map}, seeded by (name, H, W).  Treat as read-only."""
    rng = _rng(name, H, W)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    nan = np.float32(np.nan)
    kw = {}
    if name == "plane":
        m = np.full((H, W), 5.0, np.float32)
    elif name == "checker":
        m = np.where((ii + jj) % 2 == 0, 1.0, 2.0).astype(np.float32)
    elif name == "rows":
        m = np.where(ii % 2 == 0, 1.0, 2.0).astype(np.float32)
    elif name == "columns":
        m = np.where(jj % 2 == 0, 1.0, 2.0).astype(np.float32)
    elif name == "tie":  # ratio 1.5: 2 | 3 is a tie and joins, 2 | the next float above 3 does not
        above = np.nextafter(np.float32(3.0), np.float32(np.inf))
        m = np.where((ii + jj) % 2 == 0, np.float32(2.0), np.where(rng.random((H, W)) < 0.5, np.float32(3.0), above)).astype(np.float32)
        kw = {"max_jump": 0.5}
    elif name == "spiral":
        m = np.where(spiral_path(H, W), np.float32(1.0), nan)
    elif name == "two-spirals":  # the walls of the spiral are a second winding piece: valid, but a factor 4 away
        m = np.where(spiral_path(H, W), np.float32(1.0), np.float32(4.0))
    elif name == "serpentine":  # even rows, linked through one pixel of the odd row between them at alternating ends
        link = (ii % 2 == 1) & (jj == np.where(ii % 4 == 1, W - 1, 0))
        m = np.where((ii % 2 == 0) | link, np.float32(1.0), nan)
    elif name == "comb":  # teeth on the even columns, joined along the last row only
        m = np.where((jj % 2 == 0) | (ii == H - 1), np.float32(1.0), nan)
    elif name == "percolation":  # the site percolation threshold of the square lattice: components of every size
        m = np.where(rng.random((H, W)) < 0.593, np.float32(1.0), nan)
    elif name == "walk":
        m = _walk(rng, H, W)
    elif name == "score":
        m = _walk(rng, H, W, 0.01)
        score = rng.random((H, W)).astype(np.float32)
        score[rng.random((H, W)) < 0.05] = nan
        kw = {"score": score, "threshold": 0.3}
    elif name == "bad":
        m = _walk(rng, H, W, 0.01)
        pick = rng.random((H, W))
        for k, v in enumerate((nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 1.0, 64.0, 2.0 ** -20, 2.0 ** 20)):
            m[(pick >= 0.02 * k) & (pick < 0.02 * (k + 1))] = np.float32(v)
        kw = {"lo": 2.0, "hi": 8.0}  # the walk starts at 4
    elif name == "inf-jump":
        m = _walk(rng, H, W, 0.5)
        m[rng.random((H, W)) < 0.3] = nan
        kw = {"max_jump": float("inf")}
    else:
        raise KeyError(name)
    m = np.ascontiguousarray(m, np.float32)
    m.setflags(write=False)
    return {"map": m, "kw": kw}


@functools.lru_cache(maxsize=None)
def reference(name, H, W):
    f = family(name, H, W)
    return label_ref(f["map"], **f["kw"])


def speckle_frame(H, W, island=6, seed=3):
    """A `step` scene with speckles, as a disparity map: a far background (8), a near block in the middle (24) and, scattered over the background,
    2 x 3 islands of an in-between disparity (14) -- every island a component of `island` = 6 pixels that the mesh triangulates into four faces.
    -> (img (3, H, W) f32, disp (H, W) f32, the largest island's pixel count)."""
    rng = np.random.default_rng(seed)
    disp = np.full((H, W), 8.0, np.float32)
    disp[H // 3:2 * H // 3, W // 3:2 * W // 3] = 24.0
    for i in range(2, H // 3 - 4, 5):
        for j in range(2, W - 5, 7):
            if rng.random() < 0.7:
                disp[i:i + 2, j:j + 3] = 14.0
    img = rng.uniform(-0.4, 0.5, (3, H, W)).astype(np.float32)
    return img, disp, island
