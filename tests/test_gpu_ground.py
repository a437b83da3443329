"""GPU: the ground plane (fal_net_amd/ground.py, csrc/ground.hip) against its definition on the host (tests/_ground_ref.py).

hypotheses, consensus, heights, split: every comparison is == on bits, integers or bytes.  Both sides do the same correctly rounded IEEE operations
in the same order, counts are integers and the 64-bit key (count << 32) | (0xffffffff - h) decides winner and tie together, so there is no tolerance.
The shapes come from the module's exported decomposition: B = HYP_BLOCK hypotheses per workgroup, T = POINT_TILE points per LDS tile, the default
split rule, and SPLIT_TILE records per workgroup of the ordered compaction.
moments: n is equal as an integer; the sums lie within (n + 2) 2^-53 sum |term| of math.fsum (_ground_ref.moments_ref).  fit: the refined plane lies
within a bound the test computes from the reference's own centred normal matrix (plane_bounds).
FALNET_GROUND_REPORT=<file> also writes the observed worst case there (profiles/ground_vs_ref.txt holds such figures).
The device path is never compared with itself, except where the property IS self-agreement (two runs, a permutation, the two plane sources)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ground_ref as GR  # noqa: E402
import _lidar_ref as LR  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import ground as G  # noqa: E402
from fal_net_amd import inference, pseudo_lidar, velodyne  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
B, T, S = G.HYP_BLOCK, G.POINT_TILE, G.SPLIT_TILE
HS = (1, B - 1, B, B + 1)
NS = (3, T - 1, T, T + 1, 2 * T + 3)
SPLITS = (1, 2, 3, 0)  # plain store, the atomic path (with an empty split where n <= T), the library's own choice
TOL = 0.15
GUARD = 64
GUARD_WORD = 0x5A5AA5A5
GARBAGE = 0x0123456789ABCDEF
WORST = {}  # tag -> (ratio of the bound reached, n): the figures of profiles/ground_vs_ref.txt


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def cloud(kind):
    """Seeded clouds of 2 T + 3 records, computed once and left unchanged: 'road' (the planted plane of the host tests), 'lattice' (integer
    coordinates in [0, 12)^3) and 'dirty' (the road with NaN and +-inf coordinates sprinkled in)."""
    n = 2 * T + 3
    if kind == "road":
        return GR.road_cloud(n)
    if kind == "lattice":
        return GR.lattice_cloud(n)
    pts = GR.road_cloud(n).copy()
    rng = np.random.default_rng(23)
    for val in (np.nan, np.inf, -np.inf):
        rows = rng.choice(n, 60, replace=False)
        pts[rows, rng.integers(0, 3, 60)] = val
    pts[:, 3] = np.nan  # the fourth value is ignored
    return pts


def tilt(kind):
    return 60.0 if kind == "lattice" else 15.0


@functools.lru_cache(maxsize=None)
def ref_planes(kind, n, H):
    return GR.hypotheses_ref(cloud(kind)[:n], G.triples(5, H, n), tilt(kind))


@functools.lru_cache(maxsize=None)
def ref_consensus(kind, n, H, tol=TOL):
    return GR.consensus_ref(cloud(kind)[:n], ref_planes(kind, n, H), tol)


def guarded(n, dtype, fill):
    """A buffer of n entries pre-filled with `fill` and GUARD entries behind it; -> (the whole buffer, its first n entries)."""
    words = {torch.int32: 1, torch.float32: 1, torch.int64: 2, torch.float64: 2}[dtype]
    buf = torch.full(((n + GUARD) * words,), GUARD_WORD, dtype=torch.int32, device=DEV).view(dtype)
    buf[:n] = fill
    return buf, buf[:n]


def guard_intact(buf, n):
    return bool((buf[n:].contiguous().view(torch.int32) == GUARD_WORD).all())


def run_hypotheses(pts, triples, max_tilt, tag):
    H = len(triples)
    buf, out = guarded(H * 4, torch.float32, float("nan"))
    got = G.hypotheses(dev(pts), triples, max_tilt, out=out.view(H, 4))
    assert got.data_ptr() == buf.data_ptr() and guard_intact(buf, H * 4), tag + ": written behind the planes"
    return got.cpu().numpy()


def run_consensus(pts, planes, tol, splits, tag):
    """consensus() into pre-filled outputs with guard zones behind them and a garbage-filled workspace with one too.  -> (counts, best words)."""
    n, H = len(pts), len(planes)
    cbuf, counts = guarded(H, torch.int32, -7)
    bbuf, best = guarded(G.BEST_WORDS, torch.int32, -7)
    need = int(L.lib().falnet_ground_consensus_workspace_bytes(n, H, splits)) // 8
    ws = torch.full((need + GUARD,), GARBAGE, dtype=torch.int64, device=DEV)  # unless the library zeroes its counters, the counts are wrong
    ws[need:] = GUARD_WORD
    got_c, got_b = G.consensus(dev(pts), dev(planes), tol, splits=splits, out=(counts, best), workspace=ws)
    assert got_c.data_ptr() == cbuf.data_ptr() and got_b.data_ptr() == bbuf.data_ptr()
    assert guard_intact(cbuf, H) and guard_intact(bbuf, G.BEST_WORDS), tag + ": written behind an output"
    assert bool((ws[need:] == GUARD_WORD).all()), tag + ": written behind the workspace"
    return counts.cpu().numpy().astype(np.int64), best.cpu().numpy().view(np.uint32)


def assert_consensus(got, want, tag):
    counts, best = got
    want_counts, want_best = want
    words = GR.best_words(want_best)
    bad = int((counts != want_counts).sum())
    print(f"{tag}: {len(counts)} hypotheses, {bad} counts differ; key {G.best_key(best.view(np.int32)):#x} (reference {want_best['key']:#x})")
    assert bad == 0 and G.best_key(best.view(np.int32)) == want_best["key"] and np.array_equal(best, words), tag


# ---- 1. hypotheses ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["road", "lattice", "dirty"])
def test_hypotheses_equal_the_reference_bit_for_bit(kind):
    for n in (2 * T + 3, T - 1):
        for H in HS:
            want = ref_planes(kind, n, H)
            got = run_hypotheses(cloud(kind)[:n], G.triples(5, H, n), tilt(kind), f"{kind} n={n} H={H}")
            bad = int((got.view(np.uint32) != want.view(np.uint32)).any(1).sum())
            print(f"{kind} n={n} H={H}: {bad} planes differ, {int((want[:, 3] == 0).sum())} invalid")
            assert got.dtype == np.float32 and bad == 0
    want = ref_planes(kind, 2 * T + 3, B + 1)
    invalid = want[:, 3] == 0
    assert (want[invalid].view(np.uint32) == 0).all() and (want[~invalid, 3] == 1).all()
    if kind == "lattice":  # collinear and repeated triples in abundance
        assert invalid.sum() > B // 8 and (~invalid).sum() > B // 8
    if kind == "road":
        assert (~invalid).mean() >= 0.5


def test_hypotheses_repeated_and_outside_indices_are_invalid():
    pts = cloud("road")[:100]
    tr = np.array([[0, 1, 2], [4, 4, 9], [7, 3, 7], [0, 1, 100], [-1, 2, 3], [5, 6, 2 ** 31 - 1], [10, 11, 12]], np.int32)
    got = run_hypotheses(pts, tr, 89.0, "indices")
    want = GR.hypotheses_ref(pts, tr[[0, 1, 2, 6]], 89.0)
    assert np.array_equal(got[[0, 1, 2, 6]].view(np.uint32), want.view(np.uint32)) and want[0, 3] == 1 and want[3, 3] == 1
    assert (got[[1, 2, 3, 4, 5]].view(np.uint32) == 0).all()  # four +0: a repeated index by its arithmetic, an index outside the scan without a read


# ---- 2. consensus -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_consensus_equals_the_reference(n, H):
    pts, planes, want = cloud("road")[:n], ref_planes("road", n, H), ref_consensus("road", n, H)
    for s in SPLITS:
        assert_consensus(run_consensus(pts, planes, TOL, s, f"n={n} H={H} splits={s}"), want, f"n={n} H={H} splits={s}")
    chosen = L.lib().falnet_ground_splits(n, H)
    assert chosen == G.default_splits(n, H) and (chosen > 1) == (n > T)  # the library's choice takes both paths over these shapes
    if n >= T and H >= B - 1:
        assert want[1]["status"] == 1 and want[1]["count"] > n // 4


def test_ties_go_to_the_smallest_index():
    n, H = 2 * T + 3, B + 1
    pts = cloud("road")
    tr = G.triples(5, H, n).copy()
    w0 = ref_consensus("road", n, H)[1]["index"]
    assert 0 <= w0 < B - 1
    tr[B - 1] = tr[B] = tr[w0]  # the winning triple twice more, across the HYP_BLOCK border
    planes = GR.hypotheses_ref(pts, tr)
    want = GR.consensus_ref(pts, planes, TOL)
    assert want[1]["index"] == w0 and want[0][w0] == want[0][B - 1] == want[0][B] == want[0].max()
    for s in SPLITS:
        assert_consensus(run_consensus(pts, planes, TOL, s, f"tie splits={s}"), want, f"tie splits={s}")
    tr[w0] = (0, 0, 0)  # the first of them made invalid: the tie is now decided across the border
    planes = GR.hypotheses_ref(pts, tr)
    want = GR.consensus_ref(pts, planes, TOL)
    assert want[1]["index"] == B - 1 and want[0][w0] == 0 and want[0][B] == want[0][B - 1]
    got_planes = run_hypotheses(pts, tr, 15.0, "tie planes")
    assert np.array_equal(got_planes.view(np.uint32), planes.view(np.uint32))
    for s in SPLITS:
        assert_consensus(run_consensus(pts, planes, TOL, s, f"border tie splits={s}"), want, f"border tie splits={s}")


def test_lattice_ties():
    n, H = 2 * T + 3, B + 1
    pts, planes = cloud("lattice"), ref_planes("lattice", n, H)
    for tol in (0.0, 0.5):
        want = GR.consensus_ref(pts, planes, tol)
        top = want[0].max()
        assert want[1]["index"] == int(np.flatnonzero(want[0] == top)[0]) and (tol > 0 or (want[0] == top).sum() > 1)  # tol 0: a tie to decide
        for s in SPLITS:
            assert_consensus(run_consensus(pts, planes, tol, s, f"lattice tol={tol} splits={s}"), want, f"lattice tol={tol} splits={s}")


def test_an_all_collinear_cloud_has_no_plane():
    pts = GR.line_cloud(T + 5)
    tr = G.triples(0, B + 1, len(pts))
    planes = run_hypotheses(pts, tr, 89.0, "line")
    assert (planes.view(np.uint32) == 0).all()
    want = GR.consensus_ref(pts, planes, TOL)
    assert want[1]["status"] == 0 and want[1]["index"] == -1 and want[1]["key"] == GR.key_of(0, 0)
    for s in SPLITS:
        assert_consensus(run_consensus(pts, planes, TOL, s, f"line splits={s}"), want, f"line splits={s}")
    assert G.fit(dev(pts), hypotheses=B + 1, max_tilt=89.0) is None and GR.fit_ref(pts, hypotheses=B + 1, max_tilt=89.0)[0] is None
    assert G.fit(dev(pts[:2])) is None  # fewer than three points: nothing launched
    # a valid hypothesis with fewer than 3 inliers is no plane either: two points of its triple moved away after the plane was formed
    pts = cloud("road")[:50].copy()
    planes = GR.hypotheses_ref(pts, np.array([[0, 1, 2]], np.int32), 89.0)
    far = pts.copy()
    far[:, 2] += np.where(np.arange(50) == 0, 0.0, 100.0).astype(np.float32)
    want = GR.consensus_ref(far, planes, 0.01)
    assert planes[0, 3] == 1 and want[0][0] == 1 and want[1]["status"] == 0 and want[1]["count"] == 1
    assert_consensus(run_consensus(far, planes, 0.01, 0, "one inlier"), want, "one inlier")


def test_non_finite_points_count_nowhere():
    n, H = 2 * T + 3, B + 1
    pts, planes = cloud("dirty"), ref_planes("road", n, H)  # the clean cloud's planes, the dirty cloud's points
    want = GR.consensus_ref(pts, planes, TOL)
    clean = ref_consensus("road", n, H)
    assert (want[0] <= clean[0]).all() and (want[0] < clean[0]).any() and want[1]["status"] == 1
    for s in SPLITS:
        assert_consensus(run_consensus(pts, planes, TOL, s, f"dirty splits={s}"), want, f"dirty splits={s}")
    allnan = np.full((T + 3, 4), np.nan, np.float32)
    nothing = GR.consensus_ref(allnan, planes, TOL)
    assert nothing[0].sum() == 0 and nothing[1]["status"] == 0
    for s in SPLITS:
        assert_consensus(run_consensus(allnan, planes, TOL, s, f"all-NaN splits={s}"), nothing, f"all-NaN splits={s}")


def test_a_permutation_of_the_points_and_a_second_call_change_nothing():
    n, H = 2 * T + 3, B + 1
    pts, planes, want = cloud("road"), ref_planes("road", n, H), ref_consensus("road", n, H)
    perm = np.random.default_rng(9).permutation(n)
    for s in (1, 3, 0):
        got = run_consensus(pts[perm], planes, TOL, s, f"permuted splits={s}")
        assert_consensus(got, want, f"permuted splits={s}")
        again = run_consensus(pts[perm], planes, TOL, s, f"permuted again splits={s}")
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


def test_argument_checks():
    pts, planes = dev(cloud("road")), dev(ref_planes("road", 2 * T + 3, B))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.consensus(pts.cpu(), planes, TOL)
    with pytest.raises(ValueError):
        G.consensus(pts[:2], planes, TOL)
    with pytest.raises(ValueError):
        G.consensus(pts, planes, TOL, splits=G.MAX_SPLITS + 1)
    with pytest.raises(ValueError):
        G.consensus(pts, planes.double(), TOL)
    with pytest.raises(ValueError):
        G.consensus(pts, planes, float("nan"))
    with pytest.raises(ValueError):
        G.moments(pts, TOL)
    with pytest.raises(ValueError):
        G.hypotheses(pts, np.zeros((G.MAX_HYPOTHESES + 1, 3), np.int32))
    lib = L.lib()
    assert lib.falnet_ground_splits(2, 5) == 0 and lib.falnet_ground_splits(1 << 31, 5) == 0 and lib.falnet_ground_splits(100, G.MAX_HYPOTHESES + 1) == 0
    assert lib.falnet_ground_consensus_workspace_bytes(5000, 513, 1) == 0 and lib.falnet_ground_consensus_workspace_bytes(5000, 513, 2) == 2056
    counts, best = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    assert lib.falnet_ground_consensus(L.ptr(pts), 2 * T + 3, L.ptr(planes), B, TOL, 2, L.ptr(counts), L.ptr(best), None, L.stream_ptr()) != 0
    assert b"workspace" in lib.falnet_last_error()
    assert lib.falnet_ground_consensus(pts.data_ptr() + 4, 100, L.ptr(planes), B, TOL, 1, L.ptr(counts), L.ptr(best), None, L.stream_ptr()) != 0
    assert b"16-byte aligned" in lib.falnet_last_error()
    assert lib.falnet_ground_heights(None, 0, 0.0, 0.0, 0.0, 1.0, None, L.stream_ptr()) == 0  # n == 0 launches nothing
    assert lib.falnet_ground_split(None, 0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1, None, 0, None, None, L.stream_ptr()) == 0


# ---- 3. moments -----------------------------------------------------------------------------------------------------------------------------------------
def check_row(got, want, bounds, tag):
    """n and the plane's columns equal; sums within the bound of math.fsum.  Prints each figure before it asserts."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    print(f"{tag}: n {got[GR.N]:.0f} (reference {want[GR.N]:.0f}), plane columns {got[GR.INDEX:].tolist()} (reference {want[GR.INDEX:].tolist()})")
    worst = 0.0
    for col, bound in bounds.items():
        err = abs(got[col] - want[col])
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"{tag}: column {col}: {got[col]!r} (reference {want[col]!r}), |difference| {err:.3e}, bound {bound:.3e}")
    WORST[tag] = (worst, int(want[GR.N]))
    assert got[GR.N] == want[GR.N] and np.array_equal(got[GR.INDEX:], want[GR.INDEX:]), tag
    for col, bound in bounds.items():
        assert abs(got[col] - want[col]) <= bound, (tag, col)


@functools.lru_cache(maxsize=None)
def big_cloud():
    """Longer than two passes of the moments' fixed grid (64 workgroups x 256 threads), with non-finite records: every thread strides."""
    pts = GR.road_cloud(2 * 64 * 256 + 77, seed=24).copy()
    rng = np.random.default_rng(25)
    pts[rng.choice(len(pts), 400, replace=False), rng.integers(0, 3, 400)] = np.nan
    pts[rng.choice(len(pts), 200, replace=False), 2] = np.inf
    return pts


@pytest.mark.parametrize("which", ["tiles", "grid"])
def test_moments_equal_the_reference(which):
    pts = cloud("dirty") if which == "tiles" else big_cloud()
    n, H = len(pts), B + 1
    planes = GR.hypotheses_ref(pts, G.triples(5, H, n))
    _, best = GR.consensus_ref(pts, planes, TOL)
    assert best["status"] == 1
    want, bounds = GR.moments_ref(pts, best["plane"], TOL, best["index"], best["count"])
    assert want[GR.N] == best["count"] > n // 4
    d_pts = dev(pts)
    _, d_best = G.consensus(d_pts, dev(planes), TOL)
    buf, row = guarded(G.ROW, torch.float64, float("nan"))
    from_device = G.moments(d_pts, TOL, best=d_best, out=row).cpu().numpy()  # the winner read from device memory
    assert guard_intact(buf, G.ROW)
    check_row(from_device, want, bounds, f"moments {which}")
    passed = G.moments(d_pts, TOL, plane=best["plane"], index=best["index"], count=best["count"]).cpu().numpy()  # the same plane, passed by the host
    assert passed.tobytes() == from_device.tobytes()
    assert G.moments(d_pts, TOL, best=d_best).cpu().numpy().tobytes() == from_device.tobytes()  # two calls give the same bits
    pl, ref = G.solve(from_device), G.solve(want)
    assert pl.inliers == ref.inliers and pl.hypothesis == best["index"] and pl.hypothesis_count == best["count"]


def test_moments_without_a_plane():
    pts = GR.line_cloud(T + 5)
    d_pts = dev(pts)
    _, best = G.consensus(d_pts, torch.zeros(4, 4, device=DEV), TOL)
    row = G.moments(d_pts, TOL, best=best).cpu().numpy()
    want, _ = GR.moments_ref(pts, (0, 0, 0), TOL, -1, 0, 0)
    assert row.tobytes() == want.tobytes() and row[GR.STATUS] == 0 and row[GR.INDEX] == -1 and G.solve(row) is None


# ---- 4. fit -----------------------------------------------------------------------------------------------------------------------------------------------
def plane_bounds(row, pts, tol):
    """How far the plane solved from the device's row may sit from the plane solved from the reference's `row`, from the reference alone.  Every sum
    S carries the bound e(S) of moments_ref.  A centred entry is c_ab = S_ab - S_a S_b / n, so to first order |delta c_ab| <= e(S_ab) + |mean b| e(S_a)
    + |mean a| e(S_b) =: e(c_ab).  For the 2 x 2 system A (p, q) = b: |delta (p, q)| / |(p, q)| <= cond(A) (|delta A| / |A| + |delta b| / |b|), with
    |delta A| <= 2 max e(c) and |delta b| <= sqrt 2 max e(c): the condition number times the relative sum bound, times 8 for the norm constants, the
    second-order terms and the host's own roundings in solve().  r = mean z - p mean x - q mean y adds its own first-order terms."""
    _, bounds = GR.moments_ref(pts, (row[GR.P], row[GR.Q], row[GR.R]), tol)
    n = row[GR.N]
    mx, my, mz = row[GR.SX] / n, row[GR.SY] / n, row[GR.SZ] / n
    e = lambda ab, a, b, ma, mb: bounds[ab] + abs(mb) * bounds[a] + abs(ma) * bounds[b]  # noqa: E731
    eA = max(e(GR.SXX, GR.SX, GR.SX, mx, mx), e(GR.SXY, GR.SX, GR.SY, mx, my), e(GR.SYY, GR.SY, GR.SY, my, my))
    eb = max(e(GR.SXZ, GR.SX, GR.SZ, mx, mz), e(GR.SYZ, GR.SY, GR.SZ, my, mz))
    cond, A = GR.centred_condition(row)
    b = np.array([row[GR.SXZ] - row[GR.SX] * mz, row[GR.SYZ] - row[GR.SY] * mz])
    pl = G.solve(row)
    rel = 8.0 * cond * max(eA / np.linalg.norm(A, 2), eb / np.linalg.norm(b))
    dpq = rel * float(np.hypot(pl.p, pl.q))
    dr = dpq * (abs(mx) + abs(my)) + 8.0 * (bounds[GR.SZ] + abs(pl.p) * bounds[GR.SX] + abs(pl.q) * bounds[GR.SY]) / n
    return dpq, dr, cond


@pytest.mark.parametrize("refits", [1, 2])
def test_fit_end_to_end(refits):
    n, H = 2 * T + 3, B + 1
    pts = cloud("road")
    want, rows = GR.fit_ref(pts, tol=TOL, hypotheses=H, seed=5, refits=refits)
    got = G.fit(dev(pts), tol=TOL, hypotheses=H, seed=5, refits=refits)
    assert got is not None and want is not None and len(rows) == refits
    dpq, dr, cond = plane_bounds(rows[-1], pts, TOL)
    print(f"fit refits={refits}: winner {got.hypothesis} with {got.hypothesis_count} (reference {want.hypothesis} with {want.hypothesis_count}), "
          f"{got.inliers} inliers (reference {want.inliers}); |dp| {abs(got.p - want.p):.3e} |dq| {abs(got.q - want.q):.3e} bound {dpq:.3e}; "
          f"|dr| {abs(got.r - want.r):.3e} bound {dr:.3e}; condition number {cond:.1f}; sensor height {got.sensor_height:.4f}")
    WORST[f"fit refits={refits}"] = (max(abs(got.p - want.p) / dpq, abs(got.q - want.q) / dpq, abs(got.r - want.r) / dr), want.inliers)
    assert got.hypothesis == want.hypothesis and got.hypothesis_count == want.hypothesis_count and got.inliers == want.inliers and got.n == want.n == n
    assert abs(got.p - want.p) <= dpq and abs(got.q - want.q) <= dpq and abs(got.r - want.r) <= dr
    assert 0 < dpq < 1e-9 and 0 < dr < 1e-9  # the bound is a rounding bound, not a modelling tolerance
    assert abs(got.sensor_height - 1.65) < 0.03 and got.normal[2] > 0.99 and abs(got.rms - want.rms) < 1e-9
    assert set(got._fields) >= {"p", "q", "r", "normal", "d", "sensor_height", "tilt_deg", "inliers", "n", "rms", "hypothesis", "hypothesis_count"}


# ---- 5. heights and split -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_plane():
    return GR.fit_ref(cloud("road"), hypotheses=B)[0]


def test_heights_bit_for_bit():
    pl = ref_plane()
    for kind in ("road", "dirty"):
        for n in (1, 255, 257, 2 * T + 3):
            pts = cloud(kind)[:n]
            buf, out = guarded(n, torch.float32, float("nan"))
            got = G.heights(dev(pts), pl, out=out)
            assert got.data_ptr() == buf.data_ptr() and guard_intact(buf, n)
            want = GR.heights_ref(pts, pl)
            got = got.cpu().numpy()
            # a NaN height (a non-finite coordinate) is a NaN on both sides; which NaN -- sign and payload of inf - inf -- IEEE leaves to the
            # machine, and the host's differs from the device's: every other height is compared on its bits
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), (kind, n)
    h = GR.heights_ref(cloud("dirty"), pl)
    assert np.isnan(h).sum() >= 50 and np.isinf(h).sum() >= 50  # the NaN coordinates; an infinite coordinate gives an infinite height
    assert G.heights(dev(cloud("road")[:0]), pl).shape == (0,)


@pytest.mark.parametrize("n", [1, S - 1, S, S + 1])
def test_split_byte_for_byte(n):
    pl = ref_plane()
    for kind in ("road", "dirty"):
        pts = cloud(kind)[:n]
        for lo, hi in ((-0.1, 0.25), (float("-inf"), 0.2), (0.2, float("inf"))):
            for inside in (True, False):
                want = GR.split_ref(pts, pl, lo, hi, inside)
                buf, out = guarded(n * 4, torch.float32, float("nan"))
                got = G.split(dev(pts), pl, lo, hi, inside=inside, out=out.view(n, 4))
                tag = f"{kind} n={n} ({lo}, {hi}] inside={inside}"
                assert guard_intact(buf, n * 4), tag
                assert got.shape == want.shape and got.cpu().numpy().tobytes() == want.tobytes(), tag  # the kept records, in point order
                assert len(want) == 0 or got.data_ptr() == buf.data_ptr()
                assert bool(torch.isnan(out.view(n, 4)[len(want):]).all()), tag + ": written behind the kept records"
        both = len(GR.split_ref(pts, pl, -0.1, 0.25)) + len(GR.split_ref(pts, pl, -0.1, 0.25, False))
        assert both == n


def test_split_capacity():
    pl, pts = ref_plane(), cloud("road")
    want = GR.split_ref(pts, pl, -0.1, 0.25)
    assert len(want) > 200
    cap = len(want) - 100
    buf, out = guarded(cap * 4, torch.float32, float("nan"))
    with pytest.raises(RuntimeError, match=f"{len(want)} points are kept but `out` holds {cap}"):
        G.split(dev(pts), pl, -0.1, 0.25, out=out.view(cap, 4))
    assert guard_intact(buf, cap * 4)
    assert out.view(cap, 4).cpu().numpy().tobytes() == want[:cap].tobytes()  # its first records are written
    exact = G.split(dev(pts), pl, -0.1, 0.25, out=torch.empty(len(want), 4, device=DEV))
    assert exact.cpu().numpy().tobytes() == want.tobytes()
    assert G.split(dev(pts[:0]), pl, 0, 1).shape == (0, 4)


# ---- 6. the writer and the product ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    """A planted-plane depth map: a dense road cloud through velodyne.project into a 96 x 320 nominal camera."""
    H, W = 96, 320
    P = velodyne.nominal_matrix(H, W, 160.0)
    depth = velodyne.project(dev(GR.road_cloud(60000, seed=26)), P, H, W).cpu().numpy()
    assert (depth > 0).mean() > 0.25
    return H, W, P, depth


def test_the_writer_and_the_product(tmp_path):
    H, W, P, depth = scene()
    kw = dict(tol=TOL, hypotheses=B + 1, seed=3, max_tilt=15.0, refits=2)
    dense = LR.unproject_ref(depth, P, fb=None, max_depth=80.0, max_height=np.inf)
    want, _ = GR.fit_ref(dense, **kw)
    assert want is not None and abs(want.sensor_height - 1.65) < 0.1 and len(dense) > 5000
    calibration = lambda i, h, w: (P, None)  # noqa: E731  (the map is a depth)
    d_depth = dev(depth).view(1, 1, H, W)
    frame = lambda i, m: inference.Frame(i, None, None, m, None, None)  # noqa: E731
    # the product: the plane's file equals the reference's, a frame without a plane writes none
    prod = G.GroundPlanes(str(tmp_path), calibration, extra={"calibration": "test"}, **kw)
    got = prod.frame(frame(4, d_depth))
    assert prod.frame(frame(5, torch.zeros_like(d_depth))) is None
    assert sorted(os.listdir(tmp_path / "Ground")) == ["0000000004.txt"]
    assert got.hypothesis == want.hypothesis and got.hypothesis_count == want.hypothesis_count and got.inliers == want.inliers
    want_cam = G.to_camera(want, P)
    written = G.read_plane(prod.file(4))
    print(f"written plane {written.tolist()}, reference {want_cam.tolist()}")
    assert np.allclose(written, want_cam, rtol=1e-6, atol=1e-12)  # %e keeps 7 digits: half a unit of the last is 5e-7 relative
    assert written[1] < -0.99 and abs(written[3] - want.sensor_height) < 1e-5
    summ = prod.summary()
    json.dumps(summ)
    assert (summ["frames"], summ["fitted"], summ["failed"]) == (2, 1, 1) and summ["sensor_height"] == got.sensor_height and summ["tilt_deg"] == got.tilt_deg
    assert summ["inlier_fraction"] == got.inliers / got.n and summ["rms"] == got.rms and summ["calibration"] == "test" and summ["hypotheses"] == B + 1
    # the writer: the filtered scan equals the numpy index of the unfiltered one
    plain = pseudo_lidar.PseudoLidarWriter(str(tmp_path / "plain"), calibration, max_height=1.0)
    filt = pseudo_lidar.PseudoLidarWriter(str(tmp_path / "filtered"), calibration, max_height=1.0, remove_ground=0.2, ground=kw)
    for w in (plain, filt):
        w.frame(frame(4, d_depth))
        w.frame(frame(5, torch.zeros_like(d_depth)))
    a, b = velodyne.load_scan(plain.file(4)), velodyne.load_scan(filt.file(4))
    keep = ~(GR.heights_ref(a, want) <= np.float32(0.2))
    assert 0 < keep.sum() < len(a) * 0.8 and b.tobytes() == a[keep].tobytes()
    assert os.path.getsize(filt.file(5)) == 0 and os.path.getsize(plain.file(5)) == 0
    assert "remove_ground" not in plain.summary() and plain.summary()["points"] == len(a)
    fs = filt.summary()
    assert fs["remove_ground"] == 0.2 and fs["ground_failed"] == 1 and fs["ground_removed"] == len(a) - len(b) and fs["points"] == len(b)
    with pytest.raises(ValueError):
        pseudo_lidar.PseudoLidarWriter(str(tmp_path / "bad"), calibration, remove_ground=0.2, ground={"tol": -1.0})


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------------------------------------
def _child(argv, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "Test_KITTI.py")] + argv, cwd=ROOT, env=dict(os.environ, FALNET_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_cli_end_to_end(tmp_path):
    argv = ["--synthetic", "--height", "96", "--width", "320", "--iters", "1", "--allow-seeded-weights", "--pseudo-lidar"]
    out = _child(argv + ["--ground", "--pl-remove-ground", "--save-path", str(tmp_path / "g")])
    lines = {next(iter(d)): d for d in (json.loads(ln) for ln in out.splitlines() if ln.startswith("{"))}
    assert list(lines) == ["pseudo_lidar", "ground", "image"] and "=> ground: no calibration files" in out, out
    g = lines["ground"]["ground"]
    assert g["frames"] == 1 and g["fitted"] + g["failed"] == 1 and g["calibration"] == "nominal" and g["tol"] == 0.15 and g["hypotheses"] == 512
    files = sorted(os.listdir(tmp_path / "g" / "Ground"))
    assert files == (["0000000000.txt"] if g["fitted"] else [])  # a file for every fitted frame and for no failed one
    if g["fitted"]:
        plane = G.read_plane(tmp_path / "g" / "Ground" / files[0])
        assert abs(np.linalg.norm(plane[:3]) - 1.0) < 1e-5 and plane[1] < 0 and g["sensor_height"] == pytest.approx(plane[3], rel=1e-5)
        assert 0 < g["inlier_fraction"] <= 1 and g["rms"] >= 0 and 0 <= g["tilt_deg"] <= 15.0 + 1e-6
    else:
        assert g["sensor_height"] is None
    pl = lines["pseudo_lidar"]["pseudo_lidar"]
    assert pl["remove_ground"] == 0.2 and pl["ground_failed"] == g["failed"] and pl["ground_removed"] >= 0
    # the same command without the two switches: no Ground folder, no line, and a scan that is no shorter
    out = _child(argv + ["--save-path", str(tmp_path / "plain")])
    plain = {next(iter(d)): d for d in (json.loads(ln) for ln in out.splitlines() if ln.startswith("{"))}
    assert list(plain) == ["pseudo_lidar", "image"] and not os.path.exists(tmp_path / "plain" / "Ground") and '{"ground"' not in out and "=> ground" not in out
    assert "remove_ground" not in plain["pseudo_lidar"]["pseudo_lidar"]
    a = velodyne.load_scan(tmp_path / "plain" / "Pseudo_lidar" / "0000000000.bin")
    b = velodyne.load_scan(tmp_path / "g" / "Pseudo_lidar" / "0000000000.bin")
    assert len(b) <= len(a) and len(a) - len(b) == pl["ground_removed"] and plain["image"]["image"] == [96, 320]


# ---- the figures ------------------------------------------------------------------------------------------------------------------------------------------------
def test_zz_report_the_worst_case():
    """Prints the largest fraction of its bound that any sum or plane reached in this session; FALNET_GROUND_REPORT=<file> also writes the figures."""
    lines = ["# falnet_ground_moments against math.fsum, and ground.fit against the reference's plane: the largest |difference| / bound per case",
             "# (bounds: tests/_ground_ref.py: moments_ref; tests/test_gpu_ground.py: plane_bounds)", "# case | inliers | worst fraction of the bound"]
    lines += [f"{tag} | {n} | {ratio:.4f}" for tag, (ratio, n) in sorted(WORST.items())]
    print("\n".join(lines))
    path = os.environ.get("FALNET_GROUND_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert all(ratio <= 1.0 for ratio, _ in WORST.values())
