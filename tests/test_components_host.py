"""CPU: the numpy definition of the connected components (tests/_components_ref.py) holds its own invariants on every input family and agrees with
scipy.ndimage.label where the edges depend on validity alone; the command line of Test_KITTI.py --min-component; the entry points in header, binding
and build; and, where the library is built, every refused argument of falnet_components on pointers that are never dereferenced."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import _components_ref as R  # noqa: E402
import Test_KITTI as T  # noqa: E402

SIZES = [(1, 1), (1, 7), (2, 2), (3, 5), (17, 65), (37, 124), (75, 250)]
LIB = os.path.join(ROOT, "fal_net_amd", "libfalnet_hip.so")


# ---- the reference's own invariants -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", R.FAMILIES)
def test_reference_invariants(name, H, W):
    f = R.family(name, H, W)
    labels, sizes, (n_comp, n_valid, largest) = R.reference(name, H, W)
    valid, right, down = R.edges(f["map"], **f["kw"])
    flat, g = labels.reshape(-1), np.arange(H * W)
    assert labels.dtype == np.int32 and sizes.dtype == np.int32 and labels.shape == sizes.shape == (H, W)
    assert np.array_equal(flat >= 0, valid.reshape(-1)) and np.array_equal(flat[flat < 0], np.full(int((~valid).sum()), -1))
    assert np.all(flat[valid.reshape(-1)] <= g[valid.reshape(-1)])  # the smallest index of the component
    assert np.array_equal(flat[flat[flat >= 0]], flat[flat >= 0])  # labels are fixed points
    assert n_valid == int(valid.sum()) and n_comp == int((flat == g).sum()) == len(np.unique(flat[flat >= 0]))
    roots = flat == g
    assert int(sizes.reshape(-1)[roots].sum()) == n_valid  # the sizes of the components sum to the valid count
    per_label = np.bincount(flat[flat >= 0], minlength=H * W)
    assert np.array_equal(sizes.reshape(-1), np.where(flat >= 0, per_label[np.maximum(flat, 0)], 0))
    assert largest == (int(sizes.max()) if n_valid else 0) and np.all(sizes[~valid] == 0) and np.all(sizes[valid] >= 1)
    # joined neighbours share a label
    assert np.array_equal(labels[:, :-1][right], labels[:, 1:][right]) and np.array_equal(labels[:-1][down], labels[1:][down])
    # and neighbours that share a label without an edge are joined some other way: the partition is no finer than the edges allow -- every component
    # is connected through edges, i.e. a breadth-first search from its root over the edges reaches size pixels
    if n_comp:
        root = int(np.flatnonzero(roots)[np.argmax(sizes.reshape(-1)[roots])])
        seen, todo = {root}, [root]
        while todo:
            p = todo.pop()
            i, j = divmod(p, W)
            for ok, q in ((j + 1 < W and right[i, j], p + 1), (j > 0 and right[i, j - 1], p - 1), (i + 1 < H and down[i, j], p + W), (i > 0 and down[i - 1, j], p - W)):
                if ok and q not in seen:
                    seen.add(q)
                    todo.append(q)
        assert len(seen) == largest and min(seen) == root and all(flat[q] == root for q in seen)


@pytest.mark.parametrize("H,W", SIZES + [(130, 260)], ids=lambda v: str(v))
def test_closed_form_counts(H, W):
    n = H * W
    assert R.reference("plane", H, W)[2] == (1, n, n)
    assert R.reference("checker", H, W)[2] == (n, n, 1)
    assert R.reference("rows", H, W)[2] == (H, n, W) and R.reference("columns", H, W)[2] == (W, n, H)
    path = R.spiral_path(H, W)
    assert R.reference("spiral", H, W)[2] == (1, int(path.sum()), int(path.sum())) and path[0, 0]
    if min(H, W) >= 5:  # the path fills about half of the frame and winds: it comes back to every other row
        assert 0.4 * n < path.sum() < 0.6 * n and path[2, 2:-2].all() and not path[1, 1:-1].any()
    labels = R.reference("spiral", H, W)[0]
    assert np.all(labels[path] == 0) and np.all(labels[~path] == -1)
    for name in ("serpentine", "comb"):
        comps, valid, largest = R.reference(name, H, W)[2]
        assert comps == 1 and valid == largest == int(np.isfinite(R.family(name, H, W)["map"]).sum())


@pytest.mark.parametrize("H,W", SIZES + [(130, 260)], ids=lambda v: str(v))
def test_two_spirals_do_not_merge(H, W):
    path = R.spiral_path(H, W)
    labels, sizes, (comps, valid, largest) = R.reference("two-spirals", H, W)
    assert valid == H * W and np.all(labels[path] == 0) and np.all(sizes[path] == path.sum())
    if (~path).any():
        assert np.all(labels[~path] > 0) and comps >= 2 and not np.intersect1d(labels[path], labels[~path]).size


def test_tie_joins_and_the_next_float_does_not():
    H, W = 17, 65
    f = R.family("tie", H, W)
    m, labels = f["map"], R.reference("tie", H, W)[0]
    three = m == np.float32(3.0)
    above = m > np.float32(3.0)
    assert f["kw"] == {"max_jump": 0.5} and three.any() and above.any() and np.all(m[above] == np.nextafter(np.float32(3.0), np.float32(np.inf)))
    assert np.all(R.reference("tie", H, W)[1][above] == 1)  # alone: each of its neighbours is a 2
    assert np.all(labels[three] < np.arange(H * W).reshape(H, W)[three])  # joined to the 2 left of it or above it
    assert R.label_ref(np.array([[2.0, 3.0]], np.float32), max_jump=0.5)[2] == (1, 2, 2)
    assert R.label_ref(np.array([[2.0, np.nextafter(np.float32(3.0), np.float32(4.0))]], np.float32), max_jump=0.5)[2] == (2, 2, 1)


def test_validity_rules():
    nan, inf = np.nan, np.inf
    m = np.array([[nan, inf, -inf, 0.0, -0.0, -3.0, 1.0, 2.0, 8.0, 8.5]], np.float32)
    labels, sizes, info = R.label_ref(m, max_jump=inf, lo=1.0, hi=8.0)
    assert labels.tolist() == [[-1, -1, -1, -1, -1, -1, -1, 7, 7, -1]] and sizes.tolist() == [[0] * 7 + [2, 2, 0]] and info == (1, 2, 2)
    assert R.label_ref(m, max_jump=inf)[0].tolist() == [[-1, 1, -1, -1, -1, -1, 6, 6, 6, 6]]  # hi = inf keeps +inf; lo = 0 drops both zeros
    score = np.array([[1, 1, 1, 1, 1, 1, nan, 0.5, 0.49, 1]], np.float32)
    assert R.label_ref(m, max_jump=inf, score=score, threshold=0.5)[0].tolist() == [[-1, 1, -1, -1, -1, -1, -1, 7, -1, 9]]
    bad = R.family("bad", 37, 124)
    v = R.edges(bad["map"], **bad["kw"])[0]
    assert 0 < v.sum() < v.size and not np.isfinite(bad["map"]).all() and (bad["map"][~v & np.isfinite(bad["map"])] > 8).any()
    for name in R.FAMILIES:  # no subnormal and nothing beyond 2^20 among the finite positive values
        x = R.family(name, 75, 250)["map"]
        pos = x[np.isfinite(x) & (x > 0)]
        assert pos.min() >= R.LO_V and pos.max() <= R.HI_V, name


@pytest.mark.parametrize("H,W", [(3, 5), (17, 65), (37, 124), (75, 250)], ids=lambda v: str(v))
@pytest.mark.parametrize("name", R.VALIDITY_ONLY)
def test_same_partition_as_scipy(name, H, W):
    ndimage = pytest.importorskip("scipy.ndimage")
    f = R.family(name, H, W)
    valid, right, down = R.edges(f["map"], **f["kw"])
    assert np.array_equal(right, valid[:, :-1] & valid[:, 1:]) and np.array_equal(down, valid[:-1] & valid[1:])  # validity alone
    theirs, n = ndimage.label(valid)  # 4-connectivity by default
    labels, sizes, (comps, _, _) = R.reference(name, H, W)
    assert n == comps
    first = np.full(n + 1, H * W, np.int64)
    np.minimum.at(first, theirs.reshape(-1), np.arange(H * W))
    assert np.array_equal(np.where(valid, first[theirs], -1), labels)
    assert np.array_equal(np.where(valid, np.bincount(theirs.reshape(-1), minlength=n + 1)[theirs], 0), sizes)


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------------
def test_cli_switches_and_refusals():
    parse = T.parser.parse_args
    a = parse(["--mesh", "--min-component", "50", "--component-jump", "0.1"])
    assert (a.min_component, a.component_jump) == (50, 0.1)
    T.check_family_args(a)
    T.check_component_args(a)
    T.check_component_args(parse(["--pseudo-lidar", "--min-component", "1"]))
    T.check_component_args(parse([]))
    assert parse([]).min_component is None and parse([]).component_jump is None and parse(["--min-component", str(1 << 24)]).min_component == 1 << 24
    assert parse(["--mesh", "--min-component", "5", "--component-jump", "inf"]).component_jump == float("inf")
    with pytest.raises(SystemExit, match="--mesh.*--pseudo-lidar"):
        T.check_component_args(parse(["--min-component", "50"]))
    with pytest.raises(SystemExit, match="--mesh.*--pseudo-lidar"):
        T.check_component_args(parse(["--min-component", "50", "--dump", "pc"]))
    with pytest.raises(SystemExit) as e:
        T.check_family_args(parse(["--mesh", "--component-jump", "0.1"]))
    assert str(e.value) == "--component-jump sets a parameter of --min-component: add --min-component"
    for bad in (["--min-component", "0"], ["--min-component", "-3"], ["--min-component", str((1 << 24) + 1)], ["--min-component", "2.5"],
                ["--min-component", "nan"], ["--component-jump", "-0.1"], ["--component-jump", "nan"]):
        with pytest.raises(SystemExit):
            parse(["--mesh"] + bad)
    assert T.LINE_ORDER[-1] == "components" and T.LINE_ORDER[:-1] == ("view", "sparsification", "pseudo_lidar", "mesh", "sweep", "freeview", "stats")


def test_family_tables_and_settings():
    parse = T.parser.parse_args
    assert T.COMPONENT_ARGS == ("min_component", "component_jump")
    assert [f[0] for f in T.FAMILIES] == ["--sweep", "--stats", "--pseudo-lidar", "--mesh", "--sparsification", "--freeview", "--freeview-fill"]  # untouched
    assert [(f[0], f[1], f[3]) for f in T.LATER_FAMILIES] == [("--min-component", T.COMPONENT_ARGS, True)]
    assert all(len(f) == 4 and callable(f[2]) for f in T.LATER_FAMILIES)
    off, on = parse(["--mesh"]), parse(["--mesh", "--min-component", "9"])
    # hidden_settings is what it was: it does not know the new names, with or without the switch
    assert not set(T.COMPONENT_ARGS) & set(T.hidden_settings(off)) and T.hidden_settings(off) == T.hidden_settings(on)
    assert T.settings_hidden(off) == T.hidden_settings(off) + T.COMPONENT_ARGS and T.settings_hidden(on) == T.hidden_settings(on)
    # settings.txt: the names of a run without the switch are the names it had before the switch existed
    names = lambda a: [k for k in vars(a) if k not in T.settings_hidden(a)]  # noqa: E731
    assert not set(T.COMPONENT_ARGS) & set(names(off)) and set(names(on)) - set(names(off)) == set(T.COMPONENT_ARGS)
    assert set(T.COMPONENT_ARGS) <= set(vars(off))


def test_python_checks_without_a_device():
    import torch
    from fal_net_amd import components, mesh, pseudo_lidar
    assert components.check_min_component(None) is None and components.check_min_component(1) == 1 and components.check_min_component(1 << 24) == 1 << 24
    assert components.check_min_component(7.0) == 7
    for bad in (0, -1, (1 << 24) + 1, 2.5, float("nan"), float("inf"), True):
        with pytest.raises(ValueError):
            components.check_min_component(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        components.label(torch.zeros(3, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        components.size_score(np.zeros((3, 5), np.float32))
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            components.check_jump(bad)
        with pytest.raises(ValueError):
            components.ComponentsSummary(5, bad)
    s = components.ComponentsSummary(5, 0.1).summary()
    assert s["frames"] == 0 and s["min_component"] == 5 and s["max_jump"] == 0.1 and s["largest"] == 0 and s["mean_components"] != s["mean_components"]
    assert components.ComponentsSummary.key == "components"


def test_writers_take_the_keywords(tmp_path):
    from fal_net_amd import mesh, pseudo_lidar
    w = mesh.MeshWriter(str(tmp_path), max_jump=0.2, min_component=40)
    assert w.min_component == 40 and w.component_jump == 0.2 and w.summary()["min_component"] == 40
    assert mesh.MeshWriter(str(tmp_path), max_jump=0.2, min_component=40, component_jump=0.07).component_jump == 0.07
    plain = mesh.MeshWriter(str(tmp_path))
    assert plain.min_component is None and "min_component" not in plain.summary()
    p = pseudo_lidar.PseudoLidarWriter(str(tmp_path), min_component=12)
    assert p.min_component == 12 and p.component_jump == 0.05 and p.summary()["min_component"] == 12
    assert "min_component" not in pseudo_lidar.PseudoLidarWriter(str(tmp_path)).summary()
    for cls in (mesh.MeshWriter, pseudo_lidar.PseudoLidarWriter):
        with pytest.raises(ValueError):
            cls(str(tmp_path), min_component=0)
        with pytest.raises(ValueError):
            cls(str(tmp_path), min_component=5, component_jump=-1.0)


# ---- the entry points -------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_in_header_binding_and_build():
    from fal_net_amd import _build, _lib, ops
    raw = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bfalnet_components\s*\(", hdr) and re.search(r"\bfalnet_components_workspace_bytes\s*\(", hdr)
    for word in ("smallest pixel index", "max(v_p, v_q) <= min(v_p, v_q) * ratio", "A tie joins", "3 B + 1", "status word"):
        assert word in raw, word  # the definition stands beside the prototype
    P, F, I = _lib._P, _lib._F, _lib._I
    assert _lib.SIGNATURES["falnet_components"] == [P, P, F, F, F, F, I, I, I, P, P, P, P, P]
    assert _lib.SIGNATURES["falnet_components_workspace_bytes"] == [I, I, I] and _lib._RESTYPES["falnet_components_workspace_bytes"] is _lib.C.c_int64
    assert "components.hip" in _build.SOURCES and "components.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600
    src = open(os.path.join(_build.CSRC, "components.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"atomic\w*\s*\([^;]*float", code) and "cooperative" not in code and "__HIP_MEMORY_SCOPE_AGENT" in code


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_workspace_bytes_and_refusals_without_a_device():
    """The size function and every argument check run before anything touches the device."""
    from fal_net_amd import _lib as L
    lib = L.lib()
    r8 = lambda v: (v + 7) // 8 * 8  # noqa: E731
    for B, H, W in ((1, 375, 1242), (8, 256, 512), (3, 1, 1), (1, 1, 7)):
        assert lib.falnet_components_workspace_bytes(B, H, W) == 3 * r8(4 * B * H * W) + r8(B * H * W), (B, H, W)
    assert lib.falnet_components_workspace_bytes(1, (1 << 15) - 1, 1 << 15) > 0 and lib.falnet_components_workspace_bytes(1, 1, (1 << 30) - 1) > 0
    for bad in ((0, 5, 7), (1, 0, 7), (1, 5, -1), (-2, 5, 7), (1, 1 << 15, 1 << 15), (2, 1 << 15, 1 << 15), (4, 1 << 14, 1 << 15), (1 << 30, 1, 2)):
        assert lib.falnet_components_workspace_bytes(*bad) == 0, bad
    fake = L.C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
    odd = lambda k: L.C.c_void_p((1 << 20) + k)  # noqa: E731
    base = dict(map=fake, score=None, threshold=0.0, lo=0.0, hi=float("inf"), ratio=1.05, B=2, H=5, W=7, label=fake, size=fake, info=fake, ws=fake)
    nan, inf = float("nan"), float("inf")
    cases = [("null map", dict(map=None), "null map"), ("null size", dict(size=None), "null map or size"), ("null info", dict(info=None), "null info"),
             ("null workspace", dict(ws=None), "null info or workspace"), ("B = 0", dict(B=0), "B >= 1"), ("B < 0", dict(B=-1), "B >= 1"),
             ("H = 0", dict(H=0), "H W"), ("W < 0", dict(W=-7), "H W"), ("H W = 2^30", dict(B=1, H=1 << 15, W=1 << 15), "2\\^30"),
             ("B H W = 2^31", dict(B=4, H=1 << 14, W=1 << 15), "2\\^31"), ("lo < 0", dict(lo=-1.0), "lo"), ("lo = hi", dict(lo=3.0, hi=3.0), "lo < hi"),
             ("lo > hi", dict(lo=5.0, hi=3.0), "lo < hi"), ("lo NaN", dict(lo=nan), "lo"), ("hi NaN", dict(hi=nan), "hi"), ("lo inf", dict(lo=inf), "lo < hi"),
             ("ratio < 1", dict(ratio=0.99), "ratio"), ("ratio NaN", dict(ratio=nan), "ratio"), ("ratio < 0", dict(ratio=-inf), "ratio"),
             ("misaligned workspace", dict(ws=odd(4)), "8-byte"), ("misaligned info", dict(info=odd(4)), "8-byte"),
             ("misaligned map", dict(map=odd(2)), "4-byte"), ("misaligned size", dict(size=odd(1)), "4-byte"), ("misaligned label", dict(label=odd(3)), "4-byte"),
             ("misaligned score", dict(score=odd(2)), "4-byte")]
    for tag, change, word in cases:
        k = dict(base, **change)
        rc = lib.falnet_components(k["map"], k["score"], k["threshold"], k["lo"], k["hi"], k["ratio"], k["B"], k["H"], k["W"], k["label"], k["size"], k["info"],
                                   k["ws"], None)
        assert rc != 0, tag
        assert re.search(word, lib.falnet_last_error().decode()), (tag, lib.falnet_last_error().decode())
