"""GPU: the connected components of a depth or disparity map (fal_net_amd/components.py: label, csrc/components.hip) against their definition on the
host (tests/_components_ref.py: label_ref, whose own invariants tests/test_components_host.py holds).  The result is an integer partition: every
comparison is torch.equal / ==, there is no tolerance anywhere.  The device path is never compared with itself, except where the property IS
self-agreement (two calls, a batch against single calls, labels wanted or not)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _components_ref as R  # noqa: E402
import _mesh_ref as MR  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import components, dumps, mesh, pseudo_lidar  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# 1 x 1, 1 x 7, 2 x 2, 3 x 5: inside one 16 x 64 tile, H = 1 and a partial wave; 17 x 65: one pixel past the tile both ways, four tiles and both kinds of
# border; 37 x 124 and 75 x 250: 3 x 2 and 5 x 4 tiles with partial last ones; 130 x 260: 9 x 5 tiles, for the families whose one component crosses
# every tile many times
SIZES = [(1, 1), (1, 7), (2, 2), (3, 5), (17, 65), (37, 124), (75, 250)]
LONG = [("spiral", 130, 260), ("serpentine", 130, 260), ("comb", 130, 260)]
GUARD = 1024          # int32 words behind each output
FILL = 0x5A5A5A5A     # garbage the outputs start from: no label, no size
INFO_FILL = -7


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the families' arrays are read-only


def raw_label(maps, kw, want_labels=True, bufs=None):
    """falnet_components on the stacked (B, H, W) maps into garbage-filled outputs with a guard zone behind them -> (rc, label, size, info) tensors, the
    outputs with their guards."""
    B, H, W = maps.shape
    lib = L.lib()
    n = B * H * W
    if bufs is None:
        label = torch.full((n + GUARD,), FILL, dtype=torch.int32, device=DEV)
        size = torch.full((n + GUARD,), FILL, dtype=torch.int32, device=DEV)
        info = torch.full((3 * B + 1 + 4,), INFO_FILL, dtype=torch.int64, device=DEV)
        ws = torch.full((int(lib.falnet_components_workspace_bytes(B, H, W)) // 8 + 1,), INFO_FILL, dtype=torch.int64, device=DEV)
    else:
        label, size, info, ws = bufs
    d_maps, d_score = dev(maps), dev(kw.get("score"))  # both alive until the launches have run
    rc = lib.falnet_components(L.ptr(d_maps), L.ptr(d_score), float(kw.get("threshold", 0.0) or 0.0), float(kw.get("lo", 0.0)),
                               float(kw.get("hi", float("inf"))), 1.0 + float(kw.get("max_jump", 0.05)), B, H, W, L.ptr(label) if want_labels else None,
                               L.ptr(size), L.ptr(info), L.ptr(ws), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, label, size, info, ws


def check_against(refs, label, size, info, tag, want_labels=True):
    """refs: the reference results of the B images, in order."""
    B, (H, W) = len(refs), refs[0][0].shape
    n = B * H * W
    words = info.cpu().tolist()
    print(tag, "info", words[:3 * B + 1], "reference", [r[2] for r in refs])
    assert words[3 * B] == 0, tag + ": status"
    assert words[3 * B + 1:] == [INFO_FILL] * 4, tag + ": written behind info"
    assert [tuple(words[3 * b:3 * b + 3]) for b in range(B)] == [r[2] for r in refs], tag + ": info"
    assert torch.equal(size[:n].cpu().view(B, H, W), torch.from_numpy(np.stack([r[1] for r in refs]))), tag + ": sizes"
    if want_labels:
        assert torch.equal(label[:n].cpu().view(B, H, W), torch.from_numpy(np.stack([r[0] for r in refs]))), tag + ": labels"
    else:
        assert bool((label == FILL).all()), tag + ": labels written though not wanted"
    assert bool((label[n:] == FILL).all()) and bool((size[n:] == FILL).all()), tag + ": written into the guard zone"


# ---- equal to the reference ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", R.FAMILIES)
def test_equals_reference(name, H, W):
    f = R.family(name, H, W)
    rc, label, size, info, _ = raw_label(f["map"][None], f["kw"])
    assert rc == 0
    check_against([R.reference(name, H, W)], label, size, info, f"{name} {H}x{W}")


@pytest.mark.parametrize("name,H,W", LONG)
def test_one_component_through_every_tile(name, H, W):
    f = R.family(name, H, W)
    want = R.reference(name, H, W)
    assert want[2][0] == 1 and want[2][1] > H * W // 3  # one component of about half the frame
    rc, label, size, info, _ = raw_label(f["map"][None], f["kw"])
    assert rc == 0
    check_against([want], label, size, info, f"{name} {H}x{W}")


def test_a_batch_of_three_families_against_single_calls():
    H, W = 37, 124
    names = ("walk", "percolation", "checker")  # the same keywords: one call takes them together
    maps = np.stack([R.family(n, H, W)["map"] for n in names])
    assert all(R.family(n, H, W)["kw"] == {} for n in names)
    rc, label, size, info, _ = raw_label(maps, {})
    assert rc == 0
    check_against([R.reference(n, H, W) for n in names], label, size, info, "batch of 3")
    n = H * W
    for b, name in enumerate(names):
        rc1, l1, s1, i1, _ = raw_label(maps[b:b + 1], {})
        assert rc1 == 0 and torch.equal(l1[:n], label[b * n:(b + 1) * n]) and torch.equal(s1[:n], size[b * n:(b + 1) * n]), name
        assert torch.equal(i1[:3], info[3 * b:3 * b + 3]) and int(i1[3]) == 0, name
        assert int(label[b * n:(b + 1) * n].max()) < n  # indices are per image


def test_score_and_bounds_in_a_batch():
    H, W = 17, 65
    a, b = R.family("score", H, W), R.family("bad", H, W)
    kw = dict(a["kw"], **b["kw"])
    maps, score = np.stack([a["map"], b["map"]]), np.stack([a["kw"]["score"], np.flipud(a["kw"]["score"])])
    refs = [R.label_ref(maps[k], lo=kw["lo"], hi=kw["hi"], score=score[k], threshold=kw["threshold"]) for k in range(2)]
    rc, label, size, info, _ = raw_label(maps, dict(kw, score=score))
    assert rc == 0 and refs[0][2][1] > 0 and refs[1][2][1] > 0
    check_against(refs, label, size, info, "score and bounds, batch of 2")


def test_without_labels_the_sizes_are_the_same():
    for name, H, W in (("walk", 75, 250), ("spiral", 37, 124), ("bad", 17, 65)):
        f = R.family(name, H, W)
        rc, label, size, info, _ = raw_label(f["map"][None], f["kw"], want_labels=False)
        assert rc == 0
        check_against([R.reference(name, H, W)], label, size, info, f"{name} {H}x{W} without labels", want_labels=False)


def test_two_calls_give_equal_bits_in_either_mode():
    H, W = 75, 250
    lib = L.lib()
    for name in ("walk", "percolation", "spiral"):
        f = R.family(name, H, W)
        runs = []
        try:
            for mode in (1, 0, 1, 0):
                lib.falnet_set_deterministic(mode)
                rc, label, size, info, _ = raw_label(f["map"][None], f["kw"])
                assert rc == 0
                runs.append((label, size, info))
        finally:
            lib.falnet_set_deterministic(1 if L.DETERMINISTIC else 0)
        for label, size, info in runs[1:]:
            assert torch.equal(label, runs[0][0]) and torch.equal(size, runs[0][1]) and torch.equal(info, runs[0][2]), name
        assert runs[0][0].data_ptr() != runs[1][0].data_ptr()
        check_against([R.reference(name, H, W)], *runs[0], f"{name} first of four calls")


def test_every_refused_argument_returns_nonzero_and_writes_nothing():
    H, W = 17, 65
    f = R.family("walk", H, W)
    lib = L.lib()
    n = H * W
    label = torch.full((n + GUARD,), FILL, dtype=torch.int32, device=DEV)
    size = torch.full((n + GUARD,), FILL, dtype=torch.int32, device=DEV)
    info = torch.full((8,), INFO_FILL, dtype=torch.int64, device=DEV)
    ws = torch.full((int(lib.falnet_components_workspace_bytes(1, H, W)) // 8 + 1,), INFO_FILL, dtype=torch.int64, device=DEV)
    m = dev(f["map"])
    nan, inf = float("nan"), float("inf")
    odd = lambda t, k: L.C.c_void_p(t.data_ptr() + k)  # noqa: E731
    base = dict(map=L.ptr(m), score=None, threshold=0.0, lo=0.0, hi=inf, ratio=1.05, B=1, H=H, W=W, label=L.ptr(label), size=L.ptr(size), info=L.ptr(info), ws=L.ptr(ws))
    cases = [("null map", dict(map=None), "null map"), ("null size", dict(size=None), "null map or size"), ("null info", dict(info=None), "null info"),
             ("null workspace", dict(ws=None), "null info or workspace"), ("B = 0", dict(B=0), "B >= 1"), ("H = 0", dict(H=0), "H W"), ("W < 0", dict(W=-3), "H W"),
             ("H W = 2^30", dict(H=1 << 15, W=1 << 15), "2\\^30"), ("B H W = 2^31", dict(B=4, H=1 << 14, W=1 << 15), "2\\^31"), ("lo < 0", dict(lo=-0.5), "lo"),
             ("lo >= hi", dict(lo=2.0, hi=2.0), "lo < hi"), ("lo NaN", dict(lo=nan), "lo"), ("hi NaN", dict(hi=nan), "hi"), ("ratio < 1", dict(ratio=0.5), "ratio"),
             ("ratio NaN", dict(ratio=nan), "ratio"), ("misaligned workspace", dict(ws=odd(ws, 4)), "8-byte"), ("misaligned info", dict(info=odd(info, 4)), "8-byte"),
             ("misaligned size", dict(size=odd(size, 2)), "4-byte"), ("misaligned label", dict(label=odd(label, 1)), "4-byte"), ("misaligned map", dict(map=odd(m, 2)), "4-byte")]
    for tag, change, word in cases:
        k = dict(base, **change)
        rc = lib.falnet_components(k["map"], k["score"], k["threshold"], k["lo"], k["hi"], k["ratio"], k["B"], k["H"], k["W"], k["label"], k["size"], k["info"],
                                   k["ws"], L.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0, tag
        with pytest.raises(RuntimeError, match=word):
            L.check(rc, "components")
        assert bool((label == FILL).all()) and bool((size == FILL).all()) and bool((info == INFO_FILL).all()) and bool((ws == INFO_FILL).all()), tag  # nothing ran
    rc, label, size, info4, ws = raw_label(f["map"][None], f["kw"], bufs=(label, size, info, ws))  # and the next valid call is correct
    assert rc == 0 and int(ws[-1]) == INFO_FILL and info.tolist()[4:] == [INFO_FILL] * 4
    want = R.reference("walk", H, W)
    assert torch.equal(label[:n].cpu().view(H, W), torch.from_numpy(want[0])) and tuple(info.tolist()[:4]) == want[2] + (0,)
    assert raw_label(f["map"][None], dict(f["kw"], max_jump=inf, hi=inf))[0] == 0  # ratio = infinity and hi = infinity are legal


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_shapes_reads_and_errors():
    H, W = 37, 124
    names = ("walk", "percolation", "checker")
    maps = torch.stack([dev(R.family(n, H, W)["map"]) for n in names])
    for shape in ((3, H, W), (3, 1, H, W)):
        labels, sizes, info = components.label(maps.view(shape))
        assert labels.shape == shape and sizes.shape == shape and labels.dtype == sizes.dtype == torch.int32 and labels.is_cuda
        assert info == [R.reference(n, H, W)[2] for n in names]
        for b, n in enumerate(names):
            assert torch.equal(labels[b].view(H, W).cpu(), torch.from_numpy(R.reference(n, H, W)[0]))
            assert torch.equal(sizes[b].view(H, W).cpu(), torch.from_numpy(R.reference(n, H, W)[1]))
    labels, sizes, info = components.label(maps[0], want_labels=False)
    assert labels is None and sizes.shape == (H, W) and info == [R.reference("walk", H, W)[2]]
    f = R.family("score", H, W)
    sc = components.size_score(dev(f["map"]), score=dev(f["kw"]["score"]), threshold=f["kw"]["threshold"])
    assert sc.dtype == torch.float32 and torch.equal(sc.cpu(), torch.from_numpy(R.reference("score", H, W)[1].astype(np.float32)))
    f = R.family("tie", H, W)
    assert components.label(dev(f["map"]), **f["kw"])[2] == [R.reference("tie", H, W)[2]]  # 1.0 + max_jump rounded once: the tie joins
    with pytest.raises(ValueError):
        components.label(maps, score=maps)
    with pytest.raises(ValueError):
        components.label(maps, score=maps[:2], threshold=0.5)
    with pytest.raises(ValueError):
        components.label(maps.view(1, 3, H, W))
    with pytest.raises(ValueError):
        components.label(maps, max_jump=-0.1)
    with pytest.raises(ValueError):
        components.label(maps, lo=3.0, hi=2.0)
    with pytest.raises(RuntimeError):
        components.label(maps.cpu())


def speckles(H=48, W=160):
    img, disp, island = R.speckle_frame(H, W)
    return img, disp, island, dev(img).view(1, 3, H, W), dev(disp).view(1, 1, H, W)


def test_speckle_filter_on_the_mesh():
    """A step scene with 2 x 3 speckles: with K above the island size the mesh loses exactly the islands' faces, and keeps only large components."""
    H, W = 48, 160
    img, disp, island, d_img, d_disp = speckles(H, W)
    focal, baseline, K = 100.0, 0.5, island + 1
    _, sizes_ref, (comps, valid, largest) = R.label_ref(disp)
    assert valid == H * W and comps > 3 and int((sizes_ref == island).sum()) == (comps - 2) * island and largest > 1000
    sizes = components.size_score(d_disp)
    assert torch.equal(sizes.view(H, W).cpu(), torch.from_numpy(sizes_ref.astype(np.float32)))
    plain, plain_counts = mesh.build(d_img, d_disp, focal, baseline)
    kept, kept_counts = mesh.build(d_img, d_disp, focal, baseline, score=sizes, threshold=float(K))
    print("faces", plain_counts[0][1], "->", kept_counts[0][1], "vertices", plain_counts[0][0], "->", kept_counts[0][0])
    assert kept_counts[0][1] < plain_counts[0][1] and kept_counts[0][1] == plain_counts[0][1] - 4 * (comps - 2)  # a 2 x 3 island is four triangles
    want_v, want_f, ref = MR.build_ref(img, disp, focal, baseline, score=sizes_ref.astype(np.float32), threshold=float(K))
    assert torch.equal(kept[0][0].cpu(), torch.from_numpy(want_v.copy())) and torch.equal(kept[0][1].cpu(), torch.from_numpy(want_f.copy()))
    assert len(ref["used"]) == kept_counts[0][0] and int(sizes_ref.reshape(-1)[ref["used"]].min()) >= K
    # and K at the island size keeps everything: the threshold is >=
    assert mesh.build(d_img, d_disp, focal, baseline, score=sizes, threshold=float(island))[1] == plain_counts
    cloud, counts = components.filter_point_cloud(d_img, d_disp, K, focal=focal, baseline=baseline)
    assert counts == [int((sizes_ref >= K).sum())] and cloud[0].shape == (counts[0], 15)


def test_writers_equal_the_calls_made_by_hand(tmp_path):
    H, W = 48, 160
    img, disp, island, d_img, d_disp = speckles(H, W)
    K = island + 1
    conf = dev(np.random.default_rng(5).random((H, W)).astype(np.float32)).view(1, 1, H, W)
    focal, baseline = dumps.camera_for_width(W)
    fb = focal * baseline
    # the mesh: component_jump defaults to max_jump, the depth bounds go in as disparity bounds, the confidence enters the components only
    w = mesh.MeshWriter(str(tmp_path / "a"), max_jump=0.1, max_depth=60.0, min_conf=0.2, min_component=K)
    nv, nf = w.write(0, d_img, d_disp, conf=conf)
    sizes = components.size_score(d_disp, 0.1, lo=fb / 60.0, hi=float("inf"), score=conf, threshold=0.2)
    meshes, counts = mesh.build(d_img, d_disp, focal, baseline, max_jump=0.1, max_depth=60.0, score=sizes, threshold=float(K))
    raw = open(w.file(0), "rb").read()
    assert counts[0] == (nv, nf) and nf > 0 and w.summary()["min_component"] == K
    assert raw[raw.index(b"end_header\n") + 11:] == meshes[0][0].cpu().numpy().tobytes() + meshes[0][1].cpu().numpy().tobytes()
    no_filter = mesh.MeshWriter(str(tmp_path / "b"), max_jump=0.1, max_depth=60.0, min_conf=0.2).write(0, d_img, d_disp, conf=conf)
    assert nf < no_filter[1]
    w2 = mesh.MeshWriter(str(tmp_path / "c"), max_jump=0.1, min_depth=1.0, min_component=K, component_jump=0.3)
    got = w2.write(0, d_img, d_disp)
    sizes2 = components.size_score(d_disp, 0.3, lo=fb / 80.0, hi=fb / 1.0)
    assert got == mesh.build(d_img, d_disp, focal, baseline, max_jump=0.1, min_depth=1.0, score=sizes2, threshold=float(K))[1][0]
    # the scan
    import Test_KITTI as T
    P, fb_l = T.nominal_calibration(H, W)
    p = pseudo_lidar.PseudoLidarWriter(str(tmp_path / "d"), max_depth=60.0, min_depth=2.0, max_height=float("inf"), min_component=K, component_jump=0.1)
    n = p.write(0, d_disp, P, fb_l)
    sizes3 = components.size_score(d_disp, 0.1, lo=fb_l / 60.0, hi=fb_l / 2.0)
    pts = pseudo_lidar.unproject(d_disp, P, fb=fb_l, score=sizes3, threshold=float(K), max_depth=60.0, min_depth=2.0, max_height=float("inf"))
    assert n == pts.shape[0] > 0 and open(p.file(0), "rb").read() == pts.cpu().numpy().tobytes() and p.summary()["min_component"] == K
    plain = pseudo_lidar.PseudoLidarWriter(str(tmp_path / "e"), max_depth=60.0, min_depth=2.0, max_height=float("inf")).write(0, d_disp, P, fb_l)
    assert n < plain
    pc = pseudo_lidar.PseudoLidarWriter(str(tmp_path / "f"), min_conf=0.2, min_component=K)
    n_c = pc.write(0, d_disp, P, fb_l, conf=conf)
    sizes4 = components.size_score(d_disp, 0.05, lo=fb_l / 80.0, hi=float("inf"), score=conf, threshold=0.2)
    assert n_c == pseudo_lidar.unproject(d_disp, P, fb=fb_l, score=sizes4, threshold=float(K)).shape[0]
    s = components.ComponentsSummary(K, 0.05)
    s.add(d_disp)
    _, sizes_ref, (comps, valid, largest) = R.label_ref(disp)
    out = s.summary()
    assert (out["frames"], out["mean_components"], out["mean_valid"], out["largest"], out["min_component"]) == (1, comps, valid, largest, K)
    assert out["mean_small_share"] == int(((sizes_ref > 0) & (sizes_ref < K)).sum()) / valid


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def _child(script, argv, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, cwd=ROOT, env=dict(os.environ, FALNET_DETERMINISTIC="1"), capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_cli_end_to_end(tmp_path):
    import Test_KITTI as T
    H, W, K = 128, 416, 20  # the seeded weights give a noisy disparity: at a jump of 0.3 about a third of the pixels lie in pieces of 20 and more
    argv = ["--synthetic", "--height", str(H), "--width", str(W), "--iters", "1", "--mesh", "--mesh-max-jump", "0.5", "--pseudo-lidar", "--min-component", str(K),
            "--component-jump", "0.3", "--save-path", str(tmp_path / "cli")]
    out = _child(os.path.join("tests", "_components_cli.py"), [str(tmp_path / "rec")] + argv)
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert [list(ln)[0] for ln in lines[:3]] == ["pseudo_lidar", "mesh", "components"] and len(lines) == 4, out
    rec_m, rec_l = np.load(tmp_path / "rec" / "mesh_0.npz"), np.load(tmp_path / "rec" / "lidar_0.npz")
    assert np.array_equal(rec_m["disp"], rec_l["disp"]) and rec_m["disp"].shape == (H, W)
    d_disp, d_img = dev(rec_m["disp"]).view(1, 1, H, W), dev(rec_m["left"]).view(1, 3, H, W)
    # the components line: the module on the recorded disparity, and the definition
    labels_ref, sizes_ref, (comps, valid, largest) = R.label_ref(rec_m["disp"], max_jump=0.3)
    c = lines[2]["components"]
    print(c, lines[0], lines[1])
    assert components.label(d_disp, 0.3)[2] == [(comps, valid, largest)]
    assert (c["frames"], c["mean_components"], c["mean_valid"], c["largest"], c["min_component"], c["max_jump"]) == (1, comps, valid, largest, K, 0.3)
    assert c["mean_small_share"] == int(((sizes_ref > 0) & (sizes_ref < K)).sum()) / valid
    # the mesh file: mesh.build with the size map as its score
    focal, baseline = dumps.camera_for_width(W)
    sizes = components.size_score(d_disp, 0.3, lo=focal * baseline / 80.0)
    meshes, counts = mesh.build(d_img, d_disp, focal, baseline, max_jump=0.5, score=sizes, threshold=float(K))
    raw = open(tmp_path / "cli" / "Mesh" / "{:010d}.ply".format(0), "rb").read()
    assert raw[raw.index(b"end_header\n") + 11:] == meshes[0][0].cpu().numpy().tobytes() + meshes[0][1].cpu().numpy().tobytes()
    m = lines[1]["mesh"]
    assert (m["vertices"], m["faces"]) == counts[0] and m["min_component"] == K
    assert 0 < counts[0][1] < mesh.build(d_img, d_disp, focal, baseline, max_jump=0.5)[1][0][1] and 0 < c["mean_small_share"] < 1  # the filter bites, and leaves something
    # the scan
    P, fb = T.nominal_calibration(H, W)
    assert np.array_equal(rec_l["P"], P) and float(rec_l["fb"]) == fb
    pts = pseudo_lidar.unproject(d_disp, P, fb=fb, score=components.size_score(d_disp, 0.3, lo=fb / 80.0), threshold=float(K))
    assert open(tmp_path / "cli" / "Pseudo_lidar" / "{:010d}.bin".format(0), "rb").read() == pts.cpu().numpy().tobytes()
    assert lines[0]["pseudo_lidar"]["points"] == pts.shape[0] > 0 and lines[0]["pseudo_lidar"]["min_component"] == K


def test_cli_refuses_the_switch_without_a_product():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "Test_KITTI.py"), "--synthetic", "--height", "128", "--width", "416", "--iters", "1", "--min-component", "50"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--mesh" in p.stderr and "--pseudo-lidar" in p.stderr
