"""GPU: the depth mesh (fal_net_amd/mesh.py: build, csrc/mesh.hip) against its definition on the host (tests/_mesh_ref.py: build_ref, whose own
invariants tests/test_mesh_host.py holds).  Every comparison with the reference is torch.equal on bytes and counts: the f32 vertex chain is the point
cloud's, a kept triangle is decided by correctly rounded f32 operations and comparisons, and the normals are correctly rounded f64 operations in a
stated order, so there is no tolerance anywhere.  The device path is never compared with itself, except where the property IS self-agreement (two
calls)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _mesh_ref as R  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import dumps, mesh  # noqa: E402

DEV = "cuda"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# 1 x 7: no quad; 2 x 2: one; 3 x 5: a partial wave; 37 x 124: 4588 pixels, three ORD_TILE ranges of 2048 with a partial last one, for the vertices and
# for the faces (which are ranked twice per round); 75 x 250: ten ranges, rows that start anywhere in a round
SIZES = [(1, 7), (2, 2), (3, 5), (37, 124), (75, 250)]
NORMAL_SIZES = [(3, 5), (37, 124), (75, 250)]
GUARD = 4096  # bytes behind the worst-case buffers
FILL = 0xFF   # as f32 a NaN, as an index -1


@functools.lru_cache(maxsize=None)
def frame(name, H, W, kitti_camera=False):
    """One family's inputs at one size, computed once per session and left unchanged."""
    if kitti_camera:
        focal, baseline = dumps.camera_for_width(W)
        return R.family(name, H, W, focal, baseline)
    return R.family(name, H, W)


@functools.lru_cache(maxsize=None)
def reference(name, H, W, normals, kitti_camera=False):
    f = frame(name, H, W, kitti_camera)
    return R.build_ref(f["img"], f["disp"], f["focal"], f["baseline"], normals=normals, **f["kw"])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(nbytes):
    return torch.full(((nbytes + 3) // 4 * 4 + GUARD,), FILL, dtype=torch.uint8, device=DEV)


def raw_build(f, normals, bufs=(None, None, None, None), **change):
    """falnet_mesh_build on the inputs of `f` into pre-filled, guarded worst-case buffers (or into bufs = (vert, face, counts, ws)), with the arguments
    named in `change` replaced -> (rc, vert, face, counts)."""
    vert, face, counts, ws = bufs
    H, W = f["disp"].shape
    lib = L.lib()
    rec = 27 if normals else 15
    vert = guarded(H * W * rec) if vert is None else vert
    face = guarded(2 * (H - 1) * (W - 1) * 13) if face is None else face
    counts = torch.full((2,), -7, dtype=torch.int64, device=DEV) if counts is None else counts
    ws = torch.empty(int(lib.falnet_mesh_workspace_bytes(H, W)) // 8, dtype=torch.int64, device=DEV) if ws is None else ws
    kw = f["kw"]
    k = dict(img=dev(f["img"]), disp=dev(f["disp"]), focal=float(f["focal"]), baseline=float(f["baseline"]), score=dev(kw.get("score")),
             threshold=float(kw.get("threshold", 0.0)), min_depth=0.0, max_depth=80.0, max_jump=float(kw.get("max_jump", 0.05)), H=H, W=W, normals=int(normals),
             vert=vert, face=face, counts=counts, ws=ws)
    k.update(change)
    as_ptr = lambda v: L.ptr(v) if torch.is_tensor(v) or v is None else v  # noqa: E731
    rc = lib.falnet_mesh_build(as_ptr(k["img"]), R.MEAN[0], R.MEAN[1], R.MEAN[2], 255.0, as_ptr(k["disp"]), k["focal"], k["baseline"], as_ptr(k["score"]),
                               k["threshold"], k["min_depth"], k["max_depth"], k["max_jump"], k["H"], k["W"], k["normals"], as_ptr(k["vert"]), as_ptr(k["face"]),
                               as_ptr(k["counts"]), as_ptr(k["ws"]), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, vert, face, counts


def check(f, want, normals, tag):
    """The two record streams and the counts are the reference's byte for byte; the bytes beyond them, and the guard, keep their fill."""
    want_v, want_f, _ = want
    rec = 27 if normals else 15
    rc, vert, face, counts = raw_build(f, normals)
    assert rc == 0, tag
    nv, nf = counts.tolist()
    print(f"{tag}: {nv} vertices (reference {len(want_v)}), {nf} faces (reference {len(want_f)})")
    assert torch.equal(counts.cpu(), torch.tensor([len(want_v), len(want_f)])), tag
    assert torch.equal(vert[:nv * rec].cpu(), torch.from_numpy(want_v.copy()).reshape(-1)), tag + ": vertex bytes"
    assert torch.equal(face[:nf * 13].cpu(), torch.from_numpy(want_f.copy()).reshape(-1)), tag + ": face bytes"
    assert bool((vert[nv * rec:] == FILL).all()) and bool((face[nf * 13:] == FILL).all()), tag + ": written beyond the kept records"
    return vert[:nv * rec].view(nv, rec), face[:nf * 13].view(nf, 13)


# ---- byte for byte against the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", R.FAMILIES)
def test_equals_reference(name, H, W):
    check(frame(name, H, W), reference(name, H, W, False), False, f"{name} {H}x{W}")
    if (H, W) in NORMAL_SIZES:
        check(frame(name, H, W), reference(name, H, W, True), True, f"{name} {H}x{W} normals")


def test_counts_of_the_families():
    """What the families are for, on the reference the device was just held to."""
    H, W = 37, 124
    full = (H * W, 2 * (H - 1) * (W - 1))
    n = {name: (len(reference(name, H, W, False)[0]), len(reference(name, H, W, False)[1])) for name in R.FAMILIES}
    print(n)
    assert n["plane"] == full and n["inf-jump"] == full and n["step"] == (H * W, 8784)
    assert 0 < n["holes"][0] < H * W and 0 < n["random"][1] < full[1] // 4 and 0 < n["quant"][1] < full[1] and 0 < n["score"][0] < H * W


def test_past_one_chunk_of_tile_counts():
    """513 x 1025 with the KITTI camera: 257 ranges, one more than the offset scan takes at a time, so its carried base places the last range's records."""
    H, W = 513, 1025
    f, want = frame("holes", H, W, True), reference("holes", H, W, False, True)
    check(f, want, False, f"holes {H}x{W}")
    used, faces = want[2]["used"], want[2]["faces"]
    assert 0 < int((used >= 256 * 2048).sum()) < len(used) and len(faces) > 256 * 2048  # records on both sides of the 257th range's first pixel


def test_a_frame_without_a_quad_writes_only_the_counts():
    for H, W in ((1, 7), (9, 1), (1, 1)):
        f = R.family("plane", H, W)
        rc, vert, face, counts = raw_build(f, True)
        assert rc == 0 and counts.tolist() == [0, 0] and bool((vert == FILL).all()) and bool((face == FILL).all()), (H, W)


# ---- independent of the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["holes", "random", "score"])
def test_vertices_are_the_point_clouds(name):
    H, W = 75, 250
    f = frame(name, H, W)
    kw = dict(f["kw"])
    if "score" in kw:
        kw["score"] = dev(kw["score"]).view(1, 1, H, W)
    img, disp = dev(f["img"]).view(1, 3, H, W), dev(f["disp"]).view(1, 1, H, W)
    meshes, counts = mesh.build(img, disp, f["focal"], f["baseline"], **kw)
    cloud = dumps.point_cloud(img, disp, f["focal"], f["baseline"], packed=True)[0]
    used = torch.from_numpy(reference(name, H, W, False)[2]["used"]).to(DEV)
    vert, face = meshes[0]
    assert counts[0] == (vert.shape[0], face.shape[0]) and 0 < vert.shape[0] < H * W
    assert torch.equal(vert, cloud[used])
    # and every face names vertices of ONE quad of the grid, each index below the count
    idx = torch.from_numpy(np.frombuffer(face.cpu().numpy().tobytes(), R.FACE)["v"].astype(np.int64)).to(DEV)
    assert int(idx.min()) >= 0 and int(idx.max()) < vert.shape[0]
    pix = used[idx]
    i, j = pix // W, pix % W
    assert bool((i.max(1).values - i.min(1).values == 1).all()) and bool((j.max(1).values - j.min(1).values == 1).all())


def test_wrapper_takes_a_batch_and_reads_the_counts_once():
    H, W = 37, 124
    names = ("plane", "holes", "quant")
    img = torch.stack([dev(frame(n, H, W)["img"]) for n in names])
    disp = torch.stack([dev(frame(n, H, W)["disp"]) for n in names]).view(3, 1, H, W)
    for normals in (False, True):
        meshes, counts = mesh.build(img, disp, 100.0, 0.5, normals=normals)
        for b, n in enumerate(names):
            want_v, want_f, _ = reference(n, H, W, normals)
            assert counts[b] == (len(want_v), len(want_f))
            assert meshes[b][0].is_cuda and meshes[b][0].dtype == torch.uint8 and meshes[b][0].shape == want_v.shape and meshes[b][1].shape == want_f.shape
            assert torch.equal(meshes[b][0].cpu(), torch.from_numpy(want_v.copy())) and torch.equal(meshes[b][1].cpu(), torch.from_numpy(want_f.copy()))
    with pytest.raises(ValueError):
        mesh.build(img, disp, 100.0, 0.5, score=disp)
    with pytest.raises(ValueError):
        mesh.build(img, disp, 100.0, 0.5, max_depth=250.0)
    with pytest.raises(ValueError):
        mesh.build(img[:2], disp, 100.0, 0.5)
    with pytest.raises(KeyError):
        mesh.build(img, disp)  # 124 is no KITTI width


# ---- memory discipline ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes_in_either_mode():
    H, W = 75, 250
    f = frame("holes", H, W)
    want_v, want_f, _ = reference("holes", H, W, True)
    lib = L.lib()
    runs = []
    try:
        for mode in (1, 0, 1, 0):
            lib.falnet_set_deterministic(mode)
            rc, vert, face, counts = raw_build(f, True)
            assert rc == 0
            runs.append((vert, face, counts))
    finally:
        lib.falnet_set_deterministic(1 if L.DETERMINISTIC else 0)
    for vert, face, counts in runs[1:]:
        assert torch.equal(vert, runs[0][0]) and torch.equal(face, runs[0][1]) and torch.equal(counts, runs[0][2])  # the fill beyond the records included
    assert runs[0][2].tolist() == [len(want_v), len(want_f)] and runs[0][0].data_ptr() != runs[1][0].data_ptr()


def test_every_refused_argument_returns_nonzero_and_writes_nothing():
    H, W = 37, 124
    f = frame("score", H, W)
    want_v, want_f, _ = reference("score", H, W, False)
    vert, face = guarded(H * W * 15), guarded(2 * (H - 1) * (W - 1) * 13)
    counts = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((int(L.lib().falnet_mesh_workspace_bytes(H, W)) // 8 + 1,), -7, dtype=torch.int64, device=DEV)
    nan = float("nan")
    odd = lambda t, k: L.C.c_void_p(t.data_ptr() + k)  # noqa: E731
    cases = [("null image", dict(img=None), "null image"), ("null disparity", dict(disp=None), "null image or disparity"), ("null vertices", dict(vert=None), "null output"),
             ("null faces", dict(face=None), "null output"), ("null counts", dict(counts=None), "null counts"), ("null workspace", dict(ws=None), "null counts or workspace"),
             ("H = 0", dict(H=0), "pixels"), ("W < 0", dict(W=-3), "pixels"), ("H W = 2^28", dict(H=1 << 14, W=1 << 14), "pixels"),
             ("focal = 0", dict(focal=0.0), "focal"), ("focal < 0", dict(focal=-100.0), "focal"), ("min_depth < 0", dict(min_depth=-0.5), "min_depth"),
             ("min_depth >= max_depth", dict(min_depth=80.0), "min_depth"), ("max_depth = 200", dict(max_depth=200.0), "max_depth"),
             ("max_depth NaN", dict(max_depth=nan), "max_depth"), ("max_jump < 0", dict(max_jump=-0.05), "max_jump"), ("max_jump NaN", dict(max_jump=nan), "max_jump"),
             ("misaligned workspace", dict(ws=odd(ws.view(torch.uint8), 4)), "8-byte"), ("misaligned counts", dict(counts=odd(counts.view(torch.uint8), 4)), "8-byte"),
             ("misaligned vertices", dict(vert=odd(vert, 1)), "4-byte"), ("misaligned faces", dict(face=odd(face, 2)), "4-byte")]
    for tag, change, word in cases:
        rc = raw_build(f, False, (vert, face, counts[:2], ws), **change)[0]
        assert rc != 0, tag
        with pytest.raises(RuntimeError, match=word):
            L.check(rc, "mesh_build")
        assert bool((counts == -7).all()) and bool((vert == FILL).all()) and bool((face == FILL).all()) and bool((ws == -7).all()), tag  # nothing ran
    rc = raw_build(f, False, (vert, face, counts[:2], ws))[0]  # and the next valid call is correct
    assert rc == 0 and counts.tolist() == [len(want_v), len(want_f), -7, -7]
    assert torch.equal(vert[:want_v.size].cpu(), torch.from_numpy(want_v.copy()).reshape(-1)) and int(ws[-1]) == -7
    # max_jump = infinity is legal (the inf-jump family); so is a threshold without a score map
    assert raw_build(frame("plane", 3, 5), False, threshold=nan)[0] == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------
def _child(script, argv, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, cwd=ROOT, env=dict(os.environ, FALNET_DETERMINISTIC="1"), capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout


def test_cli_end_to_end(tmp_path):
    H, W = 128, 416
    argv = ["--synthetic", "--height", str(H), "--width", str(W), "--iters", "1", "--mesh", "--mesh-normals", "--mesh-max-jump", "0.5"]
    out = _child("Test_KITTI.py", argv + ["--save-path", str(tmp_path / "cli")])
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2 and list(lines[0]) == ["mesh"], out
    s = lines[0]["mesh"]
    path = tmp_path / "cli" / "Mesh" / "{:010d}.ply".format(0)
    vert, faces, hdr = R.parse_ply(str(path))
    print(s)
    assert hdr["format"] == "binary_little_endian" and hdr["properties"][3:6] == ["nx", "ny", "nz"]
    assert s["frames"] == 1 and s["vertices"] == s["mean_vertices"] == hdr["vertex"] == len(vert) and s["faces"] == s["mean_faces"] == hdr["face"] == len(faces)
    assert s["kept_fraction"] == pytest.approx(len(faces) / (2 * (H - 1) * (W - 1))) and s["max_jump"] == 0.5 and s["normals"] is True
    assert len(faces) > 0 and faces.min() >= 0 and faces.max() < len(vert)
    # the same command line once more, in a process that also records what the mesh is made of: the same file, and its records are mesh.build's and the
    # definition's on the recorded disparity
    _child(os.path.join("tests", "_mesh_cli.py"), [str(tmp_path / "rec")] + argv + ["--save-path", str(tmp_path / "again")])
    raw = open(path, "rb").read()
    assert open(tmp_path / "again" / "Mesh" / "{:010d}.ply".format(0), "rb").read() == raw
    rec = np.load(tmp_path / "rec" / "frame_0.npz")
    assert rec["disp"].shape == (H, W) and rec["conf"].size == 0
    focal, baseline = dumps.camera_for_width(W)
    meshes, counts = mesh.build(dev(rec["left"]).view(1, 3, H, W), dev(rec["disp"]).view(1, 1, H, W), focal, baseline, max_jump=0.5, normals=True)
    body = raw[raw.index(b"end_header\n") + len(b"end_header\n"):]
    assert counts[0] == (len(vert), len(faces)) and body == meshes[0][0].cpu().numpy().tobytes() + meshes[0][1].cpu().numpy().tobytes()
    want_v, want_f, _ = R.build_ref(rec["left"], rec["disp"], focal, baseline, max_jump=0.5, normals=True)
    assert body == want_v.tobytes() + want_f.tobytes()


def test_cli_without_the_switch_writes_nothing_new(tmp_path):
    out = _child("Test_KITTI.py", ["--synthetic", "--height", "128", "--width", "416", "--iters", "1", "--save-path", str(tmp_path / "plain")])
    lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and "mesh" not in lines[0] and not os.path.exists(tmp_path / "plain" / "Mesh")
