"""CPU: the depth mesh's definition (tests/_mesh_ref.py) holds its own invariants on every input family, mesh.save_ply round-trips through a
small PLY reader, the command line checks its switches, and the new entry points sit in the header, the binding and the build.  No device call."""
import importlib
import os
import re

import numpy as np
import pytest

import _mesh_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = [(2, 2), (3, 5), (37, 124)]


@pytest.mark.parametrize("H,W", SIZES, ids=["2x2", "3x5", "37x124"])
@pytest.mark.parametrize("name", R.FAMILIES)
def test_reference_invariants(name, H, W):
    f = R.family(name, H, W)
    vert, face, info = R.build_ref(f["img"], f["disp"], f["focal"], f["baseline"], **f["kw"])
    nv, nf, faces = len(vert), len(face), info["faces"]
    assert vert.shape == (nv, 15) and face.shape == (nf, 13) and faces.shape == (nf, 3)
    assert nf == 0 or (0 <= faces.min() and faces.max() < nv)                      # every index is a vertex
    assert np.array_equal(np.unique(faces), np.arange(nv))                         # every vertex is referenced
    assert (np.diff(info["used"]) > 0).all() and len(info["used"]) == nv           # in pixel order
    if name in ("plane", "inf-jump"):
        assert (nv, nf) == (H * W, 2 * (H - 1) * (W - 1))
    if name == "step" and W // 2 >= 1 and (H, W) != (2, 2):
        assert (nv, nf) == (H * W, 2 * (H - 1) * (W - 2))                          # the one column of quads across the edge goes, no vertex does
    if (name, H, W) == ("step", 37, 124):
        assert nf == 8784 and 2 * 36 * 123 == 8856
    if nf:
        xyz = info["xyz"].astype(np.float64)
        v0, v1, v2 = (xyz[faces[:, k]] for k in range(3))
        n = np.cross(v1 - v0, v2 - v0)
        facing = (n * v0).sum(1)
        print(f"{name} {H}x{W}: {nv} vertices, {nf} of {2 * (H - 1) * (W - 1)} faces, largest n.v0 {facing.max():.3e}")
        assert (facing < 0).all()                                                  # towards the camera, and so not degenerate
        assert (np.abs(n).sum(1) > 0).all()
    # a face record is the byte 3 and three little-endian int32; a vertex record the cloud's
    rec = np.frombuffer(face.tobytes(), R.FACE)
    assert (rec["n"] == 3).all() and np.array_equal(rec["v"], faces)
    if name in ("random", "quant", "holes") and (H, W) == (37, 124):
        assert 0 < nf < 2 * (H - 1) * (W - 1) and 0 < nv < H * W                   # the re-indexing is real


def test_reference_normals_are_unit_and_face_the_camera():
    f = R.family("holes", 37, 124)
    vert, _, info = R.build_ref(f["img"], f["disp"], f["focal"], f["baseline"], normals=True)
    v = np.frombuffer(vert.tobytes(), R.VERTEX_N)
    n = np.stack([v["nx"], v["ny"], v["nz"]], -1).astype(np.float64)
    assert vert.shape[1] == 27 and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
    assert ((n * info["xyz"].astype(np.float64)).sum(1) < 0).all()
    plain, _, _ = R.build_ref(f["img"], f["disp"], f["focal"], f["baseline"])
    p = np.frombuffer(plain.tobytes(), R.VERTEX)
    assert all(np.array_equal(p[k], v[k]) for k in R.VERTEX.names)  # the normals change nothing else


def test_reference_refuses_what_the_entry_point_refuses():
    f = R.family("plane", 3, 5)
    for kw in (dict(min_depth=-1.0), dict(max_depth=200.0), dict(min_depth=5.0, max_depth=5.0), dict(max_jump=-0.1), dict(max_jump=float("nan")),
               dict(max_depth=float("nan"))):
        with pytest.raises(ValueError):
            R.build_ref(f["img"], f["disp"], f["focal"], f["baseline"], **kw)


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
@pytest.mark.parametrize("fmt", ["binary", "ascii"])
def test_save_ply_round_trip(tmp_path, fmt, normals):
    from fal_net_amd import dumps, mesh
    f = R.family("holes", 37, 124)
    vert, face, info = R.build_ref(f["img"], f["disp"], f["focal"], f["baseline"], normals=normals)
    path = str(tmp_path / "m.ply")
    mesh.save_ply(path, vert, face, normals=normals, ply_format=fmt)
    got, faces, hdr = R.parse_ply(path)
    want = np.frombuffer(vert.tobytes(), R.VERTEX_N if normals else R.VERTEX)
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + ["diffuse_red", "diffuse_green", "diffuse_blue"]
    assert hdr["properties"] == names and hdr["vertex"] == len(want) and hdr["face"] == len(face)
    assert hdr["format"] == ("binary_little_endian" if fmt == "binary" else "ascii")
    # the vertex properties are the point cloud's, in its order
    cloud = [ln.split()[2] for ln in dumps._ply_header("ascii", 0).splitlines() if ln.startswith("property")]
    assert [n for n in names if n not in ("nx", "ny", "nz")] == cloud
    assert np.array_equal(faces, info["faces"])
    for a, b in zip(("diffuse_red", "diffuse_green", "diffuse_blue"), ("red", "green", "blue")):
        assert np.array_equal(got[a], want[b])
    for k in names[:-3]:
        if fmt == "binary":
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
        else:  # '%f': rounded to 1e-6 in decimal, then to the nearest f32 when read back
            assert (np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)) <= 5e-7 + 2.0 ** -24 * np.abs(want[k].astype(np.float64))).all(), k
    assert mesh.PLY_VERTEX_NORMALS == R.VERTEX_N and mesh.PLY_FACE == R.FACE and dumps.PLY_VERTEX == R.VERTEX
    with pytest.raises(ValueError):
        mesh.save_ply(path, vert, face, normals=normals, ply_format="obj")
    with pytest.raises(ValueError):
        mesh.save_ply(path, vert.reshape(-1)[:-1], face, normals=normals)


def test_writer_and_build_refuse_on_the_host(tmp_path):
    import torch
    from fal_net_amd import mesh
    for kw in (dict(max_jump=-1.0), dict(max_jump=float("nan")), dict(max_depth=200.0), dict(max_depth=0.0), dict(min_conf=0.0), dict(min_conf=1.5),
               dict(ply_format="obj")):
        with pytest.raises(ValueError):
            mesh.MeshWriter(str(tmp_path / "bad"), **kw)
    w = mesh.MeshWriter(str(tmp_path / "ok"), min_conf=0.5, normals=True)
    assert os.path.isdir(tmp_path / "ok" / "Mesh") and w.file(7).endswith(os.path.join("Mesh", "0000000007.ply"))
    s = w.summary()
    assert s["frames"] == 0 and s["normals"] is True and s["min_conf"] == 0.5 and s["mean_faces"] != s["mean_faces"]
    with pytest.raises(ValueError, match="confidence map"):
        w.write(0, torch.zeros(1, 3, 4, 5), torch.ones(1, 1, 4, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.build(torch.zeros(1, 3, 4, 5), torch.ones(1, 1, 4, 5), 100.0, 0.5)


def test_dump_kinds_and_folders_are_unchanged():
    from fal_net_amd import dumps
    assert dumps.DUMP_KINDS == ("disp", "input", "pan", "pc", "feats")
    assert "Mesh" not in dumps.FrameWriter.folders.values() and "mesh" not in dumps.FrameWriter.folders
    assert sorted(dumps.FrameWriter.folders.values()) == sorted(["l_disp", "Input im", "Pan", "Point_cloud", "feats"])


# ---- command line -------------------------------------------------------------------------------------------------------------------------------------
def test_parser_and_what_settings_hide(monkeypatch):
    monkeypatch.syspath_prepend(ROOT)
    mod = importlib.import_module("Test_KITTI")
    a = mod.parser.parse_args([])
    assert (a.mesh, a.mesh_max_jump, a.mesh_max_depth, a.mesh_min_conf, a.mesh_normals) == (False, 0.05, 80.0, None, False)
    mod.check_family_args(a)
    assert mod.MESH_ARGS == ("mesh", "mesh_max_jump", "mesh_max_depth", "mesh_min_conf", "mesh_normals") and set(mod.MESH_ARGS) <= set(vars(a))
    assert set(mod.MESH_ARGS) <= set(mod.hidden_settings(a))  # settings.txt keeps its lines without --mesh
    assert not set(mod.MESH_ARGS) & set(mod.hidden_settings(mod.parser.parse_args(["--mesh"])))
    a = mod.parser.parse_args(["--mesh", "--mesh-max-jump", "inf", "--mesh-max-depth", "60", "--mesh-min-conf", "0.5", "--mesh-normals"])
    assert (a.mesh, a.mesh_max_jump, a.mesh_max_depth, a.mesh_min_conf, a.mesh_normals) == (True, float("inf"), 60.0, 0.5, True)
    mod.check_family_args(a)
    for bad in (["--mesh-max-jump", "-0.1"], ["--mesh-max-jump", "nan"], ["--mesh-max-depth", "200"], ["--mesh-max-depth", "0"], ["--mesh-max-depth", "nan"],
                ["--mesh-min-conf", "0"], ["--mesh-min-conf", "1.5"]):
        with pytest.raises(SystemExit):
            mod.parser.parse_args(["--mesh"] + bad)
    for alone in (["--mesh-max-jump", "0.1"], ["--mesh-max-depth", "60"], ["--mesh-min-conf", "0.5"], ["--mesh-normals"]):
        with pytest.raises(SystemExit, match="--mesh"):
            mod.check_family_args(mod.parser.parse_args(alone))
        with pytest.raises(SystemExit, match=alone[0]):
            mod.check_family_args(mod.parser.parse_args(alone))
    mod.check_family_args(mod.parser.parse_args(["--mesh"]))  # and the other families' checks do not see it


def test_entry_points_in_header_binding_and_build():
    from fal_net_amd import _build, _lib, inference, mesh, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "falnet_hip.h")).read(), flags=re.S)
    assert re.search(r"\bfalnet_mesh_build\s*\(", hdr) and re.search(r"\bfalnet_mesh_workspace_bytes\s*\(", hdr)
    P, F, D, I = _lib._P, _lib._F, _lib._D, _lib._I
    assert _lib.SIGNATURES["falnet_mesh_build"] == [P, F, F, F, F, P, D, D, P, F, F, F, D, I, I, I, P, P, P, P, P]
    assert _lib.SIGNATURES["falnet_mesh_workspace_bytes"] == [I, I] and _lib._RESTYPES["falnet_mesh_workspace_bytes"] is _lib.C.c_int64
    assert "mesh.hip" in _build.SOURCES and _build.FILE_FLAGS["mesh.hip"] == ["-ffp-contract=off"] and _build.FILE_FLAGS["dump.hip"] == ["-ffp-contract=off"]
    assert "mesh.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600  # the packaged autotune cache stays valid
    src = open(os.path.join(_build.CSRC, "mesh.hip")).read()
    assert not re.search(r"atomic\w*\s*\(", src) and "block_rank" in src and "block_count" in src and "falnet_offset_scan" in src
    # the vertex chain is written once: in the header both files include
    dump = open(os.path.join(_build.CSRC, "dump.hip")).read()
    assert '#include "pc_vertex.h"' in src and '#include "pc_vertex.h"' in dump and "PcVertex pc_vertex(" not in dump and "PcVertex pc_vertex(" not in src
    assert callable(mesh.MeshWriter.frame) and callable(inference.run_products)


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "fal_net_amd", "libfalnet_hip.so")), reason="library not built")
def test_workspace_bytes_and_refusals_without_a_device():
    """The size function and every argument check run before anything touches the device."""
    from fal_net_amd import _lib as L
    lib = L.lib()
    n = 375 * 1242
    assert lib.falnet_mesh_workspace_bytes(375, 1242) == 16 * ((n + 2047) // 2048) + (4 * n + 7) // 8 * 8 + (n + 7) // 8 * 8
    assert lib.falnet_mesh_workspace_bytes(1, 1) == 16 + 8 + 8
    for bad in ((0, 5), (5, -1), (1 << 14, 1 << 14)):
        assert lib.falnet_mesh_workspace_bytes(*bad) == 0, bad
    fake = L.C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
    base = dict(img=fake, disp=fake, focal=100.0, baseline=0.5, score=None, threshold=0.0, min_depth=0.0, max_depth=80.0, max_jump=0.05, H=5, W=7, normals=0,
                vert=fake, face=fake, counts=fake, ws=fake)
    nan = float("nan")
    cases = [("null image", dict(img=None), "null image"), ("null disparity", dict(disp=None), "null image or disparity"),
             ("null vertices", dict(vert=None), "null output"), ("null faces", dict(face=None), "null output"), ("null counts", dict(counts=None), "null counts"),
             ("null workspace", dict(ws=None), "null counts or workspace"), ("H = 0", dict(H=0), "pixels"), ("W < 0", dict(W=-3), "pixels"),
             ("H W = 2^28", dict(H=1 << 14, W=1 << 14), "pixels"), ("focal = 0", dict(focal=0.0), "focal"), ("focal NaN", dict(focal=nan), "focal"),
             ("min_depth < 0", dict(min_depth=-1.0), "min_depth"), ("min_depth = max_depth", dict(min_depth=80.0), "min_depth"),
             ("max_depth = 200", dict(max_depth=200.0), "max_depth"), ("max_depth NaN", dict(max_depth=nan), "max_depth"), ("min_depth NaN", dict(min_depth=nan), "min_depth"),
             ("max_jump < 0", dict(max_jump=-0.01), "max_jump"), ("max_jump NaN", dict(max_jump=nan), "max_jump"),
             ("misaligned workspace", dict(ws=L.C.c_void_p((1 << 20) + 4)), "8-byte"), ("misaligned counts", dict(counts=L.C.c_void_p((1 << 20) + 4)), "8-byte"),
             ("misaligned output", dict(vert=L.C.c_void_p((1 << 20) + 2)), "4-byte")]
    for tag, change, word in cases:
        k = dict(base, **change)
        rc = lib.falnet_mesh_build(k["img"], 0.411, 0.432, 0.45, 255.0, k["disp"], k["focal"], k["baseline"], k["score"], k["threshold"], k["min_depth"],
                                   k["max_depth"], k["max_jump"], k["H"], k["W"], k["normals"], k["vert"], k["face"], k["counts"], k["ws"], None)
        assert rc != 0, tag
        assert re.search(word, lib.falnet_last_error().decode()), (tag, lib.falnet_last_error().decode())
