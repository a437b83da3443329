"""CPU: the host side of the test-time outputs (fal_net_amd/dumps.py, myUtils additions, Test_KITTI.py --dump): the shipped plasma table
against matplotlib's own PNG, PLY files against the reference's format expression, folder / file names, validation scalars, the parser."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def seeded_disp(shape):
    return (np.random.default_rng(0).random(shape) ** 3 * 120).astype(np.float32)


def plasma_host(disp, p95, lut):
    """Test_KITTI.py:213-216 restated with the table: v = 256 clip(d / (p95 + 1e-6), 0, 1) in f32, k = min(rint(v), 255), lut[k]."""
    v = np.float32(256) * np.clip(disp / (np.float32(p95) + np.float32(1e-6)), np.float32(0), np.float32(1))
    return lut[np.minimum(np.rint(v), 255).astype(np.int64)]


def test_plasma_table_reproduces_imsave(golden_dir):
    from fal_net_amd import dumps
    g = np.load(os.path.join(golden_dir, "dumps_plasma.npz"))
    lut = dumps.plasma_lut()
    assert lut.shape == (256, 4) and lut.dtype == np.uint8
    disp = seeded_disp((75, 250))
    p95 = np.percentile(disp, 95)
    assert p95 == g["p95_75x250"]
    assert (disp > p95).mean() > 0.04  # 5 % of the pixels saturate: index 256 -> the last entry
    got = plasma_host(disp, p95, lut)
    assert got.shape == g["rgba_75x250"].shape and np.array_equal(got, g["rgba_75x250"])


def test_dumps_module_does_not_need_matplotlib():
    src = open(os.path.join(ROOT, "fal_net_amd", "dumps.py")).read()
    assert "import matplotlib" not in src and "from matplotlib" not in src


def _ref_ascii(pc):
    """The reference's save_point_cloud body (myUtils.py:378-394), restated."""
    _, vertex_no = pc.shape
    s = 'ply\nformat ascii 1.0\nelement vertex {}\n'.format(vertex_no)
    s += 'property float x\nproperty float y\nproperty float z\n'
    s += 'property uchar diffuse_red\nproperty uchar diffuse_green\nproperty uchar diffuse_blue\nend_header\n'
    for i in range(vertex_no):
        s += '{:f} {:f} {:f} {:d} {:d} {:d}\n'.format(pc[0, i], pc[1, i], pc[2, i], int(pc[3, i]), int(pc[4, i]), int(pc[5, i]))
    return s


def _pc(n=5):
    rng = np.random.default_rng(11)
    pc = np.empty((6, n), np.float32)
    pc[:3] = (rng.standard_normal((3, n)) * 37).astype(np.float32)
    pc[1, 0], pc[0, 1] = 200.0, -1234.56789  # a capped depth, more than six integer digits' worth of formatting
    pc[3:] = rng.random((3, n)).astype(np.float32) * 255
    pc[3, 2], pc[4, 3] = 254.99998, 0.999  # colours are truncated, not rounded
    return pc


def test_save_point_cloud_ascii_and_binary(tmp_path):
    import myUtils as utils  # the drop-in alias picks the new names up
    from fal_net_amd import dumps
    pc = _pc()
    f = tmp_path / "a.ply"
    utils.save_point_cloud(pc, str(f))
    assert f.read_text() == _ref_ascii(pc)
    fb = tmp_path / "b.ply"
    utils.save_point_cloud(pc, str(fb), ply_format="binary")
    raw = fb.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 5"]
    assert lines[3:] == ["property float x", "property float y", "property float z", "property uchar diffuse_red", "property uchar diffuse_green",
                         "property uchar diffuse_blue"]
    assert dumps.PLY_VERTEX.itemsize == 15 and len(body) == 15 * 5
    rec = np.frombuffer(body, dtype=dumps.PLY_VERTEX)
    for k, name in enumerate(("x", "y", "z")):
        assert np.array_equal(rec[name], pc[k])
    for k, name in enumerate(("red", "green", "blue")):
        assert np.array_equal(rec[name], pc[3 + k].astype(np.int64))
    assert rec["red"][2] == 254 and rec["green"][3] == 0
    # a large cloud goes through the block formatter: more vertices than one block
    big = np.tile(_pc(7), (1, 10000))[:, :66001]
    utils.save_point_cloud(big, str(f))
    txt = f.read_text()
    assert txt.count("\n") == 10 + 66001 and txt.endswith(_ref_ascii(big[:, -3:]).split("end_header\n")[1])
    with pytest.raises(ValueError):
        dumps.save_ply(str(f), planar=pc, ply_format="obj")


def test_frame_writer_folders_and_names(tmp_path):
    from fal_net_amd import dumps
    w = dumps.FrameWriter(str(tmp_path / "res"), ("disp", "pc"), ply_format="ascii")
    assert sorted(os.listdir(tmp_path / "res")) == sorted(["l_disp", "Input im", "Pan", "Point_cloud", "feats"])  # Test_KITTI.py:140-158
    assert w.file("disp", 7) == os.path.join(str(tmp_path / "res"), "l_disp", "0000000007.png")
    assert w.file("input", 7) == os.path.join(str(tmp_path / "res"), "Input im", "0000000007.png")
    assert w.file("pan", 12) == os.path.join(str(tmp_path / "res"), "Pan", "0000000012.png")
    assert w.file("pc", 3) == os.path.join(str(tmp_path / "res"), "Point_cloud", "0000000003.ply")
    assert w.file("feats", 3, 1, 2) == os.path.join(str(tmp_path / "res"), "feats", "0000000003_l1_c2.png")
    assert not w.needs_views and dumps.FrameWriter(str(tmp_path / "r2"), ("feats",)).needs_views and dumps.FrameWriter(str(tmp_path / "r3"), ("pan",)).needs_views
    with pytest.raises(ValueError):
        dumps.FrameWriter(str(tmp_path / "r4"), ("disp", "depth"))
    with pytest.raises(ValueError):
        dumps.FrameWriter(str(tmp_path / "r5"), ("pc",), ply_format="obj")
    assert dumps.camera_for_width(1242) == (721.5377, 0.9982 * 0.54)
    f, b = dumps.camera_for_width(320)
    assert abs(f - 721.5377 * 320 / 1242) < 1e-9 and b == 0.9982 * 0.54


def test_no_cpu_fallback():
    from fal_net_amd import dumps
    with pytest.raises(RuntimeError, match="MI355X"):
        dumps.image_u8(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):
        dumps.percentile(torch.zeros(1, 16), 95)


def test_get_point_cloud_unknown_width_raises_keyerror():
    import myUtils as utils
    with pytest.raises(KeyError):
        utils.get_point_cloud(torch.zeros(1, 3, 8, 320), torch.zeros(1, 1, 8, 320))


def test_validation_scalars_vs_reference_formulas():
    """get_mea / get_rmse / get_psnr against myUtils.py:123-172 restated (mean_shift tensor, in-place clamps)."""
    import myUtils as utils
    g = torch.Generator().manual_seed(3)
    out = torch.rand(2, 3, 17, 23, generator=g) * 1.4 - 0.7  # beyond [0, 1] after the shift: the clamps act
    lab = torch.rand(2, 3, 17, 23, generator=g) - 0.43
    mean = (0.411, 0.432, 0.45)
    shift = torch.zeros(out.shape)
    for c in range(3):
        shift[:, c] = mean[c]
    o = (out + shift) * 255
    o[o > 255] = 255
    o[o < 0] = 0
    l = (lab + shift) * 255
    assert float(((o > 254.999) | (o < 0.001)).float().mean()) > 0.05
    assert torch.allclose(utils.get_mea(out, lab), torch.mean(torch.abs(o - l)), rtol=1e-6)
    assert torch.allclose(utils.get_rmse(out, lab), torch.mean((o - l) ** 2) ** (1 / 2), rtol=1e-6)
    imdiff = (o.round() - l).view(2, -1)
    psnr = torch.mean(20 * torch.log10(255 / torch.sqrt(torch.mean(imdiff ** 2))))
    assert torch.allclose(utils.get_psnr(out, lab), psnr, rtol=1e-6)


def _entry():
    spec = importlib.util.spec_from_file_location("Test_KITTI_entry_dumps", os.path.join(ROOT, "Test_KITTI.py"))
    tk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tk)
    return tk


def test_test_kitti_dump_flags():
    tk = _entry()
    d = tk.parser.parse_args([])
    assert d.dump == [] and d.ply_format == "binary" and d.device_percentile is False
    # the reference's defaults are what they were (the tuple of test_host_logic)
    assert (d.tdataName, d.max_disp, d.min_disp, d.batch_size, d.evaluate, d.save, d.save_pc, d.save_pan, d.save_input, d.workers, d.sparse,
            d.print_freq, d.dataset, d.time_stamp, d.model, d.no_levels, d.details, d.f_post_process, d.ms_post_process, d.median, d.rel_baselne) == \
        ("Kitti_eigen_test_improved", 300, 2, 1, True, False, False, False, False, 4, False, 10, "Kitti_stage2", "10-18-15_42", "FAL_netB", 49,
         ",e20es,b4,lr5e-05/checkpoint.pth.tar", False, True, False, 1)
    a = tk.parser.parse_args(["--dump", "disp,input,pan,pc,feats", "--ply-format", "ascii"])
    assert a.dump == ["disp", "input", "pan", "pc", "feats"] and a.ply_format == "ascii"
    assert tk.parser.parse_args(["--dump", "pc"]).dump == ["pc"]
    tk.refuse_out_of_scope(a)  # --dump is not one of the refused switches
    with pytest.raises(SystemExit):
        tk.parser.parse_args(["--dump", "disp,depth"])
    with pytest.raises(SystemExit, match="out of scope"):  # -save* stay refused with the present message
        tk.refuse_out_of_scope(tk.parser.parse_args(["--dump", "disp", "-save", "True"]))


def test_binding_declares_the_dump_entry_points():
    from fal_net_amd import _build, _lib
    for name in ("falnet_percentile_f32", "falnet_percentile_workspace_bytes", "falnet_disp_to_plasma_u8", "falnet_image_to_u8", "falnet_feature_to_u8",
                 "falnet_local_norm", "falnet_point_cloud"):
        assert name in _lib.SIGNATURES
    assert "dump.hip" in _build.SOURCES
    from fal_net_amd import ops
    assert "dump.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600  # the packaged autotune cache stays valid


def test_optimiser_packer_and_weight_gradients_are_outside_the_tuned_sources():
    import os
    from fal_net_amd import _build, ops
    for name in ("pack.hip", "wgrad.hip"):  # built, and a change to them leaves the packaged autotune cache valid
        assert name in _build.SOURCES and name not in ops._TUNE_SOURCES
    assert ops._TUNE_SOURCES == ("conv.hip", "conv_dma.hip", "conv_wave.hip", "conv_epilogue.h", "common.h")
    assert "adam_pack_wd.hip" not in _build.SOURCES and not os.path.exists(os.path.join(_build.CSRC, "adam_pack_wd.hip"))  # ONE pack_tile: pack.hip
    assert all(os.path.isfile(os.path.join(_build.CSRC, s)) for s in _build.SOURCES)
