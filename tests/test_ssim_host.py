"""CPU: the host side of SSIM -- the float64 definition of tests/_ssim_ref.py (window weights, the analytic adjoint the kernel implements against
autograd), the entry points in the header, the binding, the build list and INTEGRATION.md, the metric's column, and the new command-line switches.
No GPU."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

import _ssim_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY_POINTS = ("falnet_ssim_workspace_bytes", "falnet_ssim_metric", "falnet_ssim_loss_fwd", "falnet_ssim_loss_bwd", "falnet_ssim_loss_fwd_bwd")


def test_window_weights_sum_to_one():
    g = R.gauss_weights()
    assert g.dtype == torch.float64 and len(g) == 11 and abs(float(g.sum()) - 1.0) <= 2e-16
    assert torch.equal(g, g.flip(0)) and float(g[5]) == float(g.max())
    assert abs(float(g[4] / g[5]) - float(torch.exp(torch.tensor(-1.0 / 4.5, dtype=torch.float64)))) <= 1e-15  # sigma = 1.5
    b = R.box_weights()
    assert len(b) == 3 and abs(float(b.sum()) - 1.0) <= 2e-16 and float(b[0]) == float(b[2]) == 1.0 / 3.0
    assert R.METRIC_C1 == (0.01 * 255) ** 2 and R.METRIC_C2 == (0.03 * 255) ** 2 and R.LOSS_C1 == 1e-4 and abs(R.LOSS_C2 - 9e-4) < 1e-18


@pytest.mark.parametrize("shape,weights,c1,c2", [((2, 3, 3, 3), "box", R.LOSS_C1, R.LOSS_C2), ((1, 2, 7, 10), "box", R.LOSS_C1, R.LOSS_C2),
                                                 ((1, 1, 13, 12), "gauss", R.LOSS_C1, R.LOSS_C2), ((1, 1, 12, 14), "gauss", R.METRIC_C1, R.METRIC_C2)])
def test_analytic_adjoint_equals_autograd(shape, weights, c1, c2):
    """The formulas of csrc/ssim.hip's backward (A, Bm, Cm gathered over the windows that contain a pixel) are the gradient of the f64 definition."""
    g = R.box_weights() if weights == "box" else R.gauss_weights()
    gen = torch.Generator().manual_seed(3)
    scale = 255.0 if c1 == R.METRIC_C1 else 1.0
    x = (torch.rand(shape, generator=gen, dtype=torch.float64) * scale).requires_grad_(True)
    y = torch.rand(shape, generator=gen, dtype=torch.float64) * scale
    S = R.ssim_map(x, y, g, c1, c2)
    u = -0.5 * 0.37 / S.numel()  # the loss's upstream scalar: -gscale * scale / 2 per window
    (u * S.sum()).backward()
    got = R.analytic_grad(x.detach(), y, g, c1, c2, u)
    err = float((got - x.grad).abs().max())
    print("analytic adjoint vs autograd", shape, weights, "max abs", err, "of", float(x.grad.abs().max()))
    assert err <= 1e-13 * max(float(x.grad.abs().max()), 1e-300) + 1e-18
    assert float(x.grad.abs().min()) > 0 and got.shape == x.shape  # every pixel, the corners with their one window included


def test_identical_planes_and_constants_in_the_definition():
    x = torch.rand(1, 1, 12, 15, dtype=torch.float64) * 255
    assert float((R.ssim_map(x, x, R.gauss_weights(), R.METRIC_C1, R.METRIC_C2) - 1).abs().max()) <= 1e-12
    a, b = torch.full((1, 1, 11, 11), 40.0, dtype=torch.float64), torch.full((1, 1, 11, 11), 90.0, dtype=torch.float64)
    s = float(R.ssim_map(a, b, R.gauss_weights(), R.METRIC_C1, R.METRIC_C2))
    assert abs(s - (2 * 40 * 90 + R.METRIC_C1) / (40 ** 2 + 90 ** 2 + R.METRIC_C1)) <= 1e-12
    m = R.loss_map(*R.pair((2, 3, 9, 8), 1))
    assert m.shape == (2, 3, 7, 6) and float(m.min()) >= 0 and float(m.max()) <= 1  # |S| <= 1: no clamp


def test_case_lists():
    assert R.METRIC_SHAPES == [(1, 11, 11), (2, 13, 70), (1, 45, 77), (1, 75, 250)]
    assert R.LOSS_SHAPES == [(40, 3, 3, 3), (2, 3, 5, 9), (1, 1, 19, 35), (1, 3, 37, 70), (2, 3, 64, 128)]
    assert all(h >= 3 and w >= 3 for _, _, h, w in R.LOSS_SHAPES) and all(h >= 11 and w >= 11 for _, h, w in R.METRIC_SHAPES)


def _decl_args(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_in_header_binding_build_and_document():
    from fal_net_amd import _build, _lib, ops
    hdr = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    C = _lib.C
    kinds = {"float": C.c_float, "double": C.c_double, "int": C.c_int, "int64_t": C.c_int64}
    for name in ENTRY_POINTS:
        args = _decl_args(hdr, name)
        sig = _lib.SIGNATURES[name]
        assert len(args) == len(sig), (name, args, sig)
        for a, t in zip(args, sig):  # pointer for pointer, scalar type for scalar type
            want = C.c_void_p if "*" in a else kinds[a.split()[-2]]
            assert t is want, (name, a, t)
        assert name in doc, name
    assert _lib._RESTYPES["falnet_ssim_workspace_bytes"] is C.c_int64
    for name in ENTRY_POINTS[1:]:
        assert _lib.SIGNATURES[name][-1] is C.c_void_p  # the stream
    assert "ssim.hip" in _build.SOURCES and _build.FILE_FLAGS["ssim.hip"] == ["-ffp-contract=off"]
    assert "ssim.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600  # the packaged autotune cache stays valid


def test_metric_column():
    from fal_net_amd import metrics as M
    hdr = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    assert re.search(r"#define FALNET_MET_SSIM 23\b", hdr) and re.search(r"#define FALNET_MET_ROW 24\b", hdr)
    assert M.ROW == 24 and M.COLUMNS[23] == "ssim" and M.COL["ssim"] == 23 and "reserved" not in M.COL
    assert inspect.signature(M.ssim).parameters["mean"].default == M.MEAN and inspect.signature(M.ssim).parameters["out"].default is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.ssim(torch.zeros(1, 3, 12, 12), torch.zeros(1, 3, 12, 12))
    from fal_net_amd import myUtils as utils
    assert list(inspect.signature(utils.get_ssim).parameters) == ["output_right", "label_right", "mean"]


def test_ssim_loss_surface():
    from fal_net_amd import loss_functions as LF
    p = inspect.signature(LF.ssim_loss).parameters
    assert list(p) == ["synth", "label", "window", "mean"] and p["window"].default == 3 and tuple(p["mean"].default) == R.MEAN
    x = torch.zeros(1, 3, 8, 8)
    for w in (1, 5, 11, None):
        with pytest.raises(ValueError, match="3 x 3"):
            LF.ssim_loss(x, x, window=w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # never a quiet host path
        LF.ssim_loss(x, x)
    assert list(inspect.signature(LF.rec_loss_fnc).parameters) == ["mask", "synth", "label", "vgg_label", "a_p"]  # unchanged


def test_steps_and_loops_take_the_switches_off_by_default():
    from fal_net_amd import inference, train
    for f in (train.stage1_step, train.stage1_slow_step):
        assert inspect.signature(f).parameters["a_ssim"].default == 0.0
    assert "a_ssim" not in inspect.signature(train.stage2_step).parameters
    assert inspect.signature(inference.evaluate).parameters["products"].default == ()


def test_new_switches_parse(monkeypatch):
    """-ssim / --a_ssim on the Stage-1 parser (shared by the two derived scripts), --view-metrics on Test_KITTI.py; both off by default."""
    import importlib
    monkeypatch.syspath_prepend(ROOT)
    tr = importlib.import_module("Train_Stage1_K")
    assert tr.parser.parse_args([]).a_ssim == 0.0
    assert tr.parser.parse_args(["-ssim", "0.15"]).a_ssim == 0.15 and tr.parser.parse_args(["--a_ssim", "0.85"]).a_ssim == 0.85
    src = open(os.path.join(ROOT, "Train_Stage1_K.py")).read()
    assert "a_ssim=args.a_ssim" in src
    for script in ("Train_Stage1_Kslow.py", "Train_Stage2_K.py"):
        s = open(os.path.join(ROOT, script)).read()
        assert "import Train_Stage1_K as base" in s and "base.parser.parse_args()" in s
    te = importlib.import_module("Test_KITTI")
    assert te.parser.parse_args([]).view_metrics is False
    a = te.parser.parse_args(["--view-metrics", "--synthetic", "--device-metrics"])
    assert a.view_metrics is True and a.synthetic and a.device_metrics
    src = open(os.path.join(ROOT, "Test_KITTI.py")).read()
    assert re.search(r"if args\.view_metrics:\s+products\.append\(inference\.ViewMetrics\(", src)  # the switch is what puts the product into the run


def test_stage2_refuses_the_ssim_term():
    """A masked SSIM is not built: Train_Stage2_K.py stops at its command line, before anything touches a GPU."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "Train_Stage2_K.py"), "--synthetic", "--a_ssim", "0.1"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "a_ssim" in r.stderr and "Stage 2" in r.stderr and "Traceback" not in r.stderr
