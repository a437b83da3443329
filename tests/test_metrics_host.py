"""CPU: the host side of the device metrics -- the Make3D metric pair against values recorded from the reference's own functions
(tests/golden/metrics_make3d.npz, written by tests/golden/make_metric_goldens.py), the --device-metrics flag of the four entry scripts, and the
new entry points in the header, the binding and the build list.  No GPU."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def test_make3d_pair_vs_reference_golden(golden_dir):
    """Same numpy, same order of operations: 1e-12 relative on every masked depth and every error."""
    import myUtils as utils  # the root alias exposes the new names
    g = np.load(os.path.join(golden_dir, "metrics_make3d.npz"))
    assert utils.make_error_names == ['abs_rel', 'sq_rel', 'rms', 'log10', 'a1', 'a2', 'a3']
    gd, pd = utils.disps_to_depths_make([g["gt"].copy()], [g["pred"].copy()])
    assert gd[0].shape == g["gt_depth"].shape and gd[0].dtype == g["gt_depth"].dtype and pd[0].dtype == g["pred_depth"].dtype
    assert (g["pred"] <= 0).sum() >= 2 and (g["gt"] >= 70).sum() >= 2  # the fixture exercises the d + 1 denominator and the cap of the mask
    assert _rel(gd[0], g["gt_depth"]) <= 1e-12 and _rel(pd[0], g["pred_depth"]) <= 1e-12
    assert gd[0].max() <= 70 and gd[0].min() >= 1 and pd[0].max() <= 70 and pd[0].min() >= 1
    errs = utils.compute_make_errors(gd[0], pd[0])
    assert len(errs) == 7 and _rel(errs, g["errors"]) <= 1e-12
    # and from the recorded depths alone
    assert _rel(utils.compute_make_errors(g["gt_depth"], g["pred_depth"]), g["errors"]) <= 1e-12


def test_make3d_inputs_are_left_alone(golden_dir):
    g = np.load(os.path.join(golden_dir, "metrics_make3d.npz"))
    gt, pred = g["gt"].copy(), g["pred"].copy()
    from fal_net_amd import myUtils as utils
    utils.disps_to_depths_make([gt], [pred])
    assert np.array_equal(gt, g["gt"]) and np.array_equal(pred, g["pred"])


@pytest.mark.parametrize("script", ["Test_KITTI.py", "Train_Stage1_K.py", "Train_Stage1_Kslow.py", "Train_Stage2_K.py"])
def test_device_metrics_flag_parses_and_defaults_off(script, monkeypatch):
    """--device-metrics on every entry script, off by default (the two derived training scripts share Train_Stage1_K's parser)."""
    monkeypatch.syspath_prepend(ROOT)
    src = open(os.path.join(ROOT, script)).read()
    mod = importlib.import_module("Test_KITTI" if script == "Test_KITTI.py" else "Train_Stage1_K")
    if script in ("Train_Stage1_Kslow.py", "Train_Stage2_K.py"):
        assert "import Train_Stage1_K as base" in src and "base.parser.parse_args()" in src
    assert mod.parser.parse_args([]).device_metrics is False
    assert mod.parser.parse_args(["--device-metrics"]).device_metrics is True
    if script == "Test_KITTI.py":
        a = mod.parser.parse_args(["--device-metrics", "-median", "True", "--device-percentile"])
        assert a.device_metrics and a.median is True and a.device_percentile
        assert "device_metrics=args.device_metrics" in src
    else:
        assert "device_metrics=args.device_metrics" in open(os.path.join(ROOT, "Train_Stage1_K.py")).read()


def test_loops_take_device_metrics_off_by_default():
    import inspect
    from fal_net_amd import inference, train
    assert inspect.signature(inference.evaluate).parameters["device_metrics"].default is False
    assert inspect.signature(train.validate).parameters["device_metrics"].default is False


NEW = ("falnet_metrics_workspace_bytes", "falnet_depth_median_scale", "falnet_depth_errors", "falnet_epe", "falnet_view_errors")


def test_entry_points_in_header_binding_and_build():
    from fal_net_amd import _build, _lib, ops
    hdr = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)), name
        assert name in _lib.SIGNATURES and name in doc
    assert _lib.SIGNATURES["falnet_depth_errors"][-1] is _lib.C.c_void_p and _lib._RESTYPES["falnet_metrics_workspace_bytes"] is _lib.C.c_int64
    assert "metrics.hip" in _build.SOURCES and _build.FILE_FLAGS["metrics.hip"] == ["-ffp-contract=off"]
    assert "metrics.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600  # the packaged autotune cache stays valid


def test_python_surface_and_columns():
    from fal_net_amd import metrics as M
    hdr = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    cols = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define FALNET_MET_([A-Z0-9_]+) (\d+)", hdr)}
    assert cols.pop("row") == M.ROW == len(M.COLUMNS)
    cols["log_rms"] = cols.pop("log")
    assert cols == {k: v for k, v in M.COL.items() if k != "reserved"}  # the Python column names are the header's
    for mode, code in M.MODES.items():
        assert re.search(r"#define FALNET_DEPTH_%s %d\b" % (mode.upper(), code), hdr)
    from fal_net_amd import myUtils as utils
    assert M.focal_baseline("kitti2015", 1242) == utils.width_to_focal[1242] * 0.54
    assert M.focal_baseline("eigen", 1226) == utils.width_to_focal[1226] * utils.width_to_baseline[1226]
    assert M.focal_baseline("make3d", 999) == 721 * 0.22
    with pytest.raises(KeyError):  # a width outside the calibration table, as in the host chain
        M.focal_baseline("eigen", 1000)
    with pytest.raises(ValueError):
        M.focal_baseline("cityscapes", 1242)
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # never a quiet host path
        M.depth_errors(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), "kitti2015")
