"""The evaluator's per-frame product protocol on the host: inference.Frame / run_products / evaluate(products=...), how many forwards each product's
frame(f) makes (the device work behind it replaced by counting stubs), and Test_KITTI.py's family table, settings filter and comma-list type."""
import argparse
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import Test_KITTI as T  # noqa: E402
from fal_net_amd import confidence, dumps, freeview, inference, mesh, pseudo_lidar, sparsification, views  # noqa: E402

REMOVED = ("writer", "sweep_writer", "sweep_fractions", "stats_writer", "lidar_writer", "mesh_writer", "freeview_writer", "freeview_poses",
           "freeview_fill", "sparsification", "view_metrics")
H, W = 4, 6


class Model:
    """Counts its forwards; returns as many maps as the switches ask for."""

    def __init__(self):
        self.calls = []

    def __call__(self, left, mn, mx, ret_disp=True, ret_subocc=False, ret_pan=False):
        self.calls.append((ret_subocc, ret_pan))
        z = torch.zeros(1, 1, H, W)
        return [z] * (1 + int(ret_pan) + 2 * int(ret_subocc)) if ret_pan or ret_subocc else z

    def _plan(self, B, h, w, device):
        return argparse.Namespace(buf={"dlog0": torch.zeros(1, 7, h, w)})


def make_frame(model=None, **kw):
    return inference.Frame(3, model or Model(), torch.zeros(1, 3, H, W), torch.ones(1, 1, H, W), 2.0, 300.0, **kw)


@pytest.fixture
def from_model(monkeypatch):
    calls = []

    def stub(model, left, mn, mx, which):
        calls.append(tuple(which))
        return {k: "map of " + k for k in which}, None
    monkeypatch.setattr(confidence, "from_model", stub)
    return calls


def test_frame_holds_what_it_was_given_and_caches_nothing(from_model):
    f = make_frame(right="R", target="T", mode="kitti2015", use_median=True)
    assert (f.index, f.right, f.target, f.mode, f.use_median, f.min_disp, f.max_disp) == (3, "R", "T", "kitti2015", True, 2.0, 300.0)
    g = make_frame()
    assert (g.right, g.target, g.mode, g.use_median) == (None, None, "eigen", False)
    assert f.stats(("std", "conf")) == {"std": "map of std", "conf": "map of conf"} and f.conf() == "map of conf" and f.conf() == "map of conf"
    assert from_model == [("std", "conf"), ("conf",), ("conf",)]  # every call is one forward


def test_run_products_calls_each_once_in_list_order_with_the_same_frame():
    seen = []

    class Stub:
        def __init__(self, name):
            self.name = name

        def frame(self, f):
            seen.append((self.name, f))
    f = make_frame()
    inference.run_products([Stub(k) for k in "cab"], f)
    assert seen == [("c", f), ("a", f), ("b", f)]
    inference.run_products((), f)
    assert len(seen) == 3


def test_evaluate_signature():
    p = inspect.signature(inference.evaluate).parameters
    assert p["products"].default == () and not set(REMOVED) & set(p)
    for name, default in (("device_metrics", False), ("device_percentile", False), ("disparity", "mean"), ("post", "ms_pp"), ("use_median", False),
                          ("with_metrics", True)):
        assert p[name].default == default, name
    assert not [n for n in dir(inference) if n.endswith("_frame")]
    for cls in (dumps.FrameWriter, dumps.SweepWriter, freeview.FreeviewWriter, confidence.StatsWriter, pseudo_lidar.PseudoLidarWriter, mesh.MeshWriter,
                sparsification.SparsificationTable, inference.ViewMetrics):
        assert callable(cls.frame) and isinstance(cls.key, str), cls
    assert [c.key for c in (sparsification.SparsificationTable, inference.ViewMetrics)] == ["sparsification", "view"]
    assert all(callable(c.result) for c in (sparsification.SparsificationTable, inference.ViewMetrics))


@pytest.mark.parametrize("min_conf", [None, 0.5])
def test_lidar_and_mesh_ask_for_the_confidence_only_when_they_filter(tmp_path, monkeypatch, from_model, min_conf):
    built = []
    monkeypatch.setattr(pseudo_lidar, "unproject", lambda disp, P, **kw: built.append(("lidar", kw["score"])) or np.zeros((0, 4), np.float32))
    monkeypatch.setattr(mesh, "build", lambda left, disp, focal, baseline, **kw: built.append(("mesh", kw["score"])) or (
        [(np.zeros((0, 15), np.uint8), np.zeros((0, 13), np.uint8))], [(0, 0)]))
    asked = []
    lw = pseudo_lidar.PseudoLidarWriter(str(tmp_path), lambda i, h, w: asked.append((i, h, w)) or ("P", 100.0), min_conf=min_conf, extra={"calibration": "x"})
    mw = mesh.MeshWriter(str(tmp_path), min_conf=min_conf)
    conf = None if min_conf is None else "map of conf"
    lw.frame(make_frame())
    assert from_model == ([] if min_conf is None else [("conf",)]) and asked == [(3, H, W)] and built == [("lidar", conf)]
    mw.frame(make_frame())
    assert from_model == ([] if min_conf is None else [("conf",)] * 2) and built == [("lidar", conf), ("mesh", conf)]
    assert os.path.isfile(lw.file(3)) and os.path.isfile(mw.file(3)) and lw.frames == mw.frames == 1
    assert list(lw.summary())[-1] == "calibration" and lw.summary()["calibration"] == "x" and mw.summary()["frames"] == 1


def test_frame_goes_through_the_instances_write(tmp_path, monkeypatch, from_model):
    """A wrapper put around write() -- on the class, as the tests' recording helpers do, or on one writer -- sees every frame."""
    monkeypatch.setattr(pseudo_lidar.PseudoLidarWriter, "write", lambda self, i, disp, P, fb, conf=None: seen.append(("lidar", i, P, fb, conf)))
    monkeypatch.setattr(mesh.MeshWriter, "write", lambda self, i, left, disp, conf=None: seen.append(("mesh", i, conf)))
    seen = []
    pseudo_lidar.PseudoLidarWriter(str(tmp_path), lambda i, h, w: ("P", 1.0)).frame(make_frame())
    mesh.MeshWriter(str(tmp_path), min_conf=0.25).frame(make_frame())
    assert seen == [("lidar", 3, "P", 1.0, None), ("mesh", 3, "map of conf")]


def test_sparsification_passes_over_a_frame_without_ground_truth(monkeypatch, from_model):
    table = object.__new__(sparsification.SparsificationTable)  # the table itself lives on the device
    table.names, table.steps, table.n = ["std", "relstd"], 5, 0
    curves = []
    monkeypatch.setattr(sparsification, "curves", lambda *a, **kw: curves.append((a, kw)))
    monkeypatch.setattr(sparsification, "score_maps", lambda st, names: {k: (k, 1) for k in names})
    table.row = lambda i: ("row", i)
    model = Model()
    table.frame(make_frame(model))
    assert from_model == [] and curves == [] and model.calls == []
    f = make_frame(model, target="gt", mode="kitti2015", use_median=True)
    table.frame(f)
    assert from_model == [("mean", "std")] and len(curves) == 1 and model.calls == []
    (a, kw), = curves
    assert a[0] is f.disp and a[1:3] == ("gt", "kitti2015") and list(a[3]) == ["std", "relstd"] and kw == {"use_median": True, "steps": 5, "out": ("row", 0)}


def test_forwards_of_the_other_products(tmp_path, monkeypatch, from_model):
    renders, written = [], []
    monkeypatch.setattr(dumps, "local_normalization", lambda x: x)
    monkeypatch.setattr(views, "render", lambda model, left, mn, mx, ts: renders.append(("sweep", list(ts))) or (
        torch.zeros(1, len(ts), 3, H, W), torch.zeros(1, len(ts), 1, H, W), None))
    monkeypatch.setattr(freeview, "render", lambda model, left, mn, mx, poses, want, fill: renders.append(("freeview", len(poses), want, fill)) or (
        {"view": "V", "cover": "C", "view_filled": "F"}, None))
    model = Model()
    # dump: no forward unless the view or the masks are wanted, then one with both
    for what, calls in ((("disp", "input", "pc"), []), (("pan",), [(True, True)]), (("disp", "feats"), [(True, True)])):
        w = dumps.FrameWriter(str(tmp_path), what)
        w.write = lambda i, left, disp, pan=None, feats=None: written.append(("dump", i, pan is not None, None if feats is None else len(feats)))
        model.calls = []
        w.frame(make_frame(model))
        assert model.calls == calls and written.pop() == ("dump", 3, bool(calls), 3 if calls else None), what
    model.calls = []
    # sweep: one render; t = 1 is appended for the right view's disparity and not written as a view
    w = dumps.SweepWriter(str(tmp_path), [0.0, 0.5], extra={"views": 2, "range": [0.0, 0.5]})
    w.write = lambda i, imgs, right_disp=None: written.append(("sweep", i, imgs.shape[1], tuple(right_disp.shape)))
    w.frame(make_frame(model))
    assert renders == [("sweep", [0.0, 0.5, 1.0])] and written.pop() == ("sweep", 3, 2, (1, 1, H, W)) and w.summary() == {"views": 2, "range": [0.0, 0.5], "files": 0}
    # freeview: one render, with the fill only when the writer has a beta
    for beta in (None, 4.0):
        w = freeview.FreeviewWriter(str(tmp_path), freeview.paths.orbit(3, 0.5, 0.25), fill_beta=beta, extra={"poses": 3})
        w.write = lambda i, v, c: written.append(("freeview", i, v, c))
        w.write_filled = lambda i, v: written.append(("filled", i, v))
        del renders[:], written[:]
        w.frame(make_frame(model))
        assert renders == [("freeview", 3, ("view", "cover"), beta)]
        assert written == [("freeview", 3, "V", "C")] + ([("filled", 3, "F")] if beta is not None else [])
        assert list(w.summary()) == ["frames", "files", "mean_cover", "poses"]
    # stats: one forward for everything the writer needs
    w = confidence.StatsWriter(str(tmp_path), ("arg",), pc_min_conf=0.5)
    w.write = lambda i, left, disp, st, n_planes: written.append(("stats", i, sorted(st), n_planes))
    w.frame(make_frame(model))
    assert from_model == [w.which] and written[-1] == ("stats", 3, sorted(w.which), 7)
    # the view metric passes over a frame without a right image, without a forward
    v = object.__new__(inference.ViewMetrics)
    v.frame(make_frame(model))
    assert model.calls == []


def test_one_min_conf_and_one_ply_format_check(tmp_path):
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"thr must lie in \(0, 1\]"):
            confidence.check_min_conf(bad, "thr")
        for make in (lambda: mesh.MeshWriter(str(tmp_path), min_conf=bad), lambda: pseudo_lidar.PseudoLidarWriter(str(tmp_path), min_conf=bad),
                     lambda: confidence.StatsWriter(str(tmp_path), pc_min_conf=bad)):
            with pytest.raises(ValueError, match=r"min_conf must lie in \(0, 1\]"):
                make()
    assert confidence.check_min_conf(None) is None and confidence.check_min_conf(1.0) == 1.0 and confidence.check_min_conf(2.0 ** -20) == 2.0 ** -20
    for name in ("--pc-min-conf", "--pl-min-conf", "--mesh-min-conf"):
        parse = T.parser._option_string_actions[name].type
        assert parse("0.25") == 0.25 and parse("1") == 1.0
        for bad in ("0", "1.5", "nan", "much"):
            with pytest.raises(argparse.ArgumentTypeError):
                parse(bad)
        with pytest.raises(argparse.ArgumentTypeError, match=name + r" must lie in \(0, 1\], got 1.5"):
            parse("1.5")
    dumps.check_ply_format("binary"), dumps.check_ply_format("ascii")
    for call in (lambda: dumps.check_ply_format("obj"), lambda: dumps.FrameWriter(str(tmp_path), (), ply_format="obj"),
                 lambda: dumps.save_ply(str(tmp_path / "a.ply"), planar=np.zeros((6, 0)), ply_format="obj"),
                 lambda: mesh.MeshWriter(str(tmp_path), ply_format="obj"),
                 lambda: mesh.save_ply(str(tmp_path / "b.ply"), np.zeros((0, 15), np.uint8), np.zeros((0, 13), np.uint8), ply_format="obj")):
        with pytest.raises(ValueError, match="ply_format must be 'binary' or 'ascii', got 'obj'"):
            call()


def test_one_ply_header():
    cloud = dumps._ply_header("ascii", 5)
    assert cloud == ("ply\nformat ascii 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
                     "property uchar diffuse_red\nproperty uchar diffuse_green\nproperty uchar diffuse_blue\nend_header\n")
    full = dumps._ply_header("binary_little_endian", 5, normals=True, faces=2)
    assert full == ("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
                    "property float nx\nproperty float ny\nproperty float nz\n"
                    "property uchar diffuse_red\nproperty uchar diffuse_green\nproperty uchar diffuse_blue\n"
                    "element face 2\nproperty list uchar int vertex_indices\nend_header\n")
    assert not hasattr(mesh, "_ply_header") or mesh._ply_header is dumps._ply_header


# ---- Test_KITTI.py ------------------------------------------------------------------------------------------------------------------------------------
SWITCH_ON = {"--sweep": ["--sweep", "2"], "--stats": ["--stats", "std"], "--pseudo-lidar": ["--pseudo-lidar"], "--mesh": ["--mesh"],
             "--sparsification": ["--sparsification", "std"], "--freeview": ["--freeview", "2"], "--freeview-fill": ["--freeview-fill"]}
VALUE = {"pl_beams": ["8"], "pl_az_bins": ["512"], "pl_max_depth": ["60"], "pl_max_height": ["2"], "pl_min_conf": ["0.5"], "pl_calib": ["/calib"],
         "mesh_max_jump": ["0.1"], "mesh_max_depth": ["60"], "mesh_min_conf": ["0.5"], "mesh_normals": [], "sparsification_steps": ["20"],
         "sweep_range": ["0", "1"], "freeview_path": ["dolly"], "freeview_amp": ["1", "1", "1"], "freeview_yaw": ["5"]}


def test_family_table():
    parse = T.parser.parse_args
    assert [f[0] for f in T.FAMILIES] == list(SWITCH_ON)
    assert {f[0] for f in T.FAMILIES if f[3]} == {"--pseudo-lidar", "--mesh", "--sparsification"}
    by_switch = {f[0]: f[1] for f in T.FAMILIES}
    assert (by_switch["--pseudo-lidar"], by_switch["--mesh"], by_switch["--sparsification"], by_switch["--freeview"], by_switch["--freeview-fill"]) == (
        T.LIDAR_ARGS, T.MESH_ARGS, T.SPARSIFICATION_ARGS, T.FREEVIEW_ARGS, T.FREEVIEW_FILL_ARGS)
    everything = set(T.LIDAR_ARGS + T.MESH_ARGS + T.SPARSIFICATION_ARGS + T.FREEVIEW_ARGS + T.FREEVIEW_FILL_ARGS) | {
        "sweep", "sweep_range", "stats", "pc_min_conf", "disparity"}
    hidden = T.hidden_settings(parse([]))
    assert set(hidden) == everything and len(hidden) == len(everything) and everything <= set(vars(parse([])))
    T.check_family_args(parse([]))
    for switch, names, on, strict in T.FAMILIES:
        assert not on(parse([])) and on(parse(SWITCH_ON[switch]))
        assert set(T.hidden_settings(parse(SWITCH_ON[switch]))) == everything - set(names), switch  # exactly its names come back
        T.check_family_args(parse(SWITCH_ON[switch]))
        for n in names[1:]:
            alone = ["--" + n.replace("_", "-")] + VALUE[n] if n in VALUE else None
            if strict:
                with pytest.raises(SystemExit) as e:
                    T.check_family_args(parse(alone))
                assert "{} {} a parameter of {}: add {}".format(alone[0], "sets" if len(names) == 2 else "set(s)", switch, switch) == str(e.value)
                T.check_family_args(parse(SWITCH_ON[switch] + alone))
            elif alone is not None:
                T.check_family_args(parse(alone))  # accepted in silence, as before
    # the stats family is on with any of its three switches
    for on in (["--pc-min-conf", "0.5"], ["--disparity", "peak"]):
        assert set(T.hidden_settings(parse(on))) == everything - set(by_switch["--stats"])
    with pytest.raises(SystemExit, match="--pl-beams, --pl-calib set\\(s\\) a parameter of --pseudo-lidar: add --pseudo-lidar"):
        T.check_family_args(parse(["--pl-calib", "/c", "--pl-beams", "8", "--mesh"]))
    with pytest.raises(SystemExit, match="--pl-max-height is not a number"):
        T.check_family_args(parse(["--pseudo-lidar", "--pl-max-height", "nan"]))


def test_comma_lists():
    dump, stats, spars = (T.parser._option_string_actions[k].type for k in ("--dump", "--stats", "--sparsification"))
    assert dump("disp,pc") == ["disp", "pc"] and dump("feats,,disp,") == ["feats", "disp"] and dump("") == [] and dump("pc,pc") == ["pc", "pc"]
    with pytest.raises(argparse.ArgumentTypeError) as e:
        dump("disp,mesh,depth")
    assert str(e.value) == "unknown dump kind(s) mesh,depth: choose from disp,input,pan,pc,feats"
    assert T.DUMP_KINDS == dumps.DUMP_KINDS and T.STATS_KINDS == confidence.StatsWriter.CLI_KINDS and T.SPARSIFICATION_SCORES == tuple(sparsification.SCORES)
    for parse, name, choices in ((stats, "--stats", "std,entropy,arg,conf,peak"), (spars, "--sparsification", "std,entropy,conf,relstd")):
        assert parse("conf,std") == ["conf", "std"] and parse(choices) == choices.split(",") and parse("std,") == ["std"]
        for bad in ("", ",", "std,std", "mean", "std,depth"):
            with pytest.raises(argparse.ArgumentTypeError) as e:
                parse(bad)
            assert str(e.value) == "{} takes a comma-separated subset of {} (each once), got {!r}".format(name, choices, bad)
    assert stats("arg,peak") == ["arg", "peak"] and spars("relstd") == ["relstd"]
    for bad, parse in (("relstd", stats), ("arg", spars)):
        with pytest.raises(argparse.ArgumentTypeError):
            parse(bad)


def test_main_names_the_products_only_where_it_builds_them():
    src = open(os.path.join(ROOT, "Test_KITTI.py")).read()
    main = src[src.index("def main():"):]
    for cls in ("FrameWriter", "SweepWriter", "FreeviewWriter", "StatsWriter", "PseudoLidarWriter", "MeshWriter", "SparsificationTable", "ViewMetrics"):
        assert main.count(cls) == 1 and src.count(cls) == 1, cls
    assert "_frame(" not in src and "_writer is not None" not in src and "device_metrics=args.device_metrics" in src
