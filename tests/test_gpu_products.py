"""The property the evaluator's product protocol relies on (inference.run_products): a product's files and its JSON line do not depend on which
other products run beside it, nor on their order.  One child process runs Test_KITTI.py's main() with every product on and then with each one
alone (tests/_products_cli.py)."""
import filecmp
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BASE = ["--synthetic", "--height", "64", "--width", "128", "--iters", "1", "-no_levels", "7", "-mspp", "False"]
ALONE = {  # product -> (its switches, the key of its JSON line, the folders its files go to)
    "dump": (["--dump", "disp,input,pan,pc,feats"], None, ("l_disp", "Input im", "Pan", "Point_cloud", "feats")),
    "sweep": (["--sweep", "2"], "sweep", ("Sweep", "r_disp")),
    "freeview": (["--freeview", "2", "--freeview-fill"], "freeview", ("Freeview",)),
    "stats": (["--stats", "std,entropy,arg,conf,peak"], "stats", ("stats",)),
    "lidar": (["--pseudo-lidar", "--pl-min-conf", "0.3"], "pseudo_lidar", ("Pseudo_lidar",)),
    "mesh": (["--mesh", "--mesh-min-conf", "0.3"], "mesh", ("Mesh",)),
    "view": (["--view-metrics"], "view", ()),
}


def files_under(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs)


def test_products_do_not_depend_on_each_other(tmp_path):
    runs = {"all": BASE + [a for switches, _, _ in ALONE.values() for a in switches]}
    runs.update({name: BASE + switches for name, (switches, _, _) in ALONE.items()})
    spec = tmp_path / "runs.json"
    spec.write_text(json.dumps(runs))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_products_cli.py"), str(tmp_path), str(spec)], cwd=ROOT,
                       env=dict(os.environ, FALNET_DETERMINISTIC="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]

    def lines(name):  # the run's JSON lines by their first key, the save path taken out
        text = (tmp_path / (name + ".stdout")).read_text().replace(str(tmp_path / name), "<save>")
        return {next(iter(d)): d for d in (json.loads(ln) for ln in text.splitlines() if ln.startswith("{"))}

    everything, all_files = lines("all"), files_under(tmp_path / "all")
    assert list(everything) == ["view", "pseudo_lidar", "mesh", "sweep", "freeview", "stats", "image"]  # the order the lines are printed in
    claimed = []
    for name, (_, key, folders) in ALONE.items():
        mine = files_under(tmp_path / name)
        if name == "view":
            assert mine == ["view_errors.txt"]
        else:
            assert mine and {f.split(os.sep)[0] for f in mine} == set(folders), (name, mine)
        match, mismatch, errors = filecmp.cmpfiles(tmp_path / "all", tmp_path / name, mine, shallow=False)
        assert (sorted(match), mismatch, errors) == (mine, [], []), name  # every file of the run alone is, byte for byte, the file of the run with all
        claimed += mine
        alone = lines(name)
        assert list(alone) == ([key] if key else []) + ["image"], name
        if key:
            assert alone[key] == everything[key] and alone[key][key], name
    assert sorted(claimed) == all_files  # and the run with all of them writes nothing else
