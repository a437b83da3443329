"""Helper of tests/test_gpu_velo.py (run as a FALNET_DETERMINISTIC=1 process, so that two forwards of one frame give the same disparities and what
differs between two evaluations is the ground truth's route alone): builds a one-frame raw-KITTI tree and its image tree under the directory
given on the command line, writes the frame's `.npy` with tools/project_velodyne.py's function, and runs inference.evaluate over the `.npy` layout
and over the scan layout, each with the host metrics and with device_metrics=True -> one JSON line
{'npy': {'host', 'device'}, 'scan': {'host', 'device'}, 'npy_equals_spec', 'valid_pixels'}."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _velo_ref as R  # noqa: E402
import project_velodyne  # noqa: E402
from fal_net_amd import datasets as DS  # noqa: E402
from fal_net_amd import inference, synthetic  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402

H, W, N_POINTS = 375, 1242, 120000


def main():
    from PIL import Image
    tmp = sys.argv[1]
    root, raw = os.path.join(tmp, "Kitti_eigen_test_original"), os.path.join(tmp, "raw")
    drive, frame = "2011_09_26_drive_0002_sync", "0000000069"
    rng = np.random.default_rng(11)
    for cam in ("_02", "_03"):
        os.makedirs(os.path.join(root, drive + cam))
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, drive + cam, frame + ".jpg"))
    scan_dir = os.path.join(raw, "2011_09_26", drive, "velodyne_points", "data")
    os.makedirs(scan_dir)
    points = R.seeded_scan(4, N_POINTS)
    points.tofile(os.path.join(scan_dir, frame + ".bin"))
    R.write_calib(os.path.join(raw, "2011_09_26"))
    lst = os.path.join(tmp, "list.txt")
    with open(lst, "w") as f:
        f.write(f"{drive}_02/{frame}.jpg {drive}_03/{frame}.jpg\n")

    written, skipped = project_velodyne.write_depth_maps(lst, root, raw)
    assert written == [os.path.join(root, drive + "_02", frame + ".npy")] and skipped == 0, (written, skipped)
    npy = np.load(written[0])
    want = R.spec(R.compose_P(), points, H, W)

    model = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(49)}, 49, compute_dtype=torch.float16).to("cuda").eval()
    out = {"npy_equals_spec": bool(npy.dtype == np.float32 and np.array_equal(npy, want)), "valid_pixels": int((npy > 0).sum())}
    for layout, vroot in (("npy", None), ("scan", raw)):
        triples = DS.eigen_original_triples(lst, root, vroot)
        assert len(triples) == 1, triples
        out[layout] = {}
        for name, flag in (("host", False), ("device", True)):
            loader = DS.make_loader(DS.StereoEvalDataset(root, triples), 1, 0, shuffle=False, drop_last=False)
            res = inference.evaluate(model, loader, data_name="Kitti_eigen_test_original", post="none", log=None, device_metrics=flag)
            assert res["n"] == 1 and res["epe"] == 0
            out[layout][name] = res["kitti"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
