#!/usr/bin/env python3
"""Write the original Eigen split's ready-made ground truth: for every line of the list, project the frame's raw Velodyne scan into the left
camera on the device (fal_net_amd/velodyne.py) at the image's own size and save it as `<frame>.npy` beside the image -- the file the reference's
loader reads (Datasets/Kitti_eigen_test_original.py:34, listdataset_test.py:49-51), which it otherwise leaves to Monodepth's generate_depth_map.
After this, `Test_KITTI.py -tn Kitti_eigen_test_original` runs without --velodyne-root, and so does the reference itself.

usage: python tools/project_velodyne.py --list Datasets/kitti_eigen_test_original.txt --root <data>/Kitti_eigen_test_original --velodyne-root <raw KITTI> [--cam 2]
(on an MI355X; one JSON line {'written', 'skipped'})"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from fal_net_amd import datasets as DS  # noqa: E402
from fal_net_amd import velodyne  # noqa: E402


def write_depth_maps(list_file, root, velodyne_root, cam=2, device="cuda", log=None):
    """-> (paths written, number of list lines skipped because the image, the scan or a calibration file is missing)"""
    with open(list_file) as f:
        n_lines = sum(1 for ln in f.read().splitlines() if len(ln.split()) >= 2)
    triples = DS.eigen_original_triples(list_file, root, velodyne_root)
    P, written = {}, []
    for left, _, ref in triples:
        if ref.calib_dir not in P:
            P[ref.calib_dir] = velodyne.projection_matrix(ref.calib_dir, cam)
        H, W = DS._frame_size(os.path.join(root, left))
        points = torch.from_numpy(velodyne.load_scan(ref.scan)).to(device)
        depth = velodyne.project(points, P[ref.calib_dir], H, W).cpu().numpy()
        out = os.path.join(root, os.path.splitext(left)[0] + ".npy")
        np.save(out, depth)
        written.append(out)
        if log is not None:
            log("{}: {} points -> {} of {} x {} pixels".format(out, points.shape[0], int((depth > 0).sum()), H, W))
    return written, n_lines - len(triples)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--list", required=True, help="the split's list: one 'left right' line per frame, relative to --root")
    p.add_argument("--root", required=True, help="where the images are (<data>/Kitti_eigen_test_original); the .npy files go beside them")
    p.add_argument("--velodyne-root", required=True, help="the raw KITTI tree: <DIR>/<date>/<drive>/velodyne_points/data/<frame>.bin, <DIR>/<date>/calib_*.txt")
    p.add_argument("--cam", type=int, default=2, choices=[2, 3])
    p.add_argument("--verbose", action="store_true")
    a = p.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X (the projection has no CPU fallback)"
    written, skipped = write_depth_maps(a.list, a.root, a.velodyne_root, a.cam, log=print if a.verbose else None)
    print(json.dumps({"written": len(written), "skipped": skipped}))


if __name__ == "__main__":
    main()
