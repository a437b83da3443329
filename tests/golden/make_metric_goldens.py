#!/usr/bin/env python3
"""Generates tests/golden/metrics_make3d.npz by IMPORTING the reference's myUtils from the path given on the command line: the Make3D metric
pair (disps_to_depths_make, compute_make_errors) on a seeded 3 x 1242 strip.  Nothing of the reference is copied; the file holds the input
arrays and what the reference's functions returned for them.  usage: python tests/golden/make_metric_goldens.py [--ref /root/reference]

  pred    (3, 1242) f32  predicted disparity, some values <= 0 (they take the d + 1 denominator)
  gt      (3, 1242) f32  ground-truth depth: ~30 % of the pixels non-zero, a few at or beyond the 70 m cap (masked out)
  gt_depth, pred_depth   what disps_to_depths_make([gt], [pred]) returned (masked 1-d arrays, median-scaled, capped)
  errors  (7,) f64       compute_make_errors(gt_depth, pred_depth): abs_rel, sq_rel, rms, log10, a1, a2, a3"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def seeded_frame(seed=6, shape=(3, 1242)):
    rng = np.random.default_rng(seed)
    pred = (rng.random(shape) ** 2 * 90 + 0.5).astype(np.float32)
    depth = 721 * 0.22 / pred.astype(np.float64)
    gt = (1.3 * depth * (1 + 0.2 * rng.standard_normal(shape))).astype(np.float32)
    gt[rng.random(shape) < 0.7] = 0
    gt[0, :40:7] = 70 + np.arange(6, dtype=np.float32)  # at and beyond the cap
    pred[1, 5:60:9] = np.float32(-0.25)  # <= 0: denominator d + 1
    pred[2, 3] = 0
    return pred, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import myUtils as ref_utils  # noqa: E402
    assert os.path.abspath(ref_utils.__file__).startswith(os.path.abspath(args.ref)), ref_utils.__file__
    pred, gt = seeded_frame()
    gd, pd = ref_utils.disps_to_depths_make([gt.copy()], [pred.copy()])
    errors = np.array(ref_utils.compute_make_errors(gd[0], pd[0]), np.float64)
    np.savez_compressed(os.path.join(HERE, "metrics_make3d.npz"), pred=pred, gt=gt, gt_depth=gd[0], pred_depth=pd[0], errors=errors)
    print("selected", len(gd[0]), "of", gt.size, "dtypes", gd[0].dtype, pd[0].dtype, "errors", errors)


if __name__ == "__main__":
    main()
