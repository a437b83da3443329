#!/usr/bin/env python3
"""The background-biased pull-push (csrc/inpaint.hip) against the float64 reference of tests/_inpaint_ref.py on an MI355X: for every case of
tests/test_gpu_inpaint.py the largest |got - ref| / (K (L + 1) 2^-24 M), one line each, then the largest of all.  K is the derived count of
_inpaint_ref.py; these figures only record how much of it the kernels use.
usage: python tools/measure_inpaint.py [out.txt]   (profiles/inpaint_vs_f64.txt)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fal_net_amd import inpaint as IP  # noqa: E402
import _inpaint_ref as R  # noqa: E402

COMBOS = [(4, 1, 4.0), (3, 3, 0.0), (1, 1, 8.0)]  # as tests/test_gpu_inpaint.py


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "inpaint_vs_f64.txt"), "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
    emit(f"# pull-push hole filling vs float64 (tests/_inpaint_ref.py): largest |got - ref| / (K (L + 1) 2^-24 M), K = {R.K}; " + torch.cuda.get_device_name(0))
    cases = [(H, W, C, I, fam, beta) for H, W in R.SHAPES for fam in R.FAMILIES for C, I, beta in COMBOS]
    cases += [(*R.FULL, 4, 1, "wedge", 4.0), (256, 384, 4, 1, "sparse", 4.0), (1030, 1344, 4, 1, "wedge", 4.0)]
    worst = (0.0, None)
    for H, W, C, I, fam, beta in cases:
        inp, ref, M = R.cached(H, W, C, I, fam, 0, beta)
        v, w, g, s = (torch.from_numpy(inp[k]).cuda() for k in ("values", "weight", "guide", "guide_scale"))
        got = IP.fill(v, w, g, s, beta=beta).cpu().numpy().astype(np.float64)
        err = np.abs(got - ref)
        ratio = max((float(err[i].max() / R.bound(H, W, m)) if m > 0 else float(err[i].max() > 0) * float("inf")) if err[i].max() > 0 else 0.0 for i, m in enumerate(M))
        emit(f"{H:5d} x {W:<5d} L={R.levels(H, W):2d} C={C} I={I} beta={beta:g} {fam:10s} max error {err.max():.3g}  ratio {ratio:.3g}")
        if ratio > worst[0]:
            worst = (ratio, (H, W, C, I, fam, beta))
    emit(f"# largest ratio {worst[0]:.3g} at {worst[1]}")


if __name__ == "__main__":
    main()
