#!/usr/bin/env python3
"""Coefficients of the distribution statistics (csrc/med_stats.hip) against the float64 reference of tests/_stats_ref.py on an MI355X: for every
listed case, its logit families and seeds 0, 1, 2 the worst (|got - ref| - u |ref| - eta) / mag of every output, one line each, then the worst per
(output, disparity class) beside the DERIVED coefficient the tests hold it to (tests/_stats_ref.coef; nothing here feeds back into it).  arg is
exact: its column counts unequal elements.
usage: python tools/measure_med_stats.py [out.txt]   (profiles/med_stats_vs_f64.txt)"""
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from fal_net_amd import confidence as C  # noqa: E402
import _head_ref as R  # noqa: E402
import _stats_ref as S  # noqa: E402


def main():
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "med_stats_vs_f64.txt"), "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    emit("# MED distribution statistics vs float64 (tests/_stats_ref.py): coefficient needed = worst (|got - ref| - u |ref| - eta) / mag; " + torch.cuda.get_device_name(0))
    emit("# case family seed output coef max-norm-error over-the-bound non-finite")
    worst = {}
    for case, family in S.listed():
        cls = R.disp_class(case)
        for seed in (0, 1, 2):
            inp = S.make_inputs(case, family, seed)
            ref = S.reference(inp)
            got = C.stats(inp["dlog0"].cuda(), inp["mn"].cuda(), inp["mx"].cuda(), S.KINDS)
            got = {k: v.cpu() for k, v in got.items()}
            for k, r in S.compare_all(case, got, ref).items():
                emit(f"{case} {family} {seed} {k} {r['coef']:.4g} {r['maxnorm']:.4g} {r['bad']} {int((~torch.isfinite(got[k])).sum())}")
                key = (k, cls)
                if key not in worst or r["coef"] > worst[key][0]:
                    worst[key] = (r["coef"], f"{case} {family} seed {seed}")
    emit("# worst per (output, class) and the derived coefficient it is held to")
    for (k, cls), (c, where) in sorted(worst.items()):
        held = S.coef(k, (1, 2, 1, 1, 30.0 if cls == "d30" else 300.0))
        emit(f"{k:8s} {cls:5s} worst {c:.3e}  {where}  held to {'equality' if k == 'arg' else format(held, '.3e')}")


if __name__ == "__main__":
    main()
