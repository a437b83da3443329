#!/usr/bin/env python3
"""Coefficients of the free-viewpoint plane sweep (csrc/med_pose.hip) against the float64 reference of tests/_freeview_ref.py on an MI355X: for
every listed (case, pose set), its logit families and seeds 0, 1, 2 the worst (|got - ref| - u |ref| - eta) / mag of every pose's view, disparity
and cover, one line each, then the worst per (output, disparity class) with _head_ref.round_up_coef of it -- what tests/_freeview_ref.COEF
records.  The pure-baseline poses (set S and pose 1 of F / N9) are also listed apart, beside _sweep_ref.COEF of the same class.
usage: python tools/measure_freeview.py [out.txt]   (profiles/freeview_vs_f64.txt)"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from fal_net_amd import _lib as L  # noqa: E402
import _head_ref as R  # noqa: E402
import _sweep_ref as S  # noqa: E402
import _freeview_ref as F  # noqa: E402


def launch(inp, poses):
    """One launch per 8 poses from NaN-filled outputs -> dict of CPU tensors."""
    d0, lf, mn, mx = (inp[k].contiguous().cuda() for k in ("dlog0", "left", "mn", "mx"))
    B, N, H, W = d0.shape
    parts = {"view": [], "disp": [], "cover": []}
    for v0 in range(0, len(poses), 8):
        rec = np.ascontiguousarray(np.stack(poses[v0:v0 + 8]).astype(np.float64))
        n = len(rec)
        out = {"view": torch.full((B, n, 3, H, W), float("nan"), device="cuda"), "disp": torch.full((B, n, 1, H, W), float("nan"), device="cuda"),
               "cover": torch.full((B, n, 1, H, W), float("nan"), device="cuda")}
        L.check(L.lib().falnet_med_pose_fwd(L.ptr(d0), L.ptr(lf), L.ptr(mn), L.ptr(mx), rec.ctypes.data_as(ctypes.c_void_p), n, L.ptr(out["view"]),
                                            L.ptr(out["disp"]), L.ptr(out["cover"]), B, N, H, W, L.stream_ptr()), "med_pose_fwd")
        torch.cuda.synchronize()
        for k in parts:
            parts[k].append(out[k].cpu())
    return {k: torch.cat(v, 1) for k, v in parts.items()}


def is_baseline(pose):
    return bool((pose[:9] == np.eye(3).reshape(9)).all()) and pose[10] == 0.0 and pose[11] == 0.0 and pose[9] != 0.0


def main():
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "freeview_vs_f64.txt"), "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    emit("# free-viewpoint plane sweep vs float64 (tests/_freeview_ref.py): coefficient needed = worst (|got - ref| - u |ref| - eta) / mag; " + torch.cuda.get_device_name(0))
    emit("# case set family seed output pose coef max-norm-error non-finite")
    worst, worst_s = {}, {}
    for case in F.CASES:
        cls = R.disp_class(case)
        K = F.case_camera(case)
        for name in F.SET_NAMES:
            poses = F.pose_set(case, name)
            for family in F.families(case):
                for seed in (0, 1, 2):
                    inp = R.make_inputs(case, family, seed)
                    ref = F.reference(inp, poses, K)
                    got = launch(inp, poses)
                    for what, v, r in F.compare_outputs(case, got, ref, coefs={"view": 0.0, "disp": 0.0, "cover": 0.0}):
                        nonfinite = int((~torch.isfinite(got[what][:, v])).sum())
                        emit(f"{case} {name} {family} {seed} {what} {v} {r['coef']:.4g} {r['maxnorm']:.4g} {nonfinite}")
                        for table, use in ((worst, True), (worst_s, is_baseline(poses[v]))):
                            key = (what, cls)
                            if use and (key not in table or r["coef"] > table[key][0]):
                                table[key] = (r["coef"], f"{case} {name} {family} seed {seed}, pose {v}")
    emit("# worst per (output, class) and round_up_coef (4 x, up to a power of two)")
    for (what, cls), (c, where) in sorted(worst.items()):
        held = R.round_up_coef(c) if c > 0 else 0.0
        emit(f"{what:6s} {cls:5s} worst {c:.3e}  {where}  -> 2^{np.log2(held) if held else float('-inf'):.0f} = {held:.3e}")
    emit("# the pure-baseline poses alone, beside _sweep_ref.COEF of the class (view: the views with t != 1)")
    for (what, cls), (c, where) in sorted(worst_s.items()):
        if what in S.COEF:
            emit(f"{what:6s} {cls:5s} worst {c:.3e}  {where}  (sweep: {S.COEF[what][cls]:.3e})")


if __name__ == "__main__":
    main()
