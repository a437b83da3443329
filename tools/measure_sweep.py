#!/usr/bin/env python3
"""Coefficients of the baseline sweep (csrc/med_sweep.hip) against the float64 reference of tests/_sweep_ref.py on an MI355X: for every listed
(case, baseline set), its logit families and seeds 0, 1, 2 the worst (|got - ref| - u |ref| - eta) / mag of every view and disparity, one line
each, then the worst per (output, disparity class) with _head_ref.round_up_coef of it -- what tests/_sweep_ref.COEF records.  The t = 1 view
is listed apart (it is held to _head_ref.COEF["p_im0"]); at t = 0 the views are also compared with `left` and the disparity with the forward's.
usage: python tools/measure_sweep.py [out.txt]   (profiles/sweep_vs_f64.txt)"""
import ctypes
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from fal_net_amd import _lib as L  # noqa: E402
import _head_ref as R  # noqa: E402
import _sweep_ref as S  # noqa: E402


def launch(inp, ts):
    d0, lf, mn, mx = (inp[k].contiguous().cuda() for k in ("dlog0", "left", "mn", "mx"))
    B, N, H, W = d0.shape
    views = torch.full((B, len(ts), 3, H, W), float("nan"), device="cuda")
    disps = torch.full((B, len(ts), 1, H, W), float("nan"), device="cuda")
    t_host = (ctypes.c_float * len(ts))(*ts)
    L.check(L.lib().falnet_med_sweep_fwd(L.ptr(d0), L.ptr(lf), L.ptr(mn), L.ptr(mx), ctypes.cast(t_host, ctypes.c_void_p), len(ts), L.ptr(views), L.ptr(disps),
                                         B, N, H, W, L.stream_ptr()), "med_sweep_fwd")
    torch.cuda.synchronize()
    return views.cpu(), disps.cpu()


def main():
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sweep_vs_f64.txt"), "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    emit("# baseline sweep vs float64 (tests/_sweep_ref.py): coefficient needed = worst (|got - ref| - u |ref| - eta) / mag; " + torch.cuda.get_device_name(0))
    emit("# case set family seed output view t coef max-norm-error non-finite")
    worst = {}
    for case, sets in S.CASES.items():
        cls = R.disp_class(case)
        for name in sets:
            ts = S.SETS[name]
            for family in S.families(case):
                for seed in (0, 1, 2):
                    inp = R.make_inputs(case, family, seed)
                    ref = S.reference(inp, ts)
                    views, disps = launch(inp, ts)
                    rows = []
                    for v, t in enumerate(ts):
                        rows.append(("view_t1" if t == 1.0 else "view", v, t, R.compare(views[:, v], ref["view"][:, v], ref["mag_view"][:, v], torch.float32, 0.0)))
                        rows.append(("disp", v, t, R.compare(disps[:, v], ref["disp"][:, v], ref["mag_disp"][:, v], torch.float32, 0.0)))
                    if name == "Z":
                        d64 = S.forward_disp(inp)
                        rows.append(("view", 0, 0.0, R.compare(views[:, 0], inp["left"].double(), ref["mag_view"][:, 0], torch.float32, 0.0)))
                        rows.append(("disp", 0, 0.0, R.compare(disps[:, 0], d64, d64, torch.float32, 0.0)))
                    for what, v, t, r in rows:
                        nonfinite = int((~torch.isfinite(views[:, v] if what.startswith("view") else disps[:, v])).sum())
                        emit(f"{case} {name} {family} {seed} {what} {v} {t} {r['coef']:.4g} {r['maxnorm']:.4g} {nonfinite}")
                        key = (what, cls)
                        if key not in worst or r["coef"] > worst[key][0]:
                            worst[key] = (r["coef"], f"{case} {name} {family} seed {seed}, view {v} (t = {t})")
    emit("# worst per (output, class) and round_up_coef (4 x, up to a power of two); view_t1 is held to _head_ref.COEF['p_im0'] instead")
    for (what, cls), (c, where) in sorted(worst.items()):
        held = R.COEF["p_im0"][cls] if what == "view_t1" else R.round_up_coef(c)
        emit(f"{what:8s} {cls:5s} worst {c:.3e}  {where}  -> 2^{torch.log2(torch.tensor(held)).item():.0f} = {held:.3e}")


if __name__ == "__main__":
    main()
