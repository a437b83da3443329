"""Helper of tests/test_gpu_wgrad.py::test_deterministic_mode_child (run as a subprocess with FALNET_DETERMINISTIC=1: the switch is read
when the library is loaded).  In deterministic mode:
  * one case per weight-gradient kernel (tests/_wgrad_cases.py: DET_CASES) gives the same integers as the normal run -- run_case
    asserts them, slabs, both reduce modes (single writer per element) -- and no kernel fuses the bias gradient;
  * variant 6 takes the patch form even for an aligned image whose width is a multiple of 4;
  * falnet_bias_grad_batched is refused; falnet_bias_grad_batched_det and falnet_wgrad_reduce_batched with groups 1 give the integers."""
import ctypes as C
import json
import os
import sys

os.environ["FALNET_DETERMINISTIC"] = "1"
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from fal_net_amd import _lib as L  # noqa: E402

import _wgrad_cases as K  # noqa: E402
import test_gpu_wgrad as T  # noqa: E402

DEV = "cuda"


def main():
    lib = L.lib()
    assert lib.falnet_get_deterministic() == 1
    ncases, fused, kernels = 0, 0, set()
    for name in K.DET_CASES:
        case = K.BY_NAME[name]
        nsplit = [s for s in K.split_counts(case) if s != K.PLAN][1]
        for dtype in case["dtypes"]:
            out = K.run_case(case, dtype, nsplit, DEV)
            fused += out["fuses_bias"]
            ncases += 1
        kernels.add(case["kernel"])
    wave = K.BY_NAME["c3_wave_16x64"]
    form = K.c3_form(wave, K.run_case(wave, torch.bfloat16, 20, DEV), 20)
    variant, _ = K.planned(wave, torch.bfloat16, DEV)
    assert variant == 6
    # the batched tables, groups 1
    entries = [e[:8] + (1,) for e in T.REDUCE_ENTRIES]
    for accumulate in (0, 1):
        t = T.reduce_table(entries, DEV, accumulate)
        L.check(lib.falnet_wgrad_reduce_batched(L.ptr(t["table"]), t["n"], t["blocks"], accumulate, L.stream_ptr()), "wgrad_reduce_batched")
        flat = t["flat"].to(torch.float64)
        for (o, n, _), ref in zip(t["spans"], t["refs"]):
            msg = K._first_bad(flat[o:o + n], ref + (7.0 if accumulate else 0.0))
            assert msg is None, msg
    t = T.bias_table(T.BIAS_ENTRIES, torch.bfloat16, DEV, 3.0)
    refused = int(lib.falnet_bias_grad_batched(L.ptr(t["table"]), t["n"], t["blocks"], L.dtype_code(torch.bfloat16), L.stream_ptr()) != 0)
    ws = torch.full((512 * t["blocks"],), float("nan"), device=DEV)
    L.check(lib.falnet_bias_grad_batched_det(L.ptr(t["table"]), t["n"], t["blocks"], L.dtype_code(torch.bfloat16), L.ptr(ws), ws.numel(), L.stream_ptr()),
            "bias_grad_batched_det")
    T.check_bias(t, T.BIAS_ENTRIES, 3.0)
    torch.cuda.synchronize()
    print(json.dumps({"deterministic": 1, "cases": ncases, "kernels": sorted(kernels), "fused_bias": fused, "bias_grad_batched_refused": refused,
                      "c3_form": form, "reduce_entries": len(entries), "bias_entries": len(T.BIAS_ENTRIES)}), flush=True)


if __name__ == "__main__":
    main()
