"""Helper of tests/test_gpu_conv_budget.py::test_step_is_bit_identical_under_a_label_budget (run as a subprocess: FALNET_DETERMINISTIC and
the experiment switch FALNET_LABEL_WGS are read when the package loads).  argv[1] = the label pass's workgroup budget (0 = off).  Four
fused Stage-1 steps in bf16 at B = 2, 64 x 128 from seeded weights and inputs -- the third and fourth go through falnet_replay -- and one
JSON line: per step the loss bits and digests of the flat gradients, the flat parameters and the disparity, then what the label plan ran."""
import hashlib
import json
import os
import sys

os.environ["FALNET_DETERMINISTIC"] = "1"
os.environ["FALNET_AB"] = "1"
os.environ["FALNET_LABEL_WGS"] = sys.argv[1]
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch  # noqa: E402

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import ops, synthetic, train  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def _persistent_vgg_convs():
    """Deterministic mode replays cached choices and otherwise takes the library's heuristic -- a halo-patch kernel, which has no budget to
    honour -- and the committed cache has no B = 2 entries.  Both runs therefore build the VGG convs on the persistent LDS-DMA kernel the
    benchmark's label pass runs (variant 23) wherever it applies: the same kernels on both sides, only the grid differs."""
    orig = ops.conv_call

    def conv_call(*a, **kw):
        if kw.get("name", "").startswith("vgg conv") and kw.get("variant") is None:
            try:
                return orig(*a, **dict(kw, variant=23))
            except ValueError:
                pass
        return orig(*a, **kw)
    ops.conv_call = conv_call


def main():
    budget = int(sys.argv[1])
    assert L.lib().falnet_get_deterministic() == 1 and train.LABEL_WGS == budget and L.REPLAY
    _persistent_vgg_convs()
    dtype = torch.bfloat16
    LF.set_compute_dtype(dtype)
    sd = synthetic.seeded_falnetb_state_dict(49)
    m = FAL_netB({"state_dict": sd}, no_levels=49, compute_dtype=dtype).to("cuda").train()
    opt = train.FlatAdam(m)
    left, right, mn, mx = (t.cuda() for t in synthetic.synthetic_pair(2, 64, 128, seed=23, distinct=True))
    steps = []
    for _ in range(4):
        o = train.stage1_step(m, opt, left, right, mx)
        torch.cuda.synchronize()
        steps.append((float(o["loss"]).hex(), digest(m.flat_gradients()), digest(m.flat_parameters()), digest(o["ldisp"])))
    # the label plan of this run: its key, how many of its convs carry the budget, and how many of those run on fewer workgroups for it
    keys = sorted(k for k in LF.vgg._plans if not k[3])
    plan = LF.vgg._plans[keys[0]][0]
    lib = L.lib()
    budgeted = [c for c in plan.fwd if getattr(c, "max_wgs", 0)]
    cut = sum(1 for c in budgeted if lib.falnet_conv2d_workgroups(c.ref, c.max_wgs) < lib.falnet_conv2d_workgroups(c.ref, 0))
    print(json.dumps({"steps": steps, "label_plan_keys": [list(k) for k in keys], "budgeted": len(budgeted), "cut": cut,
                      "replayed": plan.run_fwd.seg is not None}), flush=True)


if __name__ == "__main__":
    main()
