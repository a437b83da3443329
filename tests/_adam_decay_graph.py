"""Helper of tests/test_gpu_adam_decay.py::test_captured_step_decays_through_the_standalone_update, run as a child process (a capture that
fails leaves the HIP context of its process unusable): train.GraphedStage1Step with non-zero decays against the float64 reference."""
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import synthetic, train  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402

import _adam_decay_ref as R  # noqa: E402

DEV = "cuda"
LR, BETAS, EPS, WD, BD = 1e-4, (0.5, 0.999), 1e-8, 1e-2, 3e-3


def main():
    LF.set_compute_dtype(torch.float32)
    m = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(7)}, no_levels=7, compute_dtype=torch.float32).to(DEV).train()
    opt = train.FlatAdam(m, LR, BETAS, EPS, weight_decay=WD, bias_decay=BD)
    left, right, mn, mx = (t.to(DEV) for t in synthetic.synthetic_pair(1, 64, 128, seed=9))
    m.ensure_flat()
    named = dict(m._trainable_named())
    ref, ref0 = R.RefAdam64(named, LR, BETAS, EPS, WD, BD), R.RefAdam64(named, LR, BETAS, EPS)

    def advance(k, what, seen=False):
        flat = m.flat_gradients().detach().cpu()
        g = {n: flat[off:off + p.numel()] for (n, p), off in zip(m._trainable_named(), m._offsets)}
        ref.step(g)
        ref0.step(g)
        for n, p in named.items():
            R.check(p, ref.p[n].detach(), k, LR, f"{what} {n}")
            if seen:
                R.check_decay_seen(p, ref0.p[n].detach(), k, LR, f"{what} {n}")

    for k in (1, 2):
        train.stage1_step(m, opt, left, right, mx)
        advance(k, f"eager step {k}")
    assert opt._segments is not None and opt._segments[1].key == (WD, BD)  # kept current by the pack-fused steps: ready for a capture
    step = train.GraphedStage1Step(m, opt, left, right, mx, warmup=1)  # (capture launches nothing: the buffer holds the warm-up step's gradient)
    advance(3, "warm-up step")
    for k in (4, 5, 6):
        out = step()
        assert torch.isfinite(out["loss"]).item()
        advance(k, f"replay {k - 3}", seen=k == 6)
    assert float(opt.state[1]) == 6.0
    print("graphed decay: ok", flush=True)


if __name__ == "__main__":
    main()
