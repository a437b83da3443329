"""Helper of tests/test_gpu_adam_decay.py::test_pack_fused_update_decays_and_repacks_the_decayed_masters, run as a child process with
FALNET_DETERMINISTIC=1 (read when the library is loaded).  In the default mode a forward is not reproducible bit for bit even on ONE model
(split-K / fused-bias atomics: the same model twice differs by ~2e-4 of 160 at this shape), so the bit comparison of the disparity of a
trained model with that of a fresh model loaded from its state_dict() is made where forwards are reproducible at all.
Per dtype: three decayed stage1_steps through the update fused with the re-pack, then the trained model's forward against a fresh model's."""
import hashlib
import json
import os
import sys

os.environ["FALNET_DETERMINISTIC"] = "1"
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch  # noqa: E402

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import synthetic, train  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def run(dtype):
    LF.set_compute_dtype(dtype)
    m = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(49)}, no_levels=49, compute_dtype=dtype).to("cuda").train()
    start = digest(m.ensure_flat())
    opt = train.FlatAdam(m, 1e-4, (0.5, 0.999), 1e-8, weight_decay=1e-2, bias_decay=3e-3)
    left, right, mn, mx = (t.cuda() for t in synthetic.synthetic_pair(2, 64, 128, seed=3, distinct=True))
    for _ in range(3):
        train.stage1_step(m, opt, left, right, mx)
    assert train._ADAM_PACK and m._packed_is_fresh()  # the forward below runs on what the optimiser packed
    with torch.no_grad():
        trained = m(left, mn, mx)
        again = m(left, mn, mx)
        fresh_model = FAL_netB({"state_dict": {k: v.detach().clone() for k, v in m.state_dict().items()}}, no_levels=49, compute_dtype=dtype).to("cuda").train()
        fresh = fresh_model(left, mn, mx)
    return {"moved": digest(m.flat_parameters()) != start, "trained": digest(trained), "again": digest(again), "fresh": digest(fresh)}


def main():
    assert L.lib().falnet_get_deterministic() == 1
    print(json.dumps({"f32": run(torch.float32), "bf16": run(torch.bfloat16)}), flush=True)


if __name__ == "__main__":
    main()
