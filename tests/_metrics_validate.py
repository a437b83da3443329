"""Helper of tests/test_gpu_metrics.py (run as a FALNET_DETERMINISTIC=1 process): train.validate over the KITTI-2015-shaped tree given on the
command line, with the host metrics and with device_metrics=True, same model, same frames -> one JSON line {'host', 'device', 'log'}."""
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from fal_net_amd import datasets as DS  # noqa: E402
from fal_net_amd import synthetic, train  # noqa: E402
from fal_net_amd.models import FAL_netB  # noqa: E402


def main():
    vroot = sys.argv[1]
    triples = DS.kitti2015_pairs(vroot)
    assert len(triples) == 2, triples
    model = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(49)}, 49, compute_dtype=torch.float32).to("cuda").eval()
    out, logs = {}, {}
    for name, flag in (("host", False), ("device", True)):
        loader = DS.make_loader(DS.StereoValDataset(vroot, triples), 1, 0, shuffle=False, drop_last=False)
        logs[name] = []
        out[name] = train.validate(model, loader, print_freq=1, log=logs[name].append, device_metrics=flag)
    print(json.dumps({"host": out["host"], "device": out["device"], "log": logs}))


if __name__ == "__main__":
    main()
