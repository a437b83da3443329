"""Helper of tests/test_gpu_sparsify.py: runs Test_KITTI.py's main() with the arguments after the first one, with sparsification.curves wrapped so
that what each frame's curves are made of -- the evaluated disparity, the ground truth, the mode, the median switch and the score maps with their
signs -- is also saved as <first argument>/frame_<i>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import Test_KITTI as T  # noqa: E402
from fal_net_amd import sparsification  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    curves = sparsification.curves
    frames = []

    def recording_curves(pred_disp, gt, mode, scores, use_median=False, **kw):
        H, W = pred_disp.shape[-2:]
        np.savez(os.path.join(out, "frame_{}.npz".format(len(frames))), disp=pred_disp.detach().float().cpu().numpy().reshape(H, W),
                 gt=gt.detach().float().cpu().numpy().reshape(H, W), mode=mode, use_median=bool(use_median), names=list(scores),
                 signs=[s for _, s in scores.values()], maps=np.stack([m.detach().float().cpu().numpy().reshape(H, W) for m, _ in scores.values()]),
                 steps=kw.get("steps", sparsification.DEFAULT_STEPS))
        frames.append(1)
        return curves(pred_disp, gt, mode, scores, use_median=use_median, **kw)

    sparsification.curves = recording_curves
    T.args = T.parser.parse_args(sys.argv[2:])
    T.main()


if __name__ == "__main__":
    main()
