"""Helper of tests/test_gpu_pseudo_lidar.py (run as a FALNET_DETERMINISTIC=1 process: the forward then computes what the same command line computed
in the process before it): runs Test_KITTI.py's main() with the arguments after the first one, with PseudoLidarWriter.write wrapped so that what
each frame's scan is made of -- the disparity, P, fb and the confidence map -- is also saved as <first argument>/frame_<i>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import Test_KITTI as T  # noqa: E402
from fal_net_amd import pseudo_lidar  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    write = pseudo_lidar.PseudoLidarWriter.write

    def recording_write(self, i, disp, P, fb, conf=None):
        H, W = disp.shape[-2:]
        np.savez(os.path.join(out, "frame_{}.npz".format(i)), disp=disp.detach().float().cpu().numpy().reshape(H, W), P=np.asarray(P), fb=float(fb),
                 conf=np.zeros((0, 0), np.float32) if conf is None else conf.detach().float().cpu().numpy().reshape(H, W))
        return write(self, i, disp, P, fb, conf=conf)

    pseudo_lidar.PseudoLidarWriter.write = recording_write
    T.args = T.parser.parse_args(sys.argv[2:])
    T.main()


if __name__ == "__main__":
    main()
