"""Helper of tests/test_gpu_mesh.py (run as a FALNET_DETERMINISTIC=1 process: the forward then computes what the same command line computed in the
process before it): runs Test_KITTI.py's main() with the arguments after the first one, with MeshWriter.write wrapped so that what each frame's mesh is
made of -- the input image, the disparity and the confidence map -- is also saved as <first argument>/frame_<i>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import Test_KITTI as T  # noqa: E402
from fal_net_amd import mesh  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    write = mesh.MeshWriter.write

    def recording_write(self, i, left, disp, conf=None):
        H, W = disp.shape[-2:]
        np.savez(os.path.join(out, "frame_{}.npz".format(i)), left=left.detach().float().cpu().numpy().reshape(3, H, W),
                 disp=disp.detach().float().cpu().numpy().reshape(H, W),
                 conf=np.zeros((0, 0), np.float32) if conf is None else conf.detach().float().cpu().numpy().reshape(H, W))
        return write(self, i, left, disp, conf=conf)

    mesh.MeshWriter.write = recording_write
    T.args = T.parser.parse_args(sys.argv[2:])
    T.main()


if __name__ == "__main__":
    main()
