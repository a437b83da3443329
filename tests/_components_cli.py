"""Helper of tests/test_gpu_components.py: runs Test_KITTI.py's main() with the arguments after the first one, with MeshWriter.write and
PseudoLidarWriter.write wrapped so that what each frame's mesh and scan are made of -- the input image, the disparity, P and fb -- is also saved as
<first argument>/mesh_<i>.npz and <first argument>/lidar_<i>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import Test_KITTI as T  # noqa: E402
from fal_net_amd import mesh, pseudo_lidar  # noqa: E402


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    mesh_write, lidar_write = mesh.MeshWriter.write, pseudo_lidar.PseudoLidarWriter.write

    def recording_mesh_write(self, i, left, disp, conf=None):
        H, W = disp.shape[-2:]
        np.savez(os.path.join(out, "mesh_{}.npz".format(i)), left=left.detach().float().cpu().numpy().reshape(3, H, W),
                 disp=disp.detach().float().cpu().numpy().reshape(H, W))
        return mesh_write(self, i, left, disp, conf=conf)

    def recording_lidar_write(self, i, disp, P, fb, conf=None):
        H, W = disp.shape[-2:]
        np.savez(os.path.join(out, "lidar_{}.npz".format(i)), disp=disp.detach().float().cpu().numpy().reshape(H, W), P=np.asarray(P), fb=float(fb))
        return lidar_write(self, i, disp, P, fb, conf=conf)

    mesh.MeshWriter.write = recording_mesh_write
    pseudo_lidar.PseudoLidarWriter.write = recording_lidar_write
    T.args = T.parser.parse_args(sys.argv[2:])
    T.main()


if __name__ == "__main__":
    main()
