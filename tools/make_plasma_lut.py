#!/usr/bin/env python3
"""Writes fal_net_amd/plasma_lut.txt: matplotlib's 'plasma' colour map as 256 text rows 'r g b a' -- the table plt.imsave(cmap='plasma') indexes
(reference Test_KITTI.py:215-216).  The product reads the file and never imports matplotlib.  usage: python tools/make_plasma_lut.py"""
import os

import matplotlib
import numpy as np

lut = np.ascontiguousarray(matplotlib.colormaps["plasma"](np.arange(256), bytes=True))
assert lut.shape == (256, 4) and lut.dtype == np.uint8 and (lut[:, 3] == 255).all()
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fal_net_amd", "plasma_lut.txt")
np.savetxt(out, lut, fmt="%d", header="matplotlib 'plasma', 256 rows: red green blue alpha (tools/make_plasma_lut.py)")
print(os.path.normpath(out), "matplotlib", matplotlib.__version__)
