#!/usr/bin/env python3
"""Generates tests/golden/dumps_plasma.npz with matplotlib (needed here only): the disparity PNG exactly as the reference writes it
(Test_KITTI.py:213-216) for seeded disparity maps, read back as RGBA.  usage: python tests/golden/make_dump_goldens.py

Per size (75 x 250 and 375 x 1242), input (rng(0).random(shape) ** 3 * 120) as f32:
  p95_<s>     np.percentile(disp, 95)
  rgba_<s>    the image plt.imsave wrote (75 x 250 only: the large one is rebuilt from the table in the test)
  margin_<s>  how many pixels of the HOST restatement change when p95 moves by a factor 1 +- 1e-6 (the percentile margin of
              tests/test_gpu_dumps.py), and the largest table step any of them moves by."""
import io
import os

import matplotlib
matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def seeded_disp(shape):
    return (np.random.default_rng(0).random(shape) ** 3 * 120).astype(np.float32)


def index(disp, p95):
    v = 256 * np.clip(disp / (p95 + np.float32(1e-6)), 0, 1)
    return np.minimum(np.rint(v), 255).astype(np.int32)


out = {}
for tag, shape in (("75x250", (75, 250)), ("375x1242", (375, 1242))):
    disp = seeded_disp(shape)
    p95 = np.percentile(disp, 95)
    assert p95.dtype == np.float32
    out["p95_" + tag] = p95
    k = index(disp, p95)
    changed = np.zeros(shape, bool)
    step = 0
    for f in (1 - 1e-6, 1 + 1e-6):
        k2 = index(disp, np.float32(p95 * f))
        changed |= k2 != k
        step = max(step, int(np.abs(k2 - k).max()))
    out["margin_" + tag] = np.array([int(changed.sum()), step])
    if tag == "75x250":
        disparity = 256 * np.clip(disp / (np.percentile(disp, 95) + 1e-6), 0, 1)  # the reference's two lines
        buf = io.BytesIO()
        plt.imsave(buf, np.rint(disparity).astype(np.int32), cmap="plasma", vmin=0, vmax=256, format="png")
        buf.seek(0)
        out["rgba_" + tag] = np.array(Image.open(buf).convert("RGBA"))
        assert out["rgba_" + tag].shape == shape + (4,)
    print(tag, "p95", float(p95), "pixels inside the margin", out["margin_" + tag])
np.savez_compressed(os.path.join(HERE, "dumps_plasma.npz"), **out)
