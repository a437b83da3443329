"""Host side of falnet_wgrad_t::up2 = 2 (no GPU): fal_net_amd.ops._wgrad_plan counts the units of the four-classes-per-step form WITHOUT the x4 of the
one-class-per-split form, does not round its split count to whole groups of four classes, and names wgrad3x3_up2q_kernel."""
import types

import torch

from fal_net_amd import ops

TAPS = [(dy, dx, 0) for dy, dx, _ in ops.fwd_taps(3)]


def _plan(up2, B, cin, cout, h, w, max_slabs=4096, dtype=torch.bfloat16):
    src = types.SimpleNamespace(C=cin, H=h, W=w, sy=w * cin, sx=cin, sb=h * w * cin)
    return ops._wgrad_plan(dtype, [src], TAPS, 1, B, h, w, h, w, cin, cout, max_slabs, up2=up2)


def test_units_without_the_class_factor():
    # 2 samples x 2 strips x 9 rows = 36 units, at least _WGRAD_ROWS_MIN_ROWS (8) rows per split
    assert ops._WGRAD_ROWS_MIN_ROWS == 8
    v1, n1, s1 = _plan(1, 2, 64, 64, 9, 33)
    v2, n2, s2 = _plan(2, 2, 64, 64, 9, 33)
    assert (v1, v2) == (7, 7)
    assert n1 == (4 * 36 // 8) - (4 * 36 // 8) % 8 == 16   # one class per split: 4 x 36 units, multiples of 8, whole groups of four
    assert n2 == 36 // 8 == 4                              # four classes per step: 36 units
    assert s1 == "_Z22wgrad3x3_rows16_kernelIDF16bLi4ELi2ELb1EEv14falnet_wgrad_tiiii"
    assert s2 == "_Z20wgrad3x3_up2q_kernelIDF16bLi2EEv14falnet_wgrad_tiiii"
    assert _plan(2, 2, 64, 64, 9, 33, dtype=torch.float16)[2] == "_Z20wgrad3x3_up2q_kernelIDF16_Li2EEv14falnet_wgrad_tiiii"


def test_splits_need_not_be_multiples_of_four():
    # 1 x 3 strips x 18 rows = 54 units -> 6 splits; a slab budget of 5 is taken whole (the one-class form rounds it down to 4)
    assert _plan(2, 1, 64, 64, 18, 70)[1] == 6
    assert _plan(2, 1, 64, 64, 18, 70, max_slabs=5)[1] == 5
    assert _plan(1, 1, 64, 64, 18, 70, max_slabs=5)[1] == 4
    assert _plan(2, 1, 64, 64, 18, 70, max_slabs=3)[1] == 3   # fewer than four slabs is no error for this form
    # the flagship deconv1 (B 8, 64 -> 64 at 128 x 256 low-res): one split per workgroup of the launch's budget, 64 low-resolution rows each
    assert _plan(2, 8, 64, 64, 128, 256)[1] == ops._WGRAD_ROWS_WGS
    # the high-resolution form is what it was
    assert _plan(0, 8, 64, 64, 256, 512)[2] == "_Z22wgrad3x3_rows16_kernelIDF16bLi4ELi2ELb0EEv14falnet_wgrad_tiiii"
