"""CPU: the workgroup budget of the conv launch path (falnet_conv2d_wgs) -- the entry points are replayable with the argument counts of
_lib.SIGNATURES, falnet_conv2d_workgroups gives the grid arithmetic of include/falnet_hip.h on descriptors built from committed cache keys
(no device call), and the budget is not part of the autotune key."""
import ctypes as C
import inspect
import json
import os

import pytest

from fal_net_amd import _lib as L
from fal_net_amd import ops

import _conv_ref as R

CACHE = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "autotune_cache.json")
with open(CACHE) as _f:
    ENTRIES = {k: tuple(v) for k, v in json.load(_f).items() if k.startswith("conv|")}
BUDGETS = (1, 3, 192, 4096)


_FAKE = {n: 1 << 20 for n in ("src0", "src1", "weight", "out", "bias", "addend", "actout", "pool_out", "pool_actout", "weight_up2", "splitk_ws")}
_FAKE["splitk_ws_bytes"] = 32 << 20  # (aligned stand-ins: the query checks the arguments like a launch and dereferences nothing)


def _desc(key):
    d = R.fill_desc(L.Conv(), R.parse_signature(key), _FAKE)
    d.variant, d.ksplit = ENTRIES[key]
    return d


def _key(pred):
    return next(k for k in sorted(ENTRIES) if pred(k, R.parse_signature(k), ENTRIES[k]))


def _wgs(d, budget):
    return L.lib().falnet_conv2d_workgroups(C.byref(d), budget)


@pytest.mark.parametrize("name", ["falnet_conv2d_wgs", "falnet_conv2d_multi_wgs"])
def test_budgeted_entry_points_are_replayable(name):
    cdll = L.lib()._cdll
    op = cdll.falnet_replay_op_index(name.encode())
    assert op >= 0
    nint, nflt = C.c_int(-1), C.c_int(-1)
    assert cdll.falnet_replay_op_args(op, C.byref(nint), C.byref(nflt)) == 0
    args = L.SIGNATURES[name]
    assert args[-1] is L._P  # the stream: filled in by falnet_replay
    flt = sum(1 for a in args[:-1] if a in (L._F, L._D))
    assert (nint.value, nflt.value) == (len(args) - 1 - flt, flt)
    # the unbudgeted entry point takes one integer less
    base = cdll.falnet_replay_op_index(name[:-4].encode())
    assert base >= 0 and base != op
    assert cdll.falnet_replay_op_args(base, C.byref(nint), C.byref(nflt)) == 0
    assert (nint.value, nflt.value) == (len(args) - 2 - flt, flt)


def test_workgroups_of_a_full_resolution_dma16_launch():
    """256 x 512, B = 8, 64 output channels on the 16 x 32 tile: 2048 tiles, one channel block."""
    key = _key(lambda k, s, c: c == (23, 1) and s["dtype"] == 1 and (s["B"], s["OH"], s["OW"], s["Cout"]) == (8, 256, 512, 64) and s["out_layout"] == 0)
    d = _desc(key)
    assert _wgs(d, 0) == 256
    for b in BUDGETS:
        assert _wgs(d, b) == min(b, 256), b
    assert _wgs(d, -1) < 0 and b"budget" in L.lib().falnet_last_error()


def test_workgroups_with_several_channel_blocks_and_few_tiles():
    """Every persistent (variant, shape) of the committed 16-bit keys: gx = max(1, min(budget, 256) / ny) columns of ny workgroups, never more
    than one column per tile, 4096 = 0; tile heights as in csrc/conv.hip: choose_conv_kernel."""
    th_of = {13: 16, 17: 4, 20: 8, 23: 16, 24: 4, 25: 8}
    seen = set()
    for key in sorted(ENTRIES):
        s, (v, ks) = R.parse_signature(key), ENTRIES[key]
        if v not in th_of or s["dtype"] == 0:
            continue
        ny = (s["Cout"] + 63) // 64
        ntiles = s["B"] * ((s["OW"] + 31) // 32) * ((s["OH"] + th_of[v] - 1) // th_of[v])
        if (v, ny, ntiles) in seen:
            continue
        seen.add((v, ny, ntiles))
        d = _desc(key)
        full = _wgs(d, 0)
        assert full == min(max(1, 256 // ny), ntiles) * ny, key
        for b in BUDGETS:
            got = _wgs(d, b)
            assert got == min(max(1, min(b, 256) // ny), ntiles) * ny, (key, b)
            assert got <= ntiles * ny and got <= full
        assert _wgs(d, 4096) == full
    assert any(ny > 1 for _, ny, _ in seen) and any(nt < 256 for _, _, nt in seen) and len({v for v, _, _ in seen}) >= 3


def test_a_gather_launch_ignores_the_budget():
    key = _key(lambda k, s, c: c == (1, 1) and s["dtype"] == 1 and s["B"] == 8)
    d = _desc(key)
    s = R.parse_signature(key)
    full = _wgs(d, 0)
    assert full == ((s["B"] * s["TH"] * s["TW"] + 127) // 128) * ((s["Cout"] + ops.gather_bn(s["w_rows"], s["Cout"]) - 1) // ops.gather_bn(s["w_rows"], s["Cout"]))
    for b in BUDGETS:
        assert _wgs(d, b) == full, b
    assert _wgs(d, -1) < 0


def test_budget_is_not_in_the_signature():
    """ops.conv_call takes max_wgs, ops.conv_signature reads the descriptor alone -- and falnet_conv_t has no budget field (pool_code stays last)."""
    assert "max_wgs" in inspect.signature(ops.conv_call).parameters
    assert list(inspect.signature(ops.conv_signature).parameters) == ["d"]
    assert L.Conv._fields_[-1][0] == "pool_code" and not any("wg" in f[0] for f in L.Conv._fields_)
    key = _key(lambda k, s, c: c == (23, 1) and s["dtype"] == 1)
    assert ops.conv_signature(_desc(key)) == key
