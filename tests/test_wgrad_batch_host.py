"""Host test of fal_net_amd.ops.WgradBatch.finalize (no GPU: the tables are built on the CPU and nothing is launched): a bucket with more
than 64 weight tensors / biases is cut into launches of at most 64 entries -- the batched slab reduce and bias-gradient kernels stage a
table's block_begin column in a 64-int LDS array and the library refuses longer tables."""
import types

import torch

from fal_net_amd import _lib as L
from fal_net_amd import ops


def _tables(launches, desc_type):
    out = []
    for table, n, blocks in launches:
        raw = bytes(table.numpy().tobytes())
        assert len(raw) == n * len(bytes(desc_type()))
        out.append(([desc_type.from_buffer_copy(raw, i * len(bytes(desc_type()))) for i in range(n)], blocks))
    return out


def test_finalize_cuts_long_tables_into_launches_of_64():
    wb = ops.WgradBatch(torch.bfloat16, torch.device("cpu"))
    n_items, n_bias = 70, 67
    grads, gouts, dbs = [], [], []
    for i in range(n_items):
        cout, cin = 3 + i % 5, 32 * (1 + i % 3)
        grads.append(torch.zeros(cout, cin, 3, 3))
        wb.items.append(dict(bucket=0, post=[], d=types.SimpleNamespace(partial=0), bytes=4 * 9 * 32 * cin * (1 + i % 7), nsplit=1 + i % 7, ntaps=9,
                             w_rows=32, cin_total=cin, cout=cout, cin=cin, c0_real=cin, c0_pad=cin, grad=grads[-1]))
    wb.items.append(dict(wb.items[0], bucket=1, d=types.SimpleNamespace(partial=0), post=[]))  # a second bucket with one layer and no bias
    for i in range(n_bias):
        gouts.append(torch.zeros(2, 4, 8, 32, dtype=torch.bfloat16))
        dbs.append(torch.zeros(32))
        wb.bias.append(dict(bucket=0, g=gouts[-1], npix=64 * (1 + i), gC=32, cout=3 + i % 5, db=dbs[-1]))
    out = wb.finalize()
    assert sorted(out) == [0, 1] and sorted(wb.launches) == [0, 1]
    assert wb.MAX_TABLE == 64
    red, bias = _tables(wb.launches[0]["reduce"], L.ReduceDesc), _tables(wb.launches[0]["bias"], L.BiasGradDesc)
    assert [len(t) for t, _ in red] == [64, 6] and [len(t) for t, _ in bias] == [64, 3]
    # every launch: block_begin restarts at 0 and counts its own entries only; every item appears once, in order, with its own pointers
    seen = []
    for table, blocks in red:
        blk = 0
        for r in table:
            assert r.block_begin == blk
            blk += L.lib().falnet_wgrad_reduce_blocks(r.cout, r.cin_total, 1) * r.groups
            seen.append((r.partial, r.grad, r.nsplit, r.cout, r.cin_total))
        assert blk == blocks
    items0 = [it for it in wb.items if it["bucket"] == 0]
    assert seen == [(it["partial"], it["grad"].data_ptr(), it["nsplit"], it["cout"], it["cin_total"]) for it in items0]
    assert len({s[0] for s in seen}) == n_items  # (every layer has its own slab region)
    seen = []
    for table, blocks in bias:
        blk = 0
        for b in table:
            assert b.block_begin == blk and b.blocks >= 1
            blk += b.blocks
            seen.append((b.g, b.db, b.npix, b.cout))
        assert blk == blocks
    assert seen == [(it["g"].data_ptr(), it["db"].data_ptr(), it["npix"], it["cout"]) for it in wb.bias]
    assert [len(t) for t, _ in _tables(wb.launches[1]["reduce"], L.ReduceDesc)] == [1] and wb.launches[1]["bias"] == []


def test_finalize_keeps_one_launch_for_a_bucket_of_64():
    wb = ops.WgradBatch(torch.bfloat16, torch.device("cpu"))
    g = torch.zeros(4, 32, 3, 3)
    for i in range(64):
        wb.items.append(dict(bucket=0, post=[], d=types.SimpleNamespace(partial=0), bytes=4 * 9 * 32 * 32, nsplit=1, ntaps=9, w_rows=32, cin_total=32,
                             cout=4, cin=32, c0_real=32, c0_pad=32, grad=g))
    wb.finalize()
    assert [n for _, n, _ in wb.launches[0]["reduce"]] == [64] and wb.launches[0]["bias"] == []
