"""CPU: the host side of the batched augmentation (falnet_augment_batch) and of the HBM-resident training set -- the record layout
against the header, record packing, epoch sharding and the script switches.  No GPU, no compute calls."""
import importlib
import os
import re

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _header_fields(cname):
    """Field names of a `typedef struct { ... } cname;` of the header, in order (as test_cabi_symbols parses falnet_conv_t)."""
    src = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    end = src.index("} " + cname)
    body = src[src.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.sub(r"\[.*?\]", "", part.strip().split()[-1]).lstrip("*"))
    return fields


def test_record_layout_matches_header():
    """falnet_aug_t: two 64-bit addresses, eight int32, eight doubles = 112 bytes without padding; the ctypes mirror and the numpy
    dtype the table is filled through have the header's fields in the header's order at those offsets."""
    import ctypes
    from fal_net_amd import _lib
    from fal_net_amd import data_transforms as DT
    fields = _header_fields("falnet_aug_t")
    assert fields == ["src", "H", "W", "rw", "rh", "x1", "y1", "flip", "reserved", "gamma", "bright", "cb"]
    assert fields == [f[0] for f in _lib.Aug._fields_] == list(DT.AUG_DTYPE.names)
    assert ctypes.sizeof(_lib.Aug) == DT.AUG_DTYPE.itemsize == 2 * 8 + 8 * 4 + 8 * 8 == 112
    assert [DT.AUG_DTYPE.fields[n][1] for n in fields] == [0, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56, 64]
    assert [getattr(_lib.Aug, n).offset for n in fields] == [0, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56, 64]
    one = np.zeros(1, DT.AUG_DTYPE)
    assert one["src"].shape == (1, 2) and one["src"].dtype == np.uint64 and one["cb"].shape == (1, 2, 3) and one["cb"].dtype == np.float64
    hdr = open(os.path.join(ROOT, "include", "falnet_hip.h")).read()
    assert int(re.search(r"#define FALNET_AUG_MAX_SCALE (\d+)", hdr).group(1)) == DT.MAX_SCALE == 2  # the stated range contains [0.5, 2.0]


def test_record_packing_puts_each_value_in_its_field():
    from fal_net_amd import data_transforms as DT
    cb = [[0.81, 0.92, 1.03], [1.14, 1.05, 0.96]]
    params = [dict(factor=1.1, rw=176, rh=52, x1=7, y1=3, flip=False, gamma=None, bright=None, cbright=None),
              dict(factor=0.9, rw=900, rh=300, x1=11, y1=13, flip=True, gamma=0.85, bright=1.75, cbright=cb)]
    rec = DT.pack_records([(0x1000, 0x2000, 48, 160), (0x7f0000001000, 0x7f0000900000, 375, 1242)], params)
    assert rec.dtype == DT.AUG_DTYPE and rec.shape == (2,)
    a, b = rec[0], rec[1]
    assert a["src"].tolist() == [0x1000, 0x2000]  # no flip: left feeds position 0
    assert (a["H"], a["W"], a["rw"], a["rh"], a["x1"], a["y1"], a["flip"], a["reserved"]) == (48, 160, 176, 52, 7, 3, 0, 0)
    assert a["gamma"] == 0.0 and a["bright"] == 0.0 and not a["cb"].any()  # <= 0: not applied
    assert b["src"].tolist() == [0x7f0000900000, 0x7f0000001000]  # flip: the views swap, the RIGHT frame feeds position 0
    assert (b["H"], b["W"], b["rw"], b["rh"], b["x1"], b["y1"], b["flip"]) == (375, 1242, 900, 300, 11, 13, 1)
    assert b["gamma"] == 0.85 and b["bright"] == 1.75
    assert b["cb"].tolist() == cb  # the factors belong to the positions AFTER the swap: cb[j] goes with src[j]
    # into a caller's table (the pinned staging buffer): the first n records are written in place
    table = np.zeros(5, DT.AUG_DTYPE)
    out = DT.pack_records([(1, 2, 48, 160)], params[1:], table)
    assert out.shape == (1,) and table[0]["src"].tolist() == [2, 1] and table[0]["rw"] == 900 and not table[1:].view(np.uint8).any()


def test_epoch_batches_sharding():
    from fal_net_amd import datasets as DS
    n, B = 53, 4
    one = [list(DS.epoch_batches(n, 3, B, r, 2, seed=11)) for r in (0, 1)]
    again = [list(DS.epoch_batches(n, 3, B, r, 2, seed=11)) for r in (0, 1)]
    assert one == again  # the same on two calls with the same (seed, epoch)
    assert one != [list(DS.epoch_batches(n, 4, B, r, 2, seed=11)) for r in (0, 1)]  # another epoch, another permutation
    flat = [[i for b in shard for i in b] for shard in one]
    assert all(len(b) == B for shard in one for b in shard)
    assert not set(flat[0]) & set(flat[1])  # disjoint shards
    both = flat[0] + flat[1]
    assert len(both) == len(set(both)) == n - n % (2 * B) and set(both) <= set(range(n))
    single = [i for b in DS.epoch_batches(n, 3, B, seed=11) for i in b]
    assert len(set(single)) == len(single) == n - n % B
    # the same permutation on every rank: the strided shards interleave back into it
    assert flat[0][:3] == single[0:6:2] and flat[1][:3] == single[1:6:2]


def test_script_offers_both_switches_off_by_default():
    mod = importlib.import_module("Train_Stage1_K")
    a = mod.parser.parse_args([])
    assert a.batch_augment is False and a.resident_data is False
    a = mod.parser.parse_args(["--batch-augment"])
    assert a.batch_augment is True and a.resident_data is False
    assert mod.parser.parse_args(["--resident-data"]).resident_data is True


def test_build_compiles_the_file_without_contraction_and_outside_the_autotune_hash():
    from fal_net_amd import _build, _lib, ops
    assert "augment_batch.hip" in _build.SOURCES and _build.FILE_FLAGS["augment_batch.hip"] == ["-ffp-contract=off"]
    assert "augment_batch.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600  # the packaged autotune cache stays valid
    assert _lib.SIGNATURES["falnet_augment_batch"][-1] is _lib._P
