"""CPU (needs the built library, no device): fal_net_amd.ops._wgrad_plan_desc keeps only policy and asks the library -- falnet_wgrad_kernel_name --
whether a variant applies, which kernel runs and what it is called.

 (a) The parent's answers.  tests/golden/wgrad_plan_parent.json holds what the hand-written mirror of the parent commit (named in the file)
     answered on the inputs of tests/_wgrad_plan_inputs.py -- every case of tests/_wgrad_cases.py and tests/_wgrad_up2q_cases.py in each dtype, a
     sweep over channel counts, source forms, strides, up2 forms, shapes, batch sizes and slab budgets, and every WgradBatch.add of the training
     plans at the benchmark's shape and batch, dumped on an MI355X at the parent -- with the defaults and with each switch the planner reads flipped.  The inputs have canonical taps and
     aligned pointers, where that mirror was right, so (variant, nsplit, symbol) must be equal on every row.
 (b) The disagreements the mirror had with the library, closed: a misaligned image, the library's deterministic flag alone, non-canonical taps.
 (c) Every case of tests/_wgrad_cases.py reaches the instantiation its `kernel` field names, through the table KERNEL_TABLE spelled out there.
"""
import ctypes as C
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import _wgrad_cases as K  # noqa: E402
import _wgrad_plan_inputs as I  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import ops  # noqa: E402

with open(os.path.join(os.path.dirname(__file__), "golden", "wgrad_plan_parent.json")) as f:
    GOLD = json.load(f)
SECTIONS = {"cases": [s for _, s in GOLD["cases"]], "plans": [s for _, s in GOLD["plans"]], "sweep": list(I.sweep_specs())}


def test_fixture_covers_the_inputs():
    assert len(GOLD["parent"]) == 40
    assert GOLD["cases"] == [[label, spec] for label, spec in I.case_specs()]  # every case, every dtype, as the case modules have them today
    assert len(SECTIONS["sweep"]) == GOLD["sweep_len"] == len(GOLD["default"]["sweep"]) > 10000
    names = {n for n, _ in GOLD["plans"]}
    # (34 launches: the backbone's; the label VGG is frozen, its plan adds no weight gradient)
    assert len(GOLD["plans"]) == len(names) == 34 and {"wgrad conv0", "wgrad conv1", "wgrad(low-res) deconv1", "wgrad logits[skip]"} <= names
    assert sorted(GOLD["flipped"]) == sorted(label for label, *_ in I.SWITCHES[1:])
    kernels = {a[2].split("I")[0] for a in GOLD["answers"] if len(a) == 3}
    assert len(kernels) == 9 and ["ValueError"] in GOLD["answers"]  # the eight kernels (rows: two templates) and the refused up2 launches


@pytest.mark.parametrize("label,env,attrs,det", I.SWITCHES, ids=[s[0] for s in I.SWITCHES])
def test_parent_answers(label, env, attrs, det):
    """(variant, nsplit, symbol) of every input under one switch setting: equal to the parent's, no row excepted."""
    with I.switched(L, ops, env, attrs, det):
        for sec, specs in SECTIONS.items():
            want = list(GOLD["default"][sec])
            for i, v in GOLD["flipped"].get(label, {}).get(sec, {}).items():
                want[int(i)] = v
            assert len(want) == len(specs)
            bad = [(sec, i, spec, got, GOLD["answers"][w]) for i, (spec, w) in enumerate(zip(specs, want))
                   if (got := I.plan(L, ops, spec)) != GOLD["answers"][w]]
            assert not bad, f"{len(bad)} of {len(specs)} rows differ from the parent's plan; first: {bad[0]}"


# ------------------------------------------------------------------------------------------ (b) the closed disagreements
def _first_layer(name="c3_wave_16x64"):
    return dict(I.case_specs())[name + "-bf16"]


def test_misaligned_image_plans_the_patch_form():
    spec = _first_layer()
    npatch = K.geom(K.BY_NAME["c3_wave_16x64"])["npatch"]
    assert I.plan(L, ops, spec) == [6, 2 * 2 * 16 // 64, "_Z22wgrad3x3_c3wave_kernelIDF16bEv14falnet_wgrad_ti"]
    assert I.plan(L, ops, spec, ptr=I.FAKE + 4) == [6, min(ops._WGRAD_WGS, npatch), "_Z18wgrad3x3_c3_kernelIDF16bEv14falnet_wgrad_tiiii"]
    assert npatch == 16 != 2 * 2 * 16 // 64  # (the two forms' split counts differ here)


def test_library_deterministic_flag_alone_plans_the_patch_form():
    lib = L.lib()
    old = lib.falnet_get_deterministic()
    assert not ops.DETERMINISTIC and old == 0
    try:
        lib.falnet_set_deterministic(1)
        assert I.plan(L, ops, _first_layer()) == [6, 16, "_Z18wgrad3x3_c3_kernelIDF16bEv14falnet_wgrad_tiiii"]
    finally:
        lib.falnet_set_deterministic(old)
    assert I.plan(L, ops, _first_layer())[2].startswith("_Z22wgrad3x3_c3wave_kernel")


def test_noncanonical_taps_plan_the_per_tap_kernel():
    spec = ["bf16", [[64, "nhwc"]], 3, 1, 2, 9, 33, 9, 33, 64, 4096, 0]
    assert I.plan(L, ops, spec)[::2] == [7, "_Z22wgrad3x3_rows16_kernelIDF16bLi4ELi2ELb0EEv14falnet_wgrad_tiiii"]
    taps = I.taps_of(spec, ops)
    taps[0], taps[1] = taps[1], taps[0]  # nine taps, not in the canonical order: no halo kernel takes them
    tiles = 1 * 1 * 9  # per-tap split count: 64 x 64 channel tiles x taps against the 1536-workgroup target, at most ceil(M / 256) splits
    assert I.plan(L, ops, spec, taps=taps) == [0, min((1536 + tiles - 1) // tiles, (2 * 9 * 33 + 255) // 256), "_Z12wgrad_kernelIDF16bEv14falnet_wgrad_ti"]


# ------------------------------------------------------------------------------------------ (c) named kernels are reached
RUNS = [(c, dt) for c in K.CASES for dt in c["dtypes"]]


@pytest.mark.parametrize("case,dtype", RUNS, ids=[f"{c['name']}-{K.DTYPE_NAME[dt]}" for c, dt in RUNS])
def test_case_reaches_its_kernel(case, dtype):
    """falnet_wgrad_kernel_name on the descriptor the GPU test launches (fill_desc, the variant forced) names the case's instantiation."""
    kid, sym, fuses = K.KERNEL_TABLE[case["kernel"]]
    spec = dict(I.case_specs())[f"{case['name']}-{K.DTYPE_NAME[dtype]}"]
    d = I.descriptor(L, ops, spec, ptr=I.FAKE + (4 if case.get("misalign") else 0))
    d.variant, d.up2 = case["variant"], int(case["up2"])
    buf = C.create_string_buffer(160)
    for nsplit in (s for s in K.split_counts(case) if s != K.PLAN):
        d.nsplit = nsplit
        assert L.lib().falnet_wgrad_kernel_name(C.byref(d), buf, 160) == kid, L.lib().falnet_last_error()
        assert buf.value.decode() == sym.format(T=ops.TYPE_SYM[dtype])
        assert L.lib().falnet_wgrad_fuses_bias(C.byref(d)) == int(fuses)


def test_kernel_table_covers_the_ids():
    assert set(K.KERNEL_TABLE) == set(K.KERNELS)
    assert {kid for kid, _, _ in K.KERNEL_TABLE.values()} == {L.WGK_TAP, L.WGK_PATCH, L.WGK_S2, L.WGK_C3, L.WGK_C3WAVE, L.WGK_ROWS, L.WGK_ROWS_S2,
                                                             L.WGK_WAVE} == set(range(8))


def test_reported_symbols_are_kernels_of_the_library():
    """Every symbol the query can answer with -- the table's and the fixture's -- is a kernel descriptor (<symbol>.kd) of the built library."""
    with open(L._LIB_PATH, "rb") as f:
        blob = f.read()
    syms = {a[2] for a in GOLD["answers"] if len(a) == 3}
    syms |= {sym.format(T=ops.TYPE_SYM[dt]) for c, dt in RUNS for sym in [K.KERNEL_TABLE[c["kernel"]][1]]}
    assert len(syms) >= 32
    for s in sorted(syms):
        assert (s + ".kd").encode() in blob, s


def test_refusals_keep_their_text():
    """A descriptor falnet_wgrad refuses: a negative answer and the same error text, without a workspace."""
    d = I.descriptor(L, ops, ["bf16", [[64, "nhwc"]], 3, 1, 2, 9, 33, 9, 33, 64, 4096, 0])
    d.variant, d.nsplit = 9, 1
    buf = C.create_string_buffer(160)
    assert L.lib().falnet_wgrad_kernel_name(C.byref(d), buf, 160) < 0
    assert L.lib().falnet_last_error().decode().startswith("wgrad: variant 9 needs a 16-bit dense 3x3 stride-1 launch over ONE 32-channel NHWC source")
    d.variant, d.up2 = 0, 2
    assert L.lib().falnet_wgrad_kernel_name(C.byref(d), buf, 160) < 0
    assert L.lib().falnet_last_error().decode().startswith("wgrad: up2 (a deconv layer's gradient on the low-resolution grid) is a mode of variant 7 only")
