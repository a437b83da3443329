"""CPU tests of tests/_wgrad_ref.py (the float64 reference the GPU weight-gradient tests compare with) and of the case list of
tests/_wgrad_cases.py: the reference equals float64 autograd of F.conv2d for every source form, both strides and the four tap sets;
every GPU case keeps its f32 sums exact; every kernel has a case whose largest |dW| needs more than 16 bits; three mutations of the
reference each change its result (so a kernel with the same defect could not pass)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import _wgrad_cases as K  # noqa: E402
import _wgrad_ref as R  # noqa: E402

F64 = torch.float64


def _mode(name, B, groups, cout, H, W, stride, k, forms, up2=False):
    return K._c(name, "reference", 0, B, groups, cout, H, W, (1,), stride=stride, k=k, forms=forms, up2=up2)


MODES = []
for _s in (1, 2):
    for _k in (3, (3, 1), (1, 3), 1):
        _t = f"s{_s}_k{_k if isinstance(_k, int) else '%dx%d' % _k}"
        MODES.append(_mode(f"two_sources_{_t}", 2, [5, 3], 7, 9, 11, _s, _k, ["nhwc", "nhwc"]))
        MODES.append(_mode(f"half_source_{_t}", 2, [4], 5, 8, 12, _s, _k, ["half"]))
        MODES.append(_mode(f"half_rows_second_source_{_t}", 1, [3, 4], 5, 8, 10, _s, _k, ["nhwc", "halfh"]))
        MODES.append(_mode(f"const_second_source_{_t}", 3, [6, 1], 4, 7, 10, _s, _k, ["nhwc", "bcast"]))
        MODES.append(_mode(f"planar_image_{_t}", 2, [3], 32, 6, 9, _s, _k, ["planar"]))
    MODES.append(_mode("up2_3x3", 2, [5], 6, 5, 7, 1, 3, ["nhwc"], up2=True))
K.BY_NAME.update({m["name"]: m for m in MODES})  # (host_operands looks a case up by name)


@pytest.mark.parametrize("case", MODES, ids=[m["name"] for m in MODES])
def test_reference_equals_float64_autograd(case):
    g = K.geom(case)
    desc = g["desc"]
    srcs, gout = K.host_operands(case)
    slab, oihw = R.wgrad_ref(desc, srcs, gout)
    assert slab.dtype == F64 and tuple(slab.shape) == (len(desc["taps"]), desc["gC"], desc["cin_total"])
    real = []  # the real channels of every source, NCHW
    for t, f, c in zip(srcs, case["forms"], case["groups"]):
        real.append(t[:, :c] if f in ("bcast", "planar") else t[..., :c].permute(0, 3, 1, 2))
    dw, db = R.conv_autograd(desc, real, gout[..., :desc["cout"]].permute(0, 3, 1, 2))
    assert torch.equal(oihw, dw.reshape(desc["cout"], desc["cin"], -1))
    assert torch.equal(R.bias_ref(gout, desc["cout"]), db)
    # the slab holds the same numbers at the packed columns, and nothing in the padding columns of the sources
    cols = R.unpack_columns(desc)
    assert torch.equal(slab[:, :desc["cout"]][:, :, cols].permute(1, 2, 0), oihw)
    pad = [c for c in range(desc["cin_total"]) if c not in cols]
    assert float(slab[:, :, pad].abs().max()) == 0.0 if pad else True
    assert float(oihw.abs().max()) > 0


def test_slab_sum_adds_raw_slabs_in_float64():
    ws = torch.arange(2 * 3 * 4 * 5 + 7, dtype=torch.float32)
    s = R.slab_sum(ws, 3, 2, 4, 5)
    assert s.dtype == F64 and torch.equal(s, ws[:120].view(3, 2, 4, 5).double().sum(0))
    assert torch.equal(R.slab_sum(ws, 3, 2, 4, 5, first=1), ws[40:120].view(2, 2, 4, 5).double().sum(0))


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_every_gpu_case_keeps_its_sums_exact(case):
    bound = K.exactness(case)
    assert bound < 2 ** 24
    g = K.geom(case)
    assert g["n"] <= 139_000
    srcs, gout = K.host_operands(case)
    lo, hi = K.g_range(case)
    assert float(gout.min()) >= lo and float(gout.max()) <= hi and torch.equal(gout, gout.round())
    for t, f in zip(srcs, case["forms"]):
        if case.get("image") == "odd_grid":
            assert float(t.min()) > 0 and float(t.max()) < 2 and torch.equal(t * 1024 % 2, torch.ones_like(t))
            assert not torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t)  # bf16 has to round it
        else:
            assert float(t.min()) >= R.X_RANGE[0] and float(t.max()) <= R.X_RANGE[1] and torch.equal(t, t.round())
            for dt in case["dtypes"]:
                assert torch.equal(t.to(dt).float(), t) and torch.equal(gout.to(dt).float(), gout)
    for s in K.split_counts(case):
        assert s == K.PLAN or (isinstance(s, int) and s >= 1)
    if case["up2"]:
        assert all(s == K.PLAN or s % 4 == 0 for s in case["nsplits"])


def test_exactness_assertion_refuses_what_is_not_exact():
    assert R.assert_exact(139_000, 15, 8) < 2 ** 24
    with pytest.raises(AssertionError):
        R.assert_exact(140_000, 15, 8)
    with pytest.raises(AssertionError):
        R.assert_exact(1024, 2.0, 8, unit=2.0 ** -10)


# the case of every kernel with the most positions: its largest |dW| must not fit a 16-bit intermediate
_BIGGEST = {}
for _c in K.CASES:
    if _c.get("image") != "odd_grid" and (_c["kernel"] not in _BIGGEST or K.geom(_c)["n"] > K.geom(_BIGGEST[_c["kernel"]])["n"]):
        _BIGGEST[_c["kernel"]] = _c


@pytest.mark.parametrize("kernel", K.KERNELS)
def test_every_kernel_has_a_case_beyond_16_bits(kernel):
    case = _BIGGEST[kernel]
    ref = K.reference(case)
    assert ref["max_abs"] >= 4096, (case["name"], ref["max_abs"])
    assert ref["max_abs"] < 2 ** 24


def test_det_and_mutation_cases_cover_every_kernel():
    assert {K.BY_NAME[n]["kernel"] for n in K.DET_CASES} == set(K.KERNELS)
    assert {K.BY_NAME[n]["variant"] for n in K.MUTATION_CASES.values()} == {7, 9}


MUT = K._c("mutations", "reference", 0, 2, [5, 3], 6, 7, 9, (1,))
K.BY_NAME[MUT["name"]] = MUT


def test_reference_mutations_change_the_result():
    desc = K.geom(MUT)["desc"]
    srcs, gout = K.host_operands(MUT)
    slab, oihw = R.wgrad_ref(desc, srcs, gout)
    shifted = R.wgrad_ref(desc, srcs, gout, tap_shift=(4, 1))   # the centre tap reads one pixel to the right
    assert not torch.equal(shifted[1], oihw)
    assert torch.equal(shifted[1][..., 4], oihw[..., 5])        # ... which is what the next tap reads
    dropped = R.wgrad_ref(desc, srcs, gout, drop_last_column=True)
    assert not torch.equal(dropped[1], oihw)
    swapped = R.wgrad_ref(desc, srcs, gout, swap_groups=True)
    assert not torch.equal(swapped[1], oihw) and tuple(swapped[1].shape) == tuple(oihw.shape)
    assert torch.equal(R.wgrad_ref(desc, srcs, gout)[1], oihw)  # and the reference itself is a function of its operands only
