"""falnet_wgrad_t::up2 = 2 (wgrad3x3_up2q_kernel<T,2>): the weight gradient of a `deconv` layer (nearest x2, then 3x3 / pad 1) on the low-resolution
grid with all four parity classes of the upstream gradient per row step, through the C ABI.  Small integer operands (tests/_wgrad_up2q_cases.py), so
the reduced gradient and the fused bias gradient must EQUAL the float64 CPU reference, whatever the split count; the up2 = 1 form and the
high-resolution form of the same operands must give the same integers."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import _wgrad_up2q_cases as Q  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def _first_bad(got, ref):
    bad = (got != ref) | torch.isnan(got)
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return f"{int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: got {float(got[idx])}, reference {float(ref[idx])}"


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", Q.CASES, ids=[c["name"] for c in Q.CASES])
def test_up2q_exact(case, dtype):
    """Split counts 1, 3, 5 and one above the unit count (empty splits), each with and without the fused bias gradient: gradient == reference,
    bias gradient == reference, nothing written behind the slabs or behind the `cout` bias elements."""
    Q.assert_exact(case)
    dw, db = Q.reference(case["name"])
    for nsplit in Q.split_counts(case):
        for bias in (True, False):
            gw, gb, guard = Q.launch(case, DTYPES[dtype], nsplit, 2, bias)
            what = f"{case['name']} {dtype} nsplit={nsplit} bias={bias}"
            assert guard, what
            assert _first_bad(gw, dw) is None, f"{what}: {_first_bad(gw, dw)}"
            if bias:
                assert _first_bad(gb, db) is None, f"{what} (bias): {_first_bad(gb, db)}"


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", Q.CASES, ids=[c["name"] for c in Q.CASES])
def test_up2q_equals_other_forms(case, dtype):
    """The one-class-per-split form (up2 = 1) and the high-resolution form (up2 = 0, source upsampled on the fly) over the same operands."""
    quad, qb, _ = Q.launch(case, DTYPES[dtype], 5, 2, True)
    for up2, nsplit in ((1, 8), (0, 5)):
        gw, gb, guard = Q.launch(case, DTYPES[dtype], nsplit, up2, True)
        assert guard
        assert _first_bad(quad, gw) is None, f"{case['name']} {dtype} against up2={up2}: {_first_bad(quad, gw)}"
        assert _first_bad(qb, gb) is None, f"{case['name']} {dtype} bias against up2={up2}: {_first_bad(qb, gb)}"


def test_up2q_refused_launches():
    """Two sources, or a source that is not at the launch size, do not fit the form: the library says so instead of launching."""
    import ctypes as C
    import types

    from fal_net_amd import _lib as L
    from fal_net_amd import ops
    x = torch.zeros(1, 8, 32, 64, dtype=torch.bfloat16, device="cuda")
    g = torch.zeros(1, 32, 128, 64, dtype=torch.bfloat16, device="cuda")
    d = L.Wgrad()
    ops._fill_wgrad(d, torch.bfloat16, [ops.nhwc_src(x)], 16, 64, g, [(dy, dx, 0) for dy, dx, _ in ops.fwd_taps(3)], 1, 1, 16, 64,
                    types.SimpleNamespace(cout=64, cin_pad=64))
    d.variant, d.nsplit, d.up2 = 7, 3, 2
    ws = torch.zeros(3 * 9 * 64 * 64, device="cuda")
    d.partial = ws.data_ptr()
    assert L.lib().falnet_wgrad(C.byref(d), L.stream_ptr()) != 0
