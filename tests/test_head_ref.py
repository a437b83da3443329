"""CPU: the float64 reference, the magnitudes, the comparator and the integer-margin precondition of tests/_head_ref.py -- so that the
reference tests/test_gpu_head.py holds the MED head kernels to cannot be wrong, or toothless, unnoticed."""
import pytest
import torch

from oracle import falnet_oracle as O

import _head_ref as R

f64 = torch.float64
KEYS = ("disp", "p_im0", "maskL", "maskR", "maskR_acfalse", "grad_both", "grad_disp", "grad_pan")
COEF_OF = {"disp": "disp", "p_im0": "p_im0", "maskL": "mask", "maskR": "mask", "maskR_acfalse": "mask", "grad_both": "grad",
           "grad_disp": "grad", "grad_pan": "grad"}


def test_integer_margin_holds_for_every_listed_case_and_fires_on_a_constructed_one():
    """The precondition for every listed case (both samples of the B = 2 ones) with the closest approach the list was chosen with; and
    W = 2, mx = 4, mn = 2, N = 2: d = {2, 4}, s = d / 2 = {1, 2}, on which it must fire."""
    worst = min((R.assert_integer_margin(*_mn_mx(case), case[1], case[3]), case) for case in R.ALL_CASES)
    assert worst[1] == (1, 7, 1, 2100, 300.0) and 9e-4 < worst[0] < 1e-3, worst
    assert sorted(R.NEW_CASE_KERNELS) == sorted(R.NEW_CASES)
    mn, mx = torch.tensor([2.0]), torch.tensor([4.0])
    assert R.integer_margin(mn, mx, 2, 2) < 1e-12
    with pytest.raises(AssertionError, match="from an integer"):
        R.assert_integer_margin(mn, mx, 2, 2)
    inp = R.make_inputs((1, 2, 2, 2, 4.0), "a")
    inp["mn"] = mn
    with pytest.raises(AssertionError, match="from an integer"):
        R.reference(inp)


def _mn_mx(case):
    inp = R.make_inputs(case, "c")
    return inp["mn"], inp["mx"]


@pytest.mark.parametrize("family", R.ALL_FAMILIES)
@pytest.mark.parametrize("case", R.SMALL_CASES)
def test_float64_reference_agrees_with_the_float32_oracle(case, family):
    """The float32 oracle run (the reference of tests/test_gpu_ops.py) against the float64 one, element-wise: 2^-16 of the magnitude --
    float32 accuracy over sums of up to N terms and exponents of size 100 -- and the magnitudes dominate the values."""
    inp, ref = R.cached(case, family)
    B, N, H, W, _ = case
    d0 = inp["dlog0"].clone().requires_grad_(True)
    mn, mx = inp["mn"].view(B, 1, 1), inp["mx"].view(B, 1, 1)
    out = O.med_head(d0, inp["left"], mn, mx, True, True, True)
    got = {"disp": out["disp"], "p_im0": out["p_im0"], "maskL": out["maskL"], "maskR": out["maskR"]}
    got["maskR_acfalse"] = O.med_head(d0.detach(), inp["left"], mn, mx, True, True, False, maskr_align_corners=False)["maskR"]
    ld, lp = (out["disp"] * inp["gd"]).sum(), (out["p_im0"] * inp["gp"]).sum()
    got["grad_disp"] = torch.autograd.grad(ld, d0, retain_graph=True)[0]
    got["grad_pan"] = torch.autograd.grad(lp, d0, retain_graph=True)[0]
    got["grad_both"] = torch.autograd.grad(ld + lp, d0)[0]
    for key in KEYS:
        res = R.compare(got[key], ref[key], ref["mag_" + key], torch.float32, 2.0 ** -16)
        assert res["bad"] == 0, (key, res)
        assert bool((ref["mag_" + key] * (1 + 1e-12) + 1e-300 >= ref[key].abs()).all()), key
    # the hand-written tap positions of the align_corners=False magnitude: with the bilinear weights they reproduce the oracle's grid_sample
    sm = torch.softmax(inp["dlog0"].to(f64), 1)
    d = O.plane_disparities(inp["mn"].to(f64), inp["mx"].to(f64), N)
    weighted = R._acfalse_taps(sm, d, weighted=True).clamp(max=1.0)
    assert torch.allclose(weighted, ref["maskR_acfalse"], rtol=1e-12, atol=1e-14)
    if family == "c":  # uniform softmax: disp is the mean of d_n
        assert torch.allclose(ref["disp"], d.mean(1).view(B, 1, 1, 1).expand_as(ref["disp"]), rtol=1e-14)


def _mutants(inp):
    """Three reference-side mutations of a case: (name, mutated reference, number of planes to compare)."""
    N = inp["dlog0"].shape[1]
    yield "last plane removed", R.reference(inp, n_planes=N - 1, check_margin=False), N - 1
    m = dict(inp)
    m["mn"] = inp["mn"] * (1 + 2.0 ** -10)
    yield "min_disp (1 + 2^-10)", R.reference(m, check_margin=False), N
    m = dict(inp)
    m["dlog0"] = inp["dlog0"].clone()
    m["dlog0"][:, N // 2] = torch.roll(inp["dlog0"][:, N // 2], 1, dims=-1)
    yield "one plane rolled by a pixel", R.reference(m, check_margin=False), N


@pytest.mark.parametrize("case", [R.ALL_CASES[0], R.ALL_CASES[1]])
def test_comparator_catches_reference_side_mutations(case):
    """A float32 image of a MUTATED float64 reference is outside the bound the GPU tests use, in disp, p_im0 and grad_dlog0; the float32
    image of the reference itself is inside it."""
    inp, ref = R.cached(case, "a")
    for key in ("disp", "p_im0", "grad_both"):
        res = R.compare(ref[key].float(), ref[key], ref["mag_" + key], torch.float32, R.coef(COEF_OF[key], case))
        assert res["bad"] == 0, (key, res)
    nan = ref["disp"].float().clone()
    nan.view(-1)[3] = float("nan")
    assert R.compare(nan, ref["disp"], ref["mag_disp"], torch.float32, R.coef("disp", case))["bad"] == 1
    for name, mut, n in _mutants(inp):
        for key in ("disp", "p_im0", "grad_both"):
            got = mut[key].float()
            want, mag = ref[key], ref["mag_" + key]
            if key == "grad_both":
                want, mag = want[:, :n], mag[:, :n]
            res = R.compare(got, want, mag, torch.float32, R.coef(COEF_OF[key], case))
            assert res["bad"] > 0, (name, key, res)
