"""The MED head kernels (csrc/med_head.hip, med_head2.hip: ten head kernels and the two mask kernels) through the C-ABI, element by
element against the float64 oracle run of tests/_head_ref.py:  |got - ref| <= u |ref| + c mag + eta  with the measured c of
_head_ref.COEF (tests/test_head_ref.py holds the reference, the magnitudes and the comparator to account on the CPU).

Every output buffer is NaN before its launch, so an element a kernel never writes is a violation.  The pixel-major gradient gets one
guard pixel of NaN behind it (must stay NaN) and its padding channels [N, cpad) must come back exactly zero.  The same three mutations
the CPU test applies to the reference are applied to the KERNEL's inputs here (all valid launches) and must be reported as violations
in disp, p_im0 and grad_dlog0 under the same constants: the bound can fail.

FALNET_HEAD_REPORT=<path> appends one JSON line per comparison (coefficient needed, worst ratio, max-norm error)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import ops  # noqa: E402

import _head_ref as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
HEAD_KERNELS = {"med_head_fwd_lds2_kernel", "med_head_fwd_lds2_kernel<512 threads>", "med_head_fwd_lds_kernel", "med_head_fwd_kernel",
                "med_head_bwd_kernel<planar>", "med_head_bwd_lds2_kernel", "med_head_bwd_lds2_kernel<512 threads>", "med_head_bwd_wave_kernel",
                "med_head_bwd_lds_kernel", "med_head_bwd_kernel<nhwc>"}
# output key -> (reference key, COEF key)
PLANAR = {"disp": ("disp", "disp"), "p_im0": ("p_im0", "p_im0"), "maskL": ("maskL", "mask"), "maskR": ("maskR", "mask"),
          "maskR_acfalse": ("maskR_acfalse", "mask"), "grad_both": ("grad_both", "grad"), "grad_disp": ("grad_disp", "grad"),
          "grad_pan": ("grad_pan", "grad")}
NHWC = {"nhwc_f32": torch.float32, "nhwc_bf16": torch.bfloat16, "nhwc_f16": torch.float16}


def head_kernel(pas, dt, N, W):
    buf = ctypes.create_string_buffer(96)
    L.check(L.lib().falnet_med_head_kernel_name(pas, L.dtype_code(dt), N, W, buf, 96))
    return buf.value.decode()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def launch_all(inp, dlog0=None, mn=None):
    """Every head entry point once on the inputs of `inp` (optionally with other logits / min_disp: the mutations).  Returns the outputs
    on the CPU plus `checks`, a list of (what, ok) for the exact properties (padding channels, guard pixel)."""
    lib, st = L.lib(), L.stream_ptr()
    d0 = (inp["dlog0"] if dlog0 is None else dlog0).contiguous().to(DEV)
    B, N, H, W = d0.shape
    lf = inp["left"].to(DEV)
    mnd = (inp["mn"] if mn is None else mn).to(DEV)
    mxd = inp["mx"].to(DEV)
    gd, gp = inp["gd"].to(DEV), inp["gp"].to(DEV)
    o = {"disp": _nan(B, 1, H, W), "p_im0": _nan(B, 3, H, W), "maskL": _nan(B, 1, H, W), "maskR": _nan(B, 1, H, W),
         "maskR_acfalse": _nan(B, 1, H, W), "grad_both": _nan(B, N, H, W), "grad_disp": _nan(B, N, H, W), "grad_pan": _nan(B, N, H, W)}
    stats = _nan(B, 4, H, W)
    P = L.ptr
    L.check(lib.falnet_med_head_fwd(P(d0), P(lf), P(mnd), P(mxd), P(o["disp"]), P(o["p_im0"]), P(stats), B, N, H, W, st))
    L.check(lib.falnet_med_masks_fwd(P(d0), P(mnd), P(mxd), P(stats), P(o["maskL"]), P(o["maskR"]), B, N, H, W, st))
    L.check(lib.falnet_med_maskr_acfalse_fwd(P(d0), P(mnd), P(mxd), P(stats), P(o["maskR_acfalse"]), B, N, H, W, st))
    for key, g_d, g_p in (("grad_both", gd, gp), ("grad_disp", gd, None), ("grad_pan", None, gp)):
        L.check(lib.falnet_med_head_bwd(P(d0), P(lf), P(mnd), P(mxd), P(o["disp"]), P(o["p_im0"]), P(stats), P(g_d), P(g_p), P(o[key]),
                                        B, N, H, W, st))
    cp = ops.pad_c(N)
    checks = []
    for key, dt in NHWC.items():
        flat = _nan((B * H * W + 1) * cp, dtype=dt)  # one guard pixel behind the tensor
        L.check(lib.falnet_med_head_bwd_nhwc(P(d0), P(lf), P(mnd), P(mxd), P(o["disp"]), P(o["p_im0"]), P(stats), P(gd), P(gp), P(flat), cp,
                                             L.dtype_code(dt), B, N, H, W, st))
        gn = flat[:B * H * W * cp].view(B, H, W, cp)
        o[key] = gn[..., :N].permute(0, 3, 1, 2)
        checks.append((f"{key}: padding channels [N, cpad) exactly zero", cp == N or bool((gn[..., N:] == 0).all())))
        checks.append((f"{key}: guard pixel behind the tensor still NaN", bool(torch.isnan(flat[B * H * W * cp:]).all())))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}, checks


def compare_all(case, out, ref, n=None, tag=""):
    """{output key: comparator result} against `ref` (planes [0, n) of the gradients when the reference has fewer planes)."""
    res = {}
    for key in list(PLANAR) + list(NHWC):
        rkey, ckey = PLANAR.get(key, ("grad_both", "grad"))
        dtype = NHWC.get(key, torch.float32)
        got = out[key]
        if n is not None and rkey.startswith("grad"):
            got = got[:, :n]
        res[key] = R.compare(got, ref[rkey], ref["mag_" + rkey], dtype, R.coef(ckey, case))
        R.report({"case": list(case), "tag": tag, "output": key, "coef_key": ckey, "class": R.disp_class(case), **res[key]})
    return res


def test_head_cases_cover_every_head_kernel():
    seen = set()
    for B, N, H, W, maxd in R.ALL_CASES:
        seen.add(head_kernel(0, torch.float32, N, W))
        seen.add(head_kernel(1, torch.float32, N, W))
        seen |= {head_kernel(2, dt, N, W) for dt in DTYPES}
    assert seen == HEAD_KERNELS, (seen ^ HEAD_KERNELS)
    for case, (fwd, bwd) in R.NEW_CASE_KERNELS.items():  # the kernels the added cases were recorded to take
        assert head_kernel(0, torch.float32, case[1], case[3]) == fwd, case
        assert {head_kernel(2, dt, case[1], case[3]) for dt in DTYPES} == {bwd}, case
        assert head_kernel(1, torch.float32, case[1], case[3]) == "med_head_bwd_kernel<planar>"
    assert {c[2] for c in R.ALL_CASES} >= {1, 2, 5}  # heights the align_corners=False mask is held at


@pytest.mark.parametrize("case,family", [(c, f) for c in R.ALL_CASES for f in R.families(c)])
def test_head_against_float64(case, family):
    """disp, p_im0, maskL / maskR (the saved statistics through their use), FAL_netA's maskR, the planar gradient with both upstream
    gradients / disp only / pan only, and the pixel-major gradient in f32, bf16, f16: every element within the bound."""
    inp, ref = R.cached(case, family)
    out, checks = launch_all(inp)
    res = compare_all(case, out, ref, tag=family)
    for key, r in res.items():
        print(f"{case} {family} {key}: coef {r['coef']:.3g} worst ratio {r['worst_ratio']:.3g} max-norm {r['maxnorm']:.3g}")
    assert all(ok for _, ok in checks), [what for what, ok in checks if not ok]
    bad = {key: r for key, r in res.items() if r["bad"]}
    assert not bad, bad


def test_forward_of_logits_off_the_16_byte_grid():
    """The forward on logits that start one float into their allocation (4-byte aligned, not 16): the chooser's alignment predicate sends
    them past the second-generation kernel to med_head_fwd_lds_kernel, which fills its rows with scalar loads (as W = 77 and W = 1242 do).
    disp and p_im0 within the bound of the aligned cases.  (No backward twin: its fallback stores 16-byte vectors.)"""
    case = (1, 9, 2, 40, 30.0)
    inp, ref = R.cached(case, "a")
    B, N, H, W = inp["dlog0"].shape
    assert head_kernel(0, torch.float32, N, W) == "med_head_fwd_lds2_kernel"  # what the aligned launch of this shape takes
    room = torch.zeros(inp["dlog0"].numel() + 4, device=DEV)
    d0 = room[1:1 + inp["dlog0"].numel()].view(B, N, H, W)
    d0.copy_(inp["dlog0"])
    assert d0.data_ptr() % 16 == 4 and d0.is_contiguous()
    lf, mnd, mxd = inp["left"].to(DEV), inp["mn"].to(DEV), inp["mx"].to(DEV)
    disp, pan, stats = _nan(B, 1, H, W), _nan(B, 3, H, W), _nan(B, 4, H, W)
    P = L.ptr
    L.check(L.lib().falnet_med_head_fwd(P(d0), P(lf), P(mnd), P(mxd), P(disp), P(pan), P(stats), B, N, H, W, L.stream_ptr()))
    torch.cuda.synchronize()
    for key, got in (("disp", disp), ("p_im0", pan)):
        r = R.compare(got, ref[key], ref["mag_" + key], torch.float32, R.coef(key, case))
        print(f"{case} unaligned {key}: coef {r['coef']:.3g} worst ratio {r['worst_ratio']:.3g} max-norm {r['maxnorm']:.3g}")
        assert r["bad"] == 0, (key, r)
    assert bool(torch.isfinite(stats).all())


@pytest.mark.parametrize("case", [R.ALL_CASES[0], R.ALL_CASES[1]])
def test_head_bound_can_fail(case):
    """Valid launches on perturbed inputs against the UNperturbed reference: min_disp (1 + 2^-10), one logit plane rolled by a pixel, and
    an N-plane launch against the (N - 1)-plane reference.  Each must show violations in disp, p_im0 and grad_dlog0."""
    inp, ref = R.cached(case, "a")
    N = case[1]
    rolled = inp["dlog0"].clone()
    rolled[:, N // 2] = torch.roll(inp["dlog0"][:, N // 2], 1, dims=-1)
    trials = (("min_disp (1 + 2^-10)", launch_all(inp, mn=inp["mn"] * (1 + 2.0 ** -10))[0], ref, None),
              ("one plane rolled by a pixel", launch_all(inp, dlog0=rolled)[0], ref, None),
              ("N planes against N - 1", launch_all(inp)[0], R.reference(inp, n_planes=N - 1, check_margin=False), N - 1))
    for name, out, want, n in trials:
        res = compare_all(case, out, want, n=n, tag="mutation: " + name)
        for key in ("disp", "p_im0", "grad_both", "nhwc_f32"):
            print(f"{case} {name} {key}: {res[key]['bad']} of {res[key]['n']} over the bound, worst ratio {res[key]['worst_ratio']:.3g}")
            assert res[key]["bad"] > 0, (name, key, res[key])
