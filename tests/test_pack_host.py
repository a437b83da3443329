"""CPU tests that pin tests/_pack_ref.py, the reference tests/test_gpu_pack.py holds the weight packers to: ref_wf_wd gives F.conv2d and
its autograd data gradient through tests/_conv_ref.conv_ref for every layer case; ref_wu / ref_wdd give the nearest x2 upsampling + 3x3
convolution and its autograd gradient (borders included); torch's 16-bit conversions are round-to-nearest-even on the tie sets, which a
truncating packer could not pass; a torch f32 stand-in of the fused Adam stays inside the m / v / p bounds and three wrong ones do not."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))

import _conv_ref as CR  # noqa: E402
import _pack_ref as R  # noqa: E402

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
PAD_FILL = 3.0  # what padded activation channels hold here: only ZERO weight columns / rows can hide them


def _sig(B, H, W, srcs_c, cin_total, taps, cout):
    return {"B": B, "IH": H, "IW": W, "TH": H, "TW": W, "stride": 1, "osy": 1, "ooy": 0, "oox": 0, "OH": H, "OW": W, "Cout": cout,
            "out_cstride": cout, "out_layout": CR.OUT_NHWC, "srcs": [{"C": c, "H": H, "W": W, "bcast": False} for c in srcs_c],
            "cin_total": cin_total, "taps": taps, "bias": False, "addend": False, "act": CR.ACT_NONE, "actout": False, "actout_kind": CR.ACT_NONE,
            "out": True, "pool": False, "pool_mode": 0, "pool_actout": False}


def _fwd_taps(kh, kw):
    """'same' padding: tap (kh, kw) reads pixel (y + kh - KH // 2, x + kw - KW // 2); packed tap index kh KW + kw."""
    return [(a - kh // 2, b - kw // 2, a * kw + b) for a in range(kh) for b in range(kw)]


@pytest.mark.parametrize("case", R.LAYER_CASES, ids=[c["name"] for c in R.LAYER_CASES])
def test_ref_wf_wd_give_conv2d_and_its_data_gradient(case):
    gen = torch.Generator().manual_seed(11)
    B, H, W = 2, 5, 6
    cout, cin, kh, kw = case["cout"], case["cin"], case["kh"], case["kw"]
    w = torch.randn(cout, cin, kh, kw, generator=gen, dtype=F64)
    wf, wd, real = R.ref_case(case, w, F64)
    assert wf.shape == (case["cout_pad"], case["taps"], case["cin_pad"]) and wd.shape == (case["cin_pad"], case["taps"], case["cout_pad"])
    assert int(real.sum()) == w.numel() and bool((wf[~real] == 0).all()) and torch.equal(wd, wf.permute(2, 1, 0))
    x = torch.randn(B, cin, H, W, generator=gen, dtype=F64, requires_grad=True)
    srcs, c = [], 0
    for g in case["groups"]:
        s = torch.full((B, H, W, R.pad_c(g)), PAD_FILL, dtype=F64)
        s[..., :g] = x.detach()[:, c:c + g].permute(0, 2, 3, 1)
        srcs.append(s)
        c += g
    taps = _fwd_taps(kh, kw)
    got = CR.conv_ref(_sig(B, H, W, [s.shape[3] for s in srcs], case["cin_pad"], taps, case["cout_pad"]), srcs, wf, want_mag=False)["ref"]
    y = F.conv2d(x, w, padding=(kh // 2, kw // 2))
    want = y.detach().permute(0, 2, 3, 1)
    scale = float(want.abs().max())
    assert float((got[..., :cout] - want).abs().max()) <= 1e-12 * scale
    assert bool((got[..., cout:] == 0).all())  # padded rows: exact zeros
    # wd: the transposed-operand form of the data gradient (taps mirrored, same tap index), over an upstream gradient whose padded channels are non-zero too
    gout = torch.randn(B, cout, H, W, generator=gen, dtype=F64)
    (gx,) = torch.autograd.grad(y, x, gout)
    gsrc = torch.full((B, H, W, case["cout_pad"]), PAD_FILL, dtype=F64)
    gsrc[..., :cout] = gout.permute(0, 2, 3, 1)
    dtaps = [(-dy, -dx, t) for dy, dx, t in taps]
    gin = CR.conv_ref(_sig(B, H, W, [case["cout_pad"]], case["cout_pad"], dtaps, case["cin_pad"]), [gsrc], wd, want_mag=False)["ref"]
    cols = real[0, 0]
    assert int(cols.sum()) == cin
    assert float((gin[..., cols] - gx.permute(0, 2, 3, 1)).abs().max()) <= 1e-12 * float(gx.abs().max())
    assert bool((gin[..., ~cols] == 0).all())


def test_layer_cases_are_the_listed_ones():
    got = [(c["name"], c["cout"], c["groups"], (c["kh"], c["kw"]), c["c0_real"], c["c0_pad"], c["cin_pad"], c["cout_pad"]) for c in R.LAYER_CASES]
    assert got == [("a", 32, [32], (3, 3), 32, 32, 32, 32), ("b", 64, [3], (3, 3), 3, 32, 32, 64), ("c", 49, [32, 1], (3, 3), 32, 32, 64, 64),
                   ("d", 7, [64, 32], (3, 3), 64, 64, 96, 32), ("e", 40, [49, 17], (3, 3), 49, 64, 96, 64), ("f", 96, [64], (3, 3), 64, 64, 64, 96),
                   ("g", 32, [64], (3, 1), 64, 64, 64, 32), ("h", 64, [32], (1, 3), 32, 32, 32, 64), ("i", 64, [49], (1, 1), 49, 64, 64, 64),
                   ("j", 1, [1], (3, 3), 1, 32, 32, 32)]
    assert R.UP2_CASES == [(32, 32), (49, 96), (64, 40)]
    # the padded columns the `ci < ci_end` guard of the tile kernel protects: cases b, c and e have columns beyond a group's real channels
    for name, npad in (("b", 29), ("c", 31), ("e", 15 + 15)):
        c = R.BY_NAME[name]
        assert c["cin_pad"] - c["cin"] == npad


# ------------------------------------------------------------------------------------------------------------------ sub-pixel weights
def _up2_layer(x, w):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)


@pytest.mark.parametrize("H,W", [(5, 7), (1, 1)])
@pytest.mark.parametrize("cout,cin", [(3, 2), (1, 1)])
def test_ref_wu_is_the_upsampled_convolution(H, W, cout, cin):
    """Four 2x2 convolutions over the low-resolution map, interleaved by parity; out-of-range neighbours are zero."""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, cin, H, W, generator=gen, dtype=F64)
    w = torch.randn(cout, cin, 3, 3, generator=gen, dtype=F64)
    wu = R.ref_wu(w)
    assert wu.shape == (32, 16, 32) and bool((wu[cout:] == 0).all()) and bool((wu[:, :, cin:] == 0).all())
    xp = F.pad(x, (1, 1, 1, 1))
    got = torch.zeros(2, cout, 2 * H, 2 * W, dtype=F64)
    for py in range(2):
        for px in range(2):
            acc = torch.zeros(2, cout, H, W, dtype=F64)
            for a in range(2):
                for b in range(2):
                    oy, ox = R.up_taps(py, a)[1], R.up_taps(px, b)[1]
                    nb = xp[:, :, 1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
                    acc += torch.einsum("oc,bchw->bohw", wu[:cout, 4 * (2 * py + px) + 2 * a + b, :cin], nb)
            got[:, :, py::2, px::2] = acc
    want = _up2_layer(x, w)
    assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("H,W", [(5, 7), (1, 1)])
@pytest.mark.parametrize("cout,cin", [(3, 2), (1, 1)])
def test_ref_wdd_is_the_autograd_gradient_of_the_upsampled_convolution(H, W, cout, cin):
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(2, cin, H, W, generator=gen, dtype=F64, requires_grad=True)
    w = torch.randn(cout, cin, 3, 3, generator=gen, dtype=F64)
    gout = torch.randn(2, cout, 2 * H, 2 * W, generator=gen, dtype=F64)
    (want,) = torch.autograd.grad(_up2_layer(x, w), x, gout)
    wdd = R.ref_wdd(w)
    cp = 32
    assert wdd.shape == (32, 4, 4 * cp) and bool((wdd[cin:] == 0).all())
    gp = F.pad(gout, (1, 1, 1, 1))  # row Y of gout is row Y + 1 of gp
    got = torch.zeros(2, cin, H, W, dtype=F64)
    for du in range(2):
        for dv in range(2):
            for e in range(2):
                for f in range(2):
                    blk = wdd[:cin, 2 * du + dv, (2 * e + f) * cp:(2 * e + f + 1) * cp]
                    assert bool((blk[:, cout:] == 0).all())
                    up = gp[:, :, 2 * du + e:2 * du + e + 2 * H:2, 2 * dv + f:2 * dv + f + 2 * W:2]  # rows 2 (i + du) - 1 + e, i = 0 .. H - 1
                    got += torch.einsum("co,bohw->bchw", blk[:, :cout], up)
    assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


def test_sub_pixel_tap_sets_and_f32_sum_order():
    """The tap sets the rule gives (include/falnet_hip.h states the same ones), and the f32 sums: exact on the dyadic set in any order,
    order-dependent on the normal set (so a kernel that added in another order would be told apart from one with wrong taps)."""
    assert [R.up_taps(0, 0)[0], R.up_taps(0, 1)[0], R.up_taps(1, 0)[0], R.up_taps(1, 1)[0]] == [[0], [1, 2], [0, 1], [2]]
    assert [R.adj_taps(0, 0), R.adj_taps(0, 1), R.adj_taps(1, 0), R.adj_taps(1, 1)] == [[2], [1, 2], [0, 1], [0]]
    for cout, cin in R.UP2_CASES:
        wdy = R.dyadic((cout, cin, 3, 3), 1)
        for fn in (R.ref_wu, R.ref_wdd):
            assert torch.equal(fn(wdy).double(), fn(wdy.double()))  # every four-term sum exact in f32
    wn = R.normal((64, 40, 3, 3), 2)
    kx_major = sum(wn[:, :, ky, kx] for kx in (1, 2) for ky in (1, 2))  # the other order of the four-tap class (py, px, a, b) = (0, 0, 1, 1)
    assert not torch.equal(R.ref_wu(wn)[:64, 3, :40], torch.zeros(64, 40) + kx_major)
    assert bool((R.bits_of(R.ref_wu(-torch.zeros(1, 1, 3, 3), BF16)) == 0).all())  # a lone -0 tap sums to +0 (0.f + -0.f)


# ------------------------------------------------------------------------------------------------------------------ rounding
def test_bf16_conversion_is_round_to_nearest_even_on_the_tie_set():
    x = R.ties(BF16)
    bits = x.view(torch.int32).to(torch.int64) & 0xffffffff
    rule = ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16) & 0xffff
    got = R.bits_of(x.to(BF16)).to(torch.int64) & 0xffff
    assert torch.equal(got, rule)
    n = 3000
    mid = got[n:2 * n]
    assert bool((mid & 1 == 0).all())  # exact ties went to the even neighbour ...
    h = R.bits_of(x[3 * n:4 * n].to(BF16)).to(torch.int64) & 0xffff
    assert 0.4 < float((mid != h).double().mean()) < 0.6  # ... which is the upper one for about half of them
    assert torch.equal(got[:n], h) and torch.equal(got[2 * n:3 * n] & 0x7fff, (h & 0x7fff) + 1)  # mid - ulp down, mid + ulp up


def test_f16_conversion_is_ieee_on_the_tie_set():
    x = R.ties(F16)
    with np.errstate(over="ignore"):  # (65520 -> inf is one of the cases)
        want = torch.from_numpy(x.numpy().astype(np.float16).view(np.int16).copy())
    got = R.bits_of(x.to(F16))
    assert torch.equal(got, want)
    below = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))
    assert float(torch.tensor([below]).to(F16)) == 65504.0 and float(torch.tensor([65520.0]).to(F16)) == float("inf")
    assert float(torch.tensor([-65520.0]).to(F16)) == -float("inf")
    r = x.to(F16)
    sub = (r != 0) & (r.float().abs() < 2.0 ** -14)
    assert int(sub.sum()) >= 64 and bool(torch.isinf(r).sum() == 2)  # f16 subnormal results and the two overflows are in the set


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_truncation_differs_on_a_third_of_the_tie_set(dtype):
    x = R.ties(dtype)
    rne, trunc = R.bits_of(x.to(dtype)), R.bits_of(R.truncate(x, dtype))
    assert bool((R.truncate(x, dtype).float().abs() <= x.abs()).all())
    share = float((rne != trunc).double().mean())
    pos = x > 0
    n = 3000
    kind = torch.zeros(x.numel(), dtype=torch.bool)
    kind[n:3 * n] = True  # midpoints and midpoint + 1 ulp
    print(f"pack ties {R.DTYPE_NAME[dtype]}: truncation differs from round-to-nearest-even on {share:.3f} of {x.numel()} masters; "
          f"midpoints and midpoint + 1 ulp are {float((kind & pos).sum()) / float(pos.sum()):.3f} of the positive ones")
    assert share >= 1.0 / 3.0
    assert float((kind & pos).sum()) / float(pos.sum()) > 1.0 / 3.0
    # the moderate set (sub-pixel weights) and a master filled from the set keep that power
    for y in (R.ties(dtype, moderate=True), R.master(R.BY_NAME["a"], "ties", dtype), R.master(R.BY_NAME["j"], "ties", dtype)):
        if y.numel() >= 1000:
            assert float((R.bits_of(y.reshape(-1).to(dtype)) != R.bits_of(R.truncate(y.reshape(-1), dtype))).double().mean()) >= 1.0 / 3.0
    assert float(R.ties(dtype, moderate=True).abs().max()) < 2.0 ** 13 and float(R.ties(dtype, moderate=True).abs().min()) > 2.0 ** -13


# ------------------------------------------------------------------------------------------------------------------ Adam bounds
LR = 1e-4
N_ADAM = 1 << 20


def _adam_state(steps, seed=3):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(N_ADAM, generator=gen) * 0.1
    g = torch.randn(N_ADAM, generator=gen) * 1e-3
    if steps == 0:
        return p, g, torch.zeros(N_ADAM), torch.zeros(N_ADAM)
    m = torch.randn(N_ADAM, generator=gen) * 1e-3
    v = m * m * (0.5 + torch.rand(N_ADAM, generator=gen))  # a second moment of the size the first one implies
    return p, g, m, v


@pytest.mark.parametrize("steps", [0, 999])
@pytest.mark.parametrize("decay", [0.0, 1e-2])
@pytest.mark.parametrize("gs,scaler", [(1.0, None), (0.125, [4.0, 0.0, 0.0, 0.0])])
def test_f32_standin_stays_inside_the_adam_bounds(steps, decay, gs, scaler):
    p, g, m, v = _adam_state(steps)
    kw = dict(steps=steps, lr=LR, grad_scale=gs, scaler=scaler, decay=decay)
    ref = R.ref_adam_step(p, g, m, v, **kw)
    p1, m1, v1 = R.f32_adam_standin(p, g, m, v, **kw)
    r = R.adam_ratios(p1, m1, v1, ref, LR)
    print(f"pack adam stand-in t={steps + 1} decay={decay} gs={gs} scaler={scaler is not None}: worst ratio m {r['m']:.3f}  v {r['v']:.3f}  p {r['p']:.3f}")
    assert r["m"] <= 1.0 and r["v"] <= 1.0 and r["p"] <= 1.0, r
    if decay:  # the decay is seen: far outside the decay-0 reference
        p0 = R.ref_adam_step(p, g, m, v, **dict(kw, decay=0.0))[0]
        R.AR.check_decay_seen(p1, p0, 1, LR, f"stand-in t={steps + 1}")


@pytest.mark.parametrize("wrong,which", [("unscaled", "m"), ("gr_not_squared", "v"), ("t_not_plus_1", "p")])
def test_wrong_standins_land_outside(wrong, which):
    steps = 2
    p, g, m, v = _adam_state(steps)
    kw = dict(steps=steps, lr=LR, grad_scale=0.125, scaler=[4.0, 0.0, 0.0, 0.0], decay=1e-2)
    ref = R.ref_adam_step(p, g, m, v, **kw)
    good = R.adam_ratios(*R.f32_adam_standin(p, g, m, v, **kw), ref, LR)
    r = R.adam_ratios(*R.f32_adam_standin(p, g, m, v, wrong=wrong, **kw), ref, LR)
    print(f"pack adam wrong stand-in '{wrong}': {which} misses its bound by a factor {r[which]:.3g} (right stand-in: {good[which]:.3f})")
    assert good[which] <= 1.0 and r[which] > 100.0, (wrong, r)


def test_an_element_updated_twice_or_not_at_all_is_orders_outside():
    p, g, m, v = _adam_state(0)
    kw = dict(steps=0, lr=LR)
    ref = R.ref_adam_step(p, g, m, v, **kw)
    p1, m1, v1 = R.f32_adam_standin(p, g, m, v, **kw)
    p2, m2, v2 = R.f32_adam_standin(p1, g, m1, v1, **kw)
    assert R.adam_ratios(p, m, v, ref, LR)["p"] > 1000 and R.adam_ratios(p2, m2, v2, ref, LR)["p"] > 1000


def test_packer_is_outside_the_tuned_sources():
    from fal_net_amd import _build, _lib, ops
    assert "pack.hip" in _build.SOURCES
    assert "pack.hip" not in ops._TUNE_SOURCES and _lib.EXPECTED_VERSION == 600  # the packaged autotune cache stays valid
    for name in ("falnet_pack_weights", "falnet_pack_weights_batched", "falnet_pack_up2_batched", "falnet_adam_pack_batched", "falnet_adam_pack_batched_wd"):
        assert name in _lib.SIGNATURES
    assert _lib.C.sizeof(_lib.PackDesc) == 64 and _lib.C.sizeof(_lib.PackUp2Desc) == 48
