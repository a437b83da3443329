"""CPU: the float64 reference of one falnet_conv2d launch (tests/_conv_ref.py) against torch's composed ops, the autotune-cache key
parser against fal_net_amd.ops.conv_signature, and the element-wise gradient comparator (tests/_grad_parity.py) against the norm-only
check it replaces."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from fal_net_amd import _lib as L
from fal_net_amd import ops

import _conv_ref as R
from _grad_parity import grad_parity, norm_rel

f64 = torch.float64
CACHE = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "autotune_cache.json")


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _pack(w, taps):
    """OIHW [Cout][Cin][KH][KW] -> packed [Cout][KH*KW][Cin] with tap index kh * KW + kw (as falnet_pack_weights)."""
    co, ci, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(co, kh * kw, ci)


def _sig(B, srcs, IH, IW, taps, w_rows, stride, TH, TW, OH, OW, Cout, cst=None, layout=R.OUT_NHWC, step=(1, 0, 0), bias=False,
         addend=False, act=R.ACT_NONE, actout_kind=None, pool=None, pool_actout=False, out=True, w_taps=None):
    return {"dtype": 0, "srcs": srcs, "IH": IH, "IW": IW, "cin_total": sum(s["C"] for s in srcs), "taps": taps,
            "w_taps": w_taps or (max(t[2] for t in taps) + 1), "w_rows": w_rows, "stride": stride, "B": B, "TH": TH, "TW": TW,
            "osy": step[0], "ooy": step[1], "oox": step[2], "OH": OH, "OW": OW, "Cout": Cout,
            "out_cstride": Cout if cst is None else cst, "out_layout": layout, "bias": bias, "addend": addend, "act": act,
            "actout": actout_kind is not None, "actout_kind": actout_kind or 0, "pool": pool is not None, "pool_mode": pool or 0,
            "pool_actout": pool_actout, "pool_actout_kind": R.ACT_ELU if pool_actout else 0, "out": out, "ws": False, "up2": False}


def _src(t, bcast=False):
    if bcast:
        return {"C": t.shape[1], "H": 0, "W": 0, "bcast": True}
    return {"C": t.shape[3], "H": t.shape[1], "W": t.shape[2], "bcast": False}


def _close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12), float((a - b).abs().max())


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("ksize,stride", [(3, 1), (1, 1), ((3, 1), 1), ((1, 3), 1), (3, 2)])
def test_forward_single_source(ksize, stride):
    g = _g(7)
    B, Ci, Co, H, W = 2, 5, 6, 7, 9
    KH, KW = (ksize, ksize) if isinstance(ksize, int) else ksize
    x = torch.randn(B, Ci, H, W, generator=g, dtype=f64)
    w = torch.randn(Co, Ci, KH, KW, generator=g, dtype=f64)
    b = torch.randn(Co, generator=g, dtype=f64)
    ref = F.elu(F.conv2d(x, w, b, stride=stride, padding=(KH // 2, KW // 2)))
    OH, OW = ref.shape[2:]
    taps = ops.fwd_taps(ksize)
    sig = _sig(B, [_src(_nhwc(x))], H, W, taps, Co, stride, OH, OW, OH, OW, Co, bias=True, act=R.ACT_ELU)
    res = R.conv_ref(sig, [_nhwc(x)], _pack(w, taps), b)
    _close(res["ref"], _nhwc(ref))
    # the magnitude: the same sums over |x| |w|, plus |bias|
    mag = F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=(KH // 2, KW // 2))
    _close(res["mag"], _nhwc(mag))


def test_two_sources_upsampled_and_broadcast():
    """Concat of a nearest-upsampled source, a full-size source (FAL_netB.py:57-58, :145-173) -- and a per-sample constant plane
    (the `flow` input, ops.bcast_src), residual addend, ReLU and an ELU-gradient operand."""
    g = _g(11)
    B, H, W, Co = 2, 6, 8, 4
    low = torch.randn(B, 3, H // 2, W // 2, generator=g, dtype=f64)
    full = torch.randn(B, 2, H, W, generator=g, dtype=f64)
    w = torch.randn(Co, 5, 3, 3, generator=g, dtype=f64)
    add = torch.randn(B, Co, H, W, generator=g, dtype=f64)
    y = F.elu(torch.randn(B, Co, H, W, generator=g, dtype=f64))
    pre = F.conv2d(torch.cat([F.interpolate(low, scale_factor=2, mode="nearest"), full], 1), w, padding=1) + add
    ref = F.relu(pre) * torch.where(y > 0, torch.ones_like(y), y + 1)
    taps = ops.fwd_taps(3)
    sig = _sig(B, [_src(_nhwc(low)), _src(_nhwc(full))], H, W, taps, Co, 1, H, W, H, W, Co, addend=True, act=R.ACT_RELU,
               actout_kind=R.ACT_ELU)
    res = R.conv_ref(sig, [_nhwc(low), _nhwc(full)], _pack(w, taps), addend=_nhwc(add), actout=_nhwc(y))
    _close(res["ref"], _nhwc(ref))
    _close(res["mag"], _nhwc(F.conv2d(torch.cat([F.interpolate(low, scale_factor=2, mode="nearest"), full], 1).abs(), w.abs(),
                                      padding=1) + add.abs()))
    # broadcast source: a [B][1] constant per sample seen as an H x W plane (zero padded at the border like any input)
    c = torch.randn(B, 1, generator=g, dtype=f64)
    w2 = torch.randn(Co, 3, 3, 3, generator=g, dtype=f64)
    x2 = torch.randn(B, 2, H, W, generator=g, dtype=f64)
    plane = c.view(B, 1, 1, 1).expand(B, 1, H, W)
    ref2 = F.conv2d(torch.cat([x2, plane], 1), w2, padding=1)
    sig2 = _sig(B, [_src(_nhwc(x2)), {"C": 1, "H": H, "W": W, "bcast": True}], H, W, taps, Co, 1, H, W, H, W, Co)
    _close(R.conv_ref(sig2, [_nhwc(x2), c], _pack(w2, taps))["ref"], _nhwc(ref2))


def test_dgrad_stride1_and_stride2_parity_classes():
    """Data gradients as falnet_conv2d launches: stride 1 with ops.dgrad_taps_s1, stride 2 as the four parity classes of
    ops.dgrad_taps_s2 with out_step (2, py, px) -- each class writes only its own parity, the four together are autograd's result."""
    g = _g(5)
    B, Ci, Co = 2, 3, 4
    for H, W in ((7, 9), (8, 6)):
        w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=f64)
        wd = w.permute(1, 2, 3, 0).reshape(Ci, 9, Co)  # [ci][tap][co]
        x = torch.zeros(B, Ci, H, W, dtype=f64, requires_grad=True)
        go = torch.randn(B, Co, H, W, generator=g, dtype=f64)
        (F.conv2d(x, w, padding=1) * go).sum().backward()
        sig = _sig(B, [_src(_nhwc(go))], H, W, ops.dgrad_taps_s1(3), Ci, 1, H, W, H, W, Ci, w_taps=9)
        _close(R.conv_ref(sig, [_nhwc(go)], wd)["ref"], _nhwc(x.grad))
        # stride 2
        x.grad = None
        y = F.conv2d(x, w, stride=2, padding=1)
        OH, OW = y.shape[2:]
        go2 = torch.randn(B, Co, OH, OW, generator=g, dtype=f64)
        (y * go2).sum().backward()
        acc = torch.full((B, H, W, Ci), float("nan"), dtype=f64)
        for py in range(2):
            for px in range(2):
                TH, TW = (H - py + 1) // 2, (W - px + 1) // 2
                sig = _sig(B, [_src(_nhwc(go2))], OH, OW, ops.dgrad_taps_s2(py, px), Ci, 1, TH, TW, H, W, Ci, step=(2, py, px), w_taps=9)
                r = R.conv_ref(sig, [_nhwc(go2)], wd)["ref"]
                mapped = ~torch.isnan(r)
                assert mapped[:, py::2, px::2].all() and int(mapped.sum()) == B * TH * TW * Ci  # its own parity class, nothing else
                assert torch.isnan(acc[mapped]).all()
                acc[mapped] = r[mapped]
        _close(acc, _nhwc(x.grad))


def test_planar_output_and_channel_stride():
    g = _g(3)
    B, Ci, Co, H, W = 2, 4, 3, 5, 6
    x = torch.randn(B, Ci, H, W, generator=g, dtype=f64)
    w = torch.randn(8, Ci, 3, 3, generator=g, dtype=f64)  # 8 packed rows, 3 written
    b = torch.randn(8, generator=g, dtype=f64)
    ref = F.conv2d(x, w[:Co], b[:Co], padding=1)
    taps = ops.fwd_taps(3)
    sig = _sig(B, [_src(_nhwc(x))], H, W, taps, 8, 1, H, W, H, W, Co, cst=0, layout=R.OUT_PLANAR_F32, bias=True)
    _close(R.conv_ref(sig, [_nhwc(x)], _pack(w, taps), b)["ref"], ref)
    # NHWC with a channel stride beyond Cout: channels >= Cout are not mapped
    sig = _sig(B, [_src(_nhwc(x))], H, W, taps, 8, 1, H, W, H, W, Co, cst=8, bias=True)
    r = R.conv_ref(sig, [_nhwc(x)], _pack(w, taps), b)["ref"]
    assert torch.isnan(r[..., Co:]).all()
    _close(r[..., :Co], _nhwc(ref))


@pytest.mark.parametrize("mode,keep_out", [(0, True), (0, False), (1, False)])
def test_fused_pool(mode, keep_out):
    """pool mode 0: 2x2 max of the activated output (MaxPool2d(2, 2) after a VGG slice); mode 1: the 2x2 sum times elu'(pool_actout)
    (the adjoint of the nearest upsample in front of a deconv, fused into its data gradient)."""
    g = _g(17 + mode)
    B, Ci, Co, H, W = 2, 3, 4, 6, 8
    x = torch.randn(B, Ci, H, W, generator=g, dtype=f64)
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=f64)
    b = torch.randn(Co, generator=g, dtype=f64)
    v = F.conv2d(x, w, b, padding=1)
    taps = ops.fwd_taps(3)
    if mode == 0:
        v = F.relu(v)
        pref, pa, act = F.max_pool2d(v, 2, 2), None, R.ACT_RELU
    else:
        pa = F.elu(torch.randn(B, Co, H // 2, W // 2, generator=g, dtype=f64))
        pref, act = F.avg_pool2d(v, 2, 2) * 4 * torch.where(pa > 0, torch.ones_like(pa), pa + 1), R.ACT_NONE
    sig = _sig(B, [_src(_nhwc(x))], H, W, taps, Co, 1, H, W, H, W, Co, bias=True, act=act, pool=mode, pool_actout=pa is not None,
               out=keep_out)
    res = R.conv_ref(sig, [_nhwc(x)], _pack(w, taps), b, pool_actout=None if pa is None else _nhwc(pa))
    _close(res["pool_ref"], _nhwc(pref))
    if keep_out:
        _close(res["ref"], _nhwc(v))
    else:
        assert res["ref"] is None


def test_compare_flags_violations_and_stray_writes():
    ref = torch.tensor([[1.0, float("nan")], [2.0, -3.0]], dtype=f64)
    mag = torch.tensor([[10.0, float("nan")], [10.0, 10.0]], dtype=f64)
    got = ref.clone()
    got[0, 1] = float("nan")
    assert R.compare(got.float(), ref, mag, torch.float32)["bad"] == 0
    got[1, 0] += 1e-3  # far beyond 2^-21 |ref| + 1e-5 mag
    got[0, 1] = 0.0    # a write to an unmapped element
    rep = R.compare(got, ref, mag, torch.float32)
    assert rep["bad"] == 1 and rep["unmapped_written"] == 1 and rep["worst_ratio"] > 1
    got = ref.clone()
    got[1, 1] = float("nan")  # a mapped element never written
    assert R.compare(got, ref, mag, torch.float32)["bad"] == 1


def _cache_keys():
    with open(CACHE) as f:
        return [k for k in json.load(f) if k.startswith("conv|")]


def test_signature_round_trip_every_cache_key():
    """parse_signature is the inverse of ops.conv_signature on every committed `conv|` entry."""
    keys = _cache_keys()
    assert len(keys) > 600
    for key in keys:
        d = R.fill_desc(L.Conv(), R.parse_signature(key))
        assert ops.conv_signature(d) == key, key


def test_grad_parity_catches_what_the_norm_misses():
    """A gradient with its kh / kw taps transposed (or a flipped sign, or permuted channels) has the exact norm of the right one: the
    old norm check passes it, grad_parity does not."""
    g = _g(23)
    ref = {"conv.weight": torch.randn(8, 6, 3, 3, generator=g), "conv.bias": torch.randn(8, generator=g)}
    assert grad_parity(dict(ref), ref, norm_tol=2e-3)  # identical: passes
    wrongs = {
        "kh/kw transposed": ref["conv.weight"].transpose(2, 3).contiguous(),
        "sign flipped": -ref["conv.weight"],
        "output channels permuted": ref["conv.weight"][torch.randperm(8, generator=g)],
    }
    for what, bad in wrongs.items():
        assert norm_rel(bad, ref["conv.weight"]) < 1e-6, what  # the norm check is blind to it
        with pytest.raises(AssertionError):
            grad_parity({"conv.weight": bad, "conv.bias": ref["conv.bias"]}, ref, norm_tol=2e-3, what=what)
