"""Float64 reference of ONE falnet_conv2d launch, written from the descriptor semantics in include/falnet_hip.h (falnet_conv_t), not
from the kernels; and the parser of the autotune cache's launch signatures (the inverse of fal_net_amd.ops.conv_signature).

conv_ref() evaluates on the device of its operands (torch float64: one GEMM per tap over a gathered slice), so a GPU test runs it
through the BLAS library, which shares no code with the kernels under test.  It returns, in the launch's output layout (NHWC
[B][OH][OW][out_cstride] or planar [B][Cout][OH][OW]) with NaN wherever the descriptor maps no tile position:
  ref  -- the exact result on the operands AS STORED (the caller passes them already rounded to the launch dtype);
  mag  -- the same sums over |x| |w|, plus |bias| + |addend|: the scale the f32 accumulation error is bounded by;
and the same pair for the fused 2x2 pool (pool_ref / pool_mag, NHWC [B][OH/2][OW/2][out_cstride]) when the launch has one.
"""
import re

import torch

ACT_NONE, ACT_ELU, ACT_RELU = 0, 1, 2
OUT_NHWC, OUT_PLANAR_F32 = 0, 1
DTYPE_CODE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}

_KEY = re.compile(r"conv\|t(\d+)\|([^|]+)\|(\d+)x(\d+)\|k(\d+)\|([^|]+)\|w(\d+)x(\d+)\|s(\d+)\|B(\d+)\|(\d+)x(\d+)\|"
                  r"o(\d+),(\d+),(\d+)\|(\d+)x(\d+)\|c(\d+),(\d+),(\d+)\|f(\d{9})\|ws([01])(\|up2)?$")


def parse_signature(key):
    """`conv|...` autotune-cache key -> dict of the falnet_conv_t fields it fixes (pointers as presence flags)."""
    m = _KEY.match(key)
    if m is None:
        raise ValueError(f"not a conv launch signature: {key!r}")
    g = m.groups()
    srcs = []
    for s in g[1].split(";"):
        c, h, w, bc = (int(v) for v in s.split(","))
        srcs.append({"C": c, "H": h, "W": w, "bcast": bool(bc)})
    taps = [tuple(int(v) for v in t.split(":")) for t in g[5].split(",")]
    f = [int(ch) for ch in g[20]]
    return {
        "dtype": int(g[0]), "srcs": srcs, "IH": int(g[2]), "IW": int(g[3]), "cin_total": int(g[4]), "taps": taps,
        "w_taps": int(g[6]), "w_rows": int(g[7]), "stride": int(g[8]), "B": int(g[9]), "TH": int(g[10]), "TW": int(g[11]),
        "osy": int(g[12]), "ooy": int(g[13]), "oox": int(g[14]), "OH": int(g[15]), "OW": int(g[16]),
        "Cout": int(g[17]), "out_cstride": int(g[18]), "out_layout": int(g[19]),
        "bias": bool(f[0]), "addend": bool(f[1]), "act": f[2], "actout": bool(f[3]), "actout_kind": f[4],
        "pool": bool(f[5]), "pool_mode": f[6], "pool_actout": bool(f[7]), "out": bool(f[8]),
        "pool_actout_kind": ACT_ELU if f[7] else ACT_NONE,  # (not part of the key: the plans' pool_actout is always an ELU output)
        "ws": bool(int(g[21])), "up2": g[22] is not None,
    }


def fill_desc(d, sig, ptrs=None):
    """Fill a falnet_conv_t (fal_net_amd._lib.Conv) from parse_signature(); `ptrs` maps the pointer fields (src0, src1, weight, out,
    bias, addend, actout, pool_out, pool_actout, weight_up2, splitk_ws) to device addresses -- absent ones become 1 when the signature
    says the operand is present, else NULL (enough for conv_signature; a launch passes real ones).  Source strides: contiguous NHWC
    with C channels, or a per-sample constant [B][C] (strides 0)."""
    ptrs = ptrs or {}
    p = lambda name, present: ptrs.get(name, 1) if present else 0  # noqa: E731
    d.nsrc = len(sig["srcs"])
    for i, s in enumerate(sig["srcs"]):
        src = d.src[i]
        src.ptr, src.C, src.H, src.W = p(f"src{i}", True), s["C"], s["H"], s["W"]
        if s["bcast"]:
            src.sb, src.sy, src.sx = s["C"], 0, 0
        else:
            src.sb, src.sy, src.sx = s["H"] * s["W"] * s["C"], s["W"] * s["C"], s["C"]
    d.IH, d.IW = sig["IH"], sig["IW"]
    d.weight = p("weight", True)
    d.cin_total, d.w_taps, d.w_rows = sig["cin_total"], sig["w_taps"], sig["w_rows"]
    d.ntaps = len(sig["taps"])
    for t, (dy, dx, w) in enumerate(sig["taps"]):
        d.tap_dy[t], d.tap_dx[t], d.tap_w[t] = dy, dx, w
    d.isy = d.isx = sig["stride"]
    d.B, d.TH, d.TW = sig["B"], sig["TH"], sig["TW"]
    d.osy = d.osx = sig["osy"]
    d.ooy, d.oox = sig["ooy"], sig["oox"]
    d.out = p("out", sig["out"])
    d.OH, d.OW, d.Cout, d.out_cstride, d.out_layout = sig["OH"], sig["OW"], sig["Cout"], sig["out_cstride"], sig["out_layout"]
    d.bias = p("bias", sig["bias"])
    d.addend = p("addend", sig["addend"])
    d.act = sig["act"]
    d.actout = p("actout", sig["actout"])
    d.actout_kind = sig["actout_kind"]
    d.pool_out = p("pool_out", sig["pool"])
    d.pool_mode, d.pool_actout_kind = sig["pool_mode"], sig.get("pool_actout_kind", ACT_NONE)
    d.pool_actout = p("pool_actout", sig["pool_actout"])
    d.weight_up2 = p("weight_up2", sig["up2"])
    d.dtype = sig["dtype"]
    d.variant, d.ksplit = 0, 1
    d.splitk_ws = p("splitk_ws", sig["ws"])
    d.splitk_ws_bytes = ptrs.get("splitk_ws_bytes", 1) if sig["ws"] else 0
    return d


def act_fwd(v, act):
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    if act == ACT_RELU:
        return v.clamp_min(0)
    return v


def act_grad_from_out(y, kind):
    """d act / d pre from the activation OUTPUT y (ELU: y > 0 ? 1 : y + 1, ReLU: y > 0)."""
    if kind == ACT_ELU:
        return (y + 1).clamp(0, 1)
    if kind == ACT_RELU:
        return (y > 0).to(y.dtype)
    return torch.ones_like(y)


def _virtual_input(src, bcast, IH, IW):
    """[B][IH][IW][C] view of one source: a per-sample constant [B][C] broadcast, or NHWC nearest-upsampled to the launch size
    (F.interpolate(mode='nearest'): source index floor(i * H / IH))."""
    if bcast:
        B, Cc = src.shape
        return src.view(B, 1, 1, Cc).expand(B, IH, IW, Cc)
    _, H, W, _ = src.shape
    if (H, W) != (IH, IW):
        iy = torch.div(torch.arange(IH, device=src.device) * H, IH, rounding_mode="floor")
        ix = torch.div(torch.arange(IW, device=src.device) * W, IW, rounding_mode="floor")
        src = src[:, iy][:, :, ix]
    return src


def conv_ref(sig, srcs, weight, bias=None, addend=None, actout=None, pool_actout=None, want_mag=True):
    """Float64 result of one falnet_conv2d launch.  sig: parse_signature() dict (or the same keys); srcs: NHWC [B][H][W][C] tensors
    (or [B][C] for broadcast sources) in source order; weight: packed [w_rows][w_taps][cin_total]; bias: [>= Cout]; addend / actout:
    laid out like the output; pool_actout: like the pooled output.  Every operand is used as given (pass the stored values).
    Returns dict(ref, mag, pool_ref, pool_mag) -- the pool pair only when the launch pools, ref / mag None when it keeps no `out`."""
    f64 = torch.float64
    B, IH, IW, TH, TW = sig["B"], sig["IH"], sig["IW"], sig["TH"], sig["TW"]
    s, osy, ooy, oox = sig["stride"], sig["osy"], sig["ooy"], sig["oox"]
    OH, OW, Cout, cst, planar = sig["OH"], sig["OW"], sig["Cout"], sig["out_cstride"], sig["out_layout"] == OUT_PLANAR_F32
    assert sum(x["C"] for x in sig["srcs"]) == sig["cin_total"], "sources must fill the packed weight's K"
    dev = weight.device
    xin = torch.cat([_virtual_input(t.to(f64), x["bcast"], IH, IW)[..., :x["C"]] for t, x in zip(srcs, sig["srcs"])], dim=3)
    w = weight.to(f64)
    K = xin.shape[3]
    M = B * TH * TW
    acc = torch.zeros(M, Cout, dtype=f64, device=dev)
    mag = torch.zeros(M, Cout, dtype=f64, device=dev) if want_mag else None
    ty = torch.arange(TH, device=dev) * s
    tx = torch.arange(TW, device=dev) * s
    for dy, dx, tw in sig["taps"]:
        iy, ix = ty + dy, tx + dx
        my, mx = (iy >= 0) & (iy < IH), (ix >= 0) & (ix < IW)
        g = xin[:, iy.clamp(0, IH - 1)][:, :, ix.clamp(0, IW - 1)]
        g = g * (my.view(1, TH, 1, 1) & mx.view(1, 1, TW, 1)).to(f64)
        g = g.reshape(M, K)
        wt = w[:Cout, tw, :]  # [Cout][K]
        acc += g @ wt.t()
        if want_mag:
            mag += g.abs() @ wt.abs().t()
        del g
    oy = torch.arange(TH, device=dev) * osy + ooy
    ox = torch.arange(TW, device=dev) * osy + oox
    assert int(oy[-1]) < OH and int(ox[-1]) < OW, "tile space maps outside the output map"

    def at_out(t):  # operand laid out like the output -> [M][Cout] at the tile positions
        t = t.to(f64)
        if planar:
            t = t[:, :Cout].permute(0, 2, 3, 1)
        return t[:, oy][:, :, ox][..., :Cout].reshape(M, Cout)

    v = acc
    if sig["bias"]:
        bv = bias.to(f64)[:Cout]
        v = v + bv
        if want_mag:
            mag = mag + bv.abs()
    if sig["addend"]:
        a = at_out(addend)
        v = v + a
        if want_mag:
            mag = mag + a.abs()
    v = act_fwd(v, sig["act"])
    if sig["actout"]:
        v = v * act_grad_from_out(at_out(actout), sig["actout_kind"])

    def place(t):  # [M][Cout] -> the output layout, NaN where nothing is mapped
        if planar:
            o = torch.full((B, Cout, OH, OW), float("nan"), dtype=f64, device=dev)
            o[:, :, oy[:, None], ox[None, :]] = t.view(B, TH, TW, Cout).permute(0, 3, 1, 2)
        else:
            o = torch.full((B, OH, OW, cst), float("nan"), dtype=f64, device=dev)
            o[:, oy[:, None], ox[None, :], :Cout] = t.view(B, TH, TW, Cout)
        return o

    res = {"ref": None, "mag": None}
    if sig["out"]:
        res["ref"] = place(v)
        res["mag"] = place(mag) if want_mag else None
    if sig["pool"]:
        assert not planar and (osy, ooy, oox) == (1, 0, 0) and (TH, TW) == (OH, OW) and OH % 2 == 0 and OW % 2 == 0
        q = v.view(B, OH // 2, 2, OW // 2, 2, Cout)
        qm = mag.view(B, OH // 2, 2, OW // 2, 2, Cout) if want_mag else None
        if sig["pool_mode"] == 0:
            pv = q.amax(dim=(2, 4))
            pm = qm.amax(dim=(2, 4)) if want_mag else None
        else:
            pv = q.sum(dim=(2, 4))
            pm = qm.sum(dim=(2, 4)) if want_mag else None
        if sig["pool_actout"]:
            pv = pv * act_grad_from_out(pool_actout.to(f64)[..., :Cout], sig.get("pool_actout_kind", ACT_ELU))
        po = torch.full((B, OH // 2, OW // 2, cst), float("nan"), dtype=f64, device=dev)
        po[..., :Cout] = pv
        res["pool_ref"] = po
        if want_mag:
            pmo = torch.full_like(po, float("nan"))
            pmo[..., :Cout] = pm
            res["pool_mag"] = pmo
    return res


def unit_roundoff(out_dtype):
    """u of the stored output: 2^-8 (bf16), 2^-11 (f16), 2^-21 (f32 -- a few ulps of the f32 epilogue arithmetic)."""
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -21}[out_dtype]


def violations(got, ref, mag, out_dtype, mag_coef=1e-5):
    """Boolean tensor in the output layout: the mapped elements compare() counts as `bad` (where a fault shows, not only how often)."""
    mapped = ~torch.isnan(ref)
    r, m = torch.nan_to_num(ref), torch.nan_to_num(mag)
    ok = (got.to(torch.float64) - r).abs() <= unit_roundoff(out_dtype) * r.abs() + mag_coef * m  # a NaN in `got` fails here
    return mapped & ~ok


def compare(got, ref, mag, out_dtype, mag_coef=1e-5):
    """Element-wise check of a launch's output against conv_ref: mapped elements (ref not NaN) within u |ref| + mag_coef mag, unmapped
    ones still NaN (the sentinel the caller filled the buffer with).  Returns dict(bad, unmapped_written, worst_ratio, maxnorm_rel)."""
    got = got.to(torch.float64)
    mapped = ~torch.isnan(ref)
    r, m, g = ref[mapped], mag[mapped], got[mapped]
    bound = unit_roundoff(out_dtype) * r.abs() + mag_coef * m
    err = (g - r).abs()
    ok = err <= bound  # a NaN in `got` fails here
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bound.clamp_min(1e-300))
    return {
        "bad": int((~ok).sum()),
        "unmapped_written": int((~torch.isnan(got[~mapped])).sum()),
        "worst_ratio": float(ratio.max()) if ratio.numel() else 0.0,
        "maxnorm_rel": float(err.max() / r.abs().max().clamp_min(1e-300)) if r.numel() else 0.0,
        "mapped": int(mapped.sum()),
    }
