"""Ragged-shape cases of falnet_conv2d shared by tests/test_conv_edges_host.py (CPU) and tests/test_gpu_conv_edges.py (GPU).

The committed autotune cache pins 675 launches at B in {8, 16} on even maps of the benchmark's sizes; the tile heights in use are 4, 8, 16
and 32 rows by 32 columns.  The cases here are the smallest maps with a partial last tile row for each height, a partial (down to 1-pixel)
last tile column and odd sizes, at B in {1, 2, 3, 6}.  A case is a high-level description of ONE operation (forward conv, data gradient, ...)
from which
  * sigs(case, dtype)      gives the launch signature(s) (tests/_conv_ref.py: parse_signature-style dicts) -- what the kernels see;
  * operands(case, dtype)  gives the seeded randn operands, rounded to the launch dtype before any reference sees them (CPU tensors);
  * torch_ref(case, ops)   gives the same operation composed from torch's own ops in float64 (F.conv2d / F.interpolate / autograd),
                           which the host test holds conv_ref to: the tap tables are tied to torch, not to fal_net_amd.ops.
EXPECT pins, per (launch, 16- or 32-bit), every (variant) choose_conv_kernel accepts; the host test holds the library to it, the GPU test
runs exactly those and takes any other return code than 0 as a failure.

What the dispatch itself limits (falnet_conv2d_kernel_name / falnet_conv_s2d_dma_applicable, read on the CPU):
  * variant 14 takes even maps only, so the odd 47 x 141 data gradient (P) runs as single and fused gather launches and P14 is the
    smallest even map with partial tiles in both directions for variant 14; P's groups have 32 weight rows, so variant 12 (64 channels per
    workgroup) is reached through P14's 64;
  * variant 19 at K's 128 input channels has one slice width (128 / 64 = 2 slices is not a multiple of 4): both widths run at J;
  * the gather kernels accept variant 26's descriptor but compute another operation on it (RUN_ONLY below)."""
import torch
import torch.nn.functional as F

from fal_net_amd import ops

import _conv_ref as R

f64 = torch.float64
H16 = (torch.bfloat16, torch.float16)
ALL = (torch.bfloat16, torch.float16, torch.float32)
DT_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
VARIANTS = list(range(0, 14)) + list(range(15, 28)) + [29]  # every single-launch variant of include/falnet_hip.h (14 is falnet_conv2d_multi's)
# rows of a tile per variant (32 columns each); None: the gather kernels tile the flattened position index (128 positions per workgroup),
# 19 takes whole maps, 27 / 29 stream strips of 32 / 16 columns
TILE_H = {0: None, 1: None, 11: None, 12: None, 2: 8, 3: 8, 4: 8, 5: 8, 6: 16, 7: 16, 8: 4, 9: 4, 10: 8, 16: 4, 13: 16, 17: 4, 20: 8, 21: 16, 22: 32,
          23: 16, 24: 4, 25: 8, 15: 8, 18: 32, 26: 16, 19: None, 27: None, 29: None}  # (18: 16 low-resolution rows = 32 output rows)
UP2D_TAPS = [(0, 0, 0), (0, 1, 1), (1, 0, 2), (1, 1, 3)]  # = fal_net_amd.ops.UP2D_TAPS (asserted by the host test)


def pad(c):
    return (c + 31) // 32 * 32


def _fwd(name, note, B, H, W, srcs, cout, ksize=3, stride=1, bias=False, addend=None, act=R.ACT_NONE, planar=False, pool=None, up2=False,
         dtypes=H16, seed=0):
    """Forward convolution, 'same' padding.  srcs: [(C, how)], how in full / half (nearest-upsampled 2x inside the launch) / bcast (a per-sample
    constant); addend: None / 'sep' / 'alias' (the addend IS `out`: accumulate); pool: None / 'keep' / 'drop' (fused 2x2 max, `out` kept or NULL);
    up2: a `deconv` layer with sub-pixel weights (variant 18 among the candidates; master weights on the 1/64 grid)."""
    return dict(name=name, note=note, op="fwd", B=B, H=H, W=W, srcs=srcs, cout=cout, ksize=ksize, stride=stride, bias=bias, addend=addend, act=act,
                planar=planar, pool=pool, up2=up2, dtypes=dtypes, seed=seed)


def _dgrad1(name, note, B, H, W, K, cin_groups, group, pool=False, seed=0):
    """Stride-1 3x3 data gradient of a conv with `K` (padded) output channels w.r.t. concat group `group` of its input (weight = that group's rows
    of wd), times elu'(actout).  pool: the deconv adjoint -- 2x2 block sums times elu'(pool_actout), the full-resolution map not stored."""
    return dict(name=name, note=note, op="dgrad1", B=B, H=H, W=W, K=K, cin_groups=cin_groups, group=group, pool=pool, dtypes=H16, seed=seed)


def _dgrad2(name, note, B, H, W, K, cin, seed=0):
    """Stride-2 3x3 pad-1 data gradient w.r.t. a `cin`-channel input of H x W: four output-parity classes, + addend, times elu'(actout)."""
    return dict(name=name, note=note, op="dgrad2", B=B, H=H, W=W, K=K, cin=cin, dtypes=H16, seed=seed)


def _up2d(name, note, B, h, w, cin, cout, seed=0):
    """Data gradient of a `deconv` layer (nearest 2x + 3x3 conv, cin -> cout) on the low-resolution h x w grid (variant 26), times elu'(actout)."""
    return dict(name=name, note=note, op="up2d", B=B, h=h, w=w, cin=cin, cout=cout, dtypes=H16, seed=seed)


ELU, RELU, NONE = R.ACT_ELU, R.ACT_RELU, R.ACT_NONE
CASES = [
    _fwd("A", "21 rows: partial last tile row for heights 4, 8, 16; 75 columns: 11-pixel last column; bias + separate addend + ELU",
         2, 21, 75, [(64, "full")], 64, bias=True, addend="sep", act=ELU, dtypes=ALL, seed=101),
    _fwd("B", "37 rows: partial last row for all four heights (32 included); 70 columns; the addend aliases out (accumulate)",
         1, 37, 70, [(128, "full")], 128, addend="alias", act=ELU, seed=102),
    _fwd("C", "two sources, 49 output channels below the 64-row pad (zero weight rows), odd batch", 3, 21, 75, [(32, "full"), (32, "full")], 49,
         bias=True, dtypes=ALL, seed=103),
    _fwd("D", "32 -> 32: the wave-streaming kernel's launch; 13 x 45: one partial 16-row range, 13-pixel last strip", 2, 13, 45, [(32, "full")], 32,
         bias=True, act=ELU, seed=104),
    _fwd("D2", "32 -> 32 with a residual: 5 rows, a 1-pixel last strip", 1, 5, 33, [(32, "full")], 32, addend="sep", act=ELU, seed=124),
    _fwd("E", "5 x 33: one ragged 1-pixel column, 256 channels (gather with split-K)", 1, 5, 33, [(256, "full")], 256, bias=True, act=ELU,
         dtypes=ALL, seed=105),
    _fwd("F", "fused nearest upsample (17 x 33 -> 34 x 66) + concat; 34 rows: 2-row last tile at every height, 2-pixel last column",
         2, 34, 66, [(64, "half"), (32, "full")], 64, bias=True, act=ELU, seed=106),
    _fwd("Fb", "as F with the second source a per-sample constant plane", 2, 34, 66, [(64, "half"), (32, "bcast")], 64, bias=True, act=ELU, seed=107),
    _fwd("G", "64 -> 3 planar f32 (the VGG adjoint's last launch): 19 rows, 70 columns = 6-pixel last 16-column strip", 2, 19, 70, [(64, "full")], 3,
         planar=True, seed=108),
    _fwd("G2", "64 -> 3 planar f32 on 5 x 17: a 1-pixel last strip", 1, 5, 17, [(64, "full")], 3, bias=True, planar=True, seed=128),
    _fwd("H", "stride 2 from an odd 47 x 141 map, two sources: 24 x 71 outputs (7-pixel last column)", 2, 47, 141, [(32, "full"), (32, "full")], 64,
         stride=2, bias=True, act=ELU, dtypes=ALL, seed=109),
    _fwd("I", "stride 2, 33 x 130 -> 17 x 65: 1-row last tile, 1-pixel last column, 96 output channels", 1, 33, 130, [(128, "full")], 96, stride=2,
         act=ELU, seed=110),
    _fwd("J", "deep level, stride 2: 16 x 32 -> 8 x 16 (one image per 128-position tile), ragged batch of 6", 6, 16, 32, [(256, "full")], 512, stride=2,
         bias=True, act=ELU, seed=111),
    _fwd("K", "deep level: 4 x 8 maps, four images per tile and three in the batch (a partly filled tile)", 3, 4, 8, [(128, "full")], 64, act=ELU,
         seed=112),
    _fwd("M", "fused 2x2 max pool with out kept: 22 x 70 (even, partial rows for 4 / 8 / 16, 6-pixel last column)", 2, 22, 70, [(64, "full")], 64,
         bias=True, act=RELU, pool="keep", seed=113),
    _fwd("Md", "fused 2x2 max pool with out = NULL", 2, 22, 70, [(64, "full")], 64, bias=True, act=RELU, pool="drop", seed=114),
    _dgrad1("N0", "stride-1 data gradient of C w.r.t. its first concat group", 3, 21, 75, 64, [32, 32], 0, seed=115),
    _dgrad1("N1", "... w.r.t. its second concat group (weight rows 32..63 of wd)", 3, 21, 75, 64, [32, 32], 1, seed=116),
    _dgrad1("O", "deconv adjoint: stride-1 data gradient with the fused 2x2 sum and elu'(pool_actout), 22 x 70 -> 11 x 35", 2, 22, 70, 64, [64], 0,
            pool=True, seed=117),
    _dgrad2("P", "stride-2 data gradient of H's first group at the odd 47 x 141 input: classes of 24x71, 24x70, 23x71, 23x70 positions",
            2, 47, 141, 64, 32, seed=118),
    _dgrad2("P14", "the same for a 64-channel input on an even 34 x 70 map (variant 14 takes even maps only): 17 x 35 gout, 1-row / 3-pixel partial tiles",
            2, 34, 70, 64, 64, seed=119),
    _fwd("Q1", "deconv forward, low-res 9 x 40 (96 -> 49): 18 x 80 outputs", 2, 18, 80, [(96, "half")], 49, bias=True, act=ELU, up2=True, seed=120),
    _fwd("Q2", "deconv forward, low-res 5 x 33 (256 -> 128): a 1-pixel low-res column", 3, 10, 66, [(256, "half")], 128, bias=True, up2=True, seed=121),
    _up2d("R1", "deconv data gradient at low-res 17 x 40 (96 <- 49): 1-row last tile, 8-pixel last column", 2, 17, 40, 96, 49, seed=122),
    _up2d("R2", "deconv data gradient at low-res 16 x 33 (256 <- 128): 1-pixel last column", 1, 16, 33, 256, 128, seed=123),
    _fwd("S1", "1x1, 49 -> 49 at 6 x 40", 1, 6, 40, [(49, "full")], 49, ksize=1, bias=True, dtypes=ALL, seed=125),
    _fwd("S2", "3x1, 64 -> 64 at 12 x 40", 2, 12, 40, [(64, "full")], 64, ksize=(3, 1), act=ELU, dtypes=ALL, seed=126),
    _fwd("S3", "1x3 + residual, 128 -> 128 at 9 x 21", 1, 9, 21, [(128, "full")], 128, ksize=(1, 3), addend="sep", act=ELU, dtypes=ALL, seed=127),
]
BY_NAME = {c["name"]: c for c in CASES}
# falnet_conv3x3_c3 (its own entry point, no variants): B, H, W, Cout, act
C3_CASES = [(B, H, W, cout, act) for B, H, W in ((1, 9, 13), (2, 37, 70)) for cout in (32, 64) for act in (ELU, RELU)]


def base_sig(dt, srcs, IH, IW, taps, w_taps, w_rows, stride, B, TH, TW, OH, OW, Cout, cst, **kw):
    sig = {"dtype": DT_CODE[dt], "srcs": srcs, "IH": IH, "IW": IW, "cin_total": sum(s["C"] for s in srcs), "taps": [tuple(t) for t in taps],
           "w_taps": w_taps, "w_rows": w_rows, "stride": stride, "B": B, "TH": TH, "TW": TW, "osy": 1, "ooy": 0, "oox": 0, "OH": OH, "OW": OW,
           "Cout": Cout, "out_cstride": cst, "out_layout": R.OUT_NHWC, "bias": False, "addend": False, "act": NONE, "actout": False,
           "actout_kind": NONE, "pool": False, "pool_mode": 0, "pool_actout": False, "pool_actout_kind": NONE, "out": True, "ws": True, "up2": False}
    sig.update(kw)
    if sig["pool_actout"]:
        sig["pool_actout_kind"] = ELU
    return sig


def sigs(case, dt):
    """[(label, signature)] of the launches of `case` in dtype `dt` (one, or the four parity classes of a stride-2 data gradient).  `ws`: the
    split-K workspace as ops.conv_call attaches it (NHWC output, no fused pool)."""
    c = case
    if c["op"] == "fwd":
        srcs = []
        for C, how in c["srcs"]:
            hh, ww = (c["H"] // 2, c["W"] // 2) if how == "half" else (c["H"], c["W"])
            srcs.append({"C": pad(C), "H": hh, "W": ww, "bcast": how == "bcast"})
        s = c["stride"]
        OH, OW = (c["H"] + s - 1) // s, (c["W"] + s - 1) // s
        taps = ops.fwd_taps(c["ksize"])
        rows = pad(c["cout"])
        Cout, cst, layout = (c["cout"], 0, R.OUT_PLANAR_F32) if c["planar"] else (rows, rows, R.OUT_NHWC)
        return [("", base_sig(dt, srcs, c["H"], c["W"], taps, len(taps), rows, s, c["B"], OH, OW, OH, OW, Cout, cst, out_layout=layout,
                               bias=c["bias"], addend=c["addend"] is not None, act=c["act"], pool=c["pool"] is not None, out=c["pool"] != "drop",
                               ws=not c["planar"] and c["pool"] is None, up2=c["up2"]))]
    if c["op"] == "dgrad1":
        rows = pad(c["cin_groups"][c["group"]])
        src = [{"C": c["K"], "H": c["H"], "W": c["W"], "bcast": False}]
        kw = dict(pool=True, pool_mode=1, pool_actout=True, out=False, ws=False) if c["pool"] else dict(actout=True, actout_kind=ELU)
        return [("", base_sig(dt, src, c["H"], c["W"], ops.dgrad_taps_s1(3), 9, rows, 1, c["B"], c["H"], c["W"], c["H"], c["W"], rows, rows, **kw))]
    if c["op"] == "dgrad2":
        H, W = c["H"], c["W"]
        GH, GW = (H + 1) // 2, (W + 1) // 2
        src = [{"C": c["K"], "H": GH, "W": GW, "bcast": False}]
        rows = pad(c["cin"])
        out = []
        for py in range(2):
            for px in range(2):
                sig = base_sig(dt, src, GH, GW, ops.dgrad_taps_s2(py, px), 9, rows, 1, c["B"], (H - py + 1) // 2, (W - px + 1) // 2, H, W, rows, rows,
                                addend=True, actout=True, actout_kind=ELU)
                sig.update(osy=2, ooy=py, oox=px)
                out.append((f"/{py}{px}", sig))
        return out
    if c["op"] == "up2d":
        h, w, Kp, rows = c["h"], c["w"], pad(c["cout"]), pad(c["cin"])
        src = [{"C": Kp, "H": 2 * h, "W": 2 * w, "bcast": False}]
        sig = base_sig(dt, src, 2 * h, 2 * w, UP2D_TAPS, 4, rows, 1, c["B"], h, w, h, w, rows, rows, actout=True, actout_kind=ELU)
        sig["cin_total"] = 4 * Kp  # the packed wdd row: four summed-tap tiles of Kp channels
        return [("", sig)]
    raise ValueError(c["op"])


def up2d_plain_sig(sig):
    """The plain form of a variant-26 launch, for the reference: the 3x3 stride-1 data gradient at 2h x 2w with the 2x2 sums and elu'(pool_actout)
    in the epilogue (pool_mode 1), full-resolution map not stored."""
    s = dict(sig)
    s.update(taps=[tuple(t) for t in ops.dgrad_taps_s1(3)], w_taps=9, cin_total=sig["srcs"][0]["C"], TH=sig["IH"], TW=sig["IW"], OH=sig["IH"],
             OW=sig["IW"], actout=False, actout_kind=NONE, pool=True, pool_mode=1, pool_actout=sig["actout"], pool_actout_kind=ELU, out=False, ws=False)
    return s


def _elu(t):
    return torch.where(t > 0, t, torch.expm1(t))


def _grid_weight(g, *shape):
    """Master weights on the 1/64 grid below 1/4 in magnitude: they, and the sums of up to four of them the sub-pixel packings form, are exact in
    bf16 and f16."""
    return torch.randint(-16, 17, shape, generator=g).float() / 64


def operands(case, dt):
    """Seeded operands of `case`, rounded to `dt` (bias stays f32), as CPU tensors in the layouts the launch reads:
    srcs, w (OIHW master weight, as rounded), weight (the packed operand of the plain form), bias, addend, actout, pool_actout."""
    c = case
    g = torch.Generator().manual_seed(c["seed"])
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dt)  # noqa: E731
    o = dict(bias=None, addend=None, actout=None, pool_actout=None)
    B = c["B"]
    if c["op"] == "fwd":
        sig = sigs(c, dt)[0][1]
        o["srcs"] = []
        for (C, how), s in zip(c["srcs"], sig["srcs"]):
            t = rnd(B, s["C"]) if s["bcast"] else rnd(B, s["H"], s["W"], s["C"])
            t[..., C:] = 0  # padding channels of a source
            o["srcs"].append(t)
        cin_real = [C for C, _ in c["srcs"]]
        KH, KW = (c["ksize"], c["ksize"]) if isinstance(c["ksize"], int) else c["ksize"]
        K = sig["cin_total"]
        if c["up2"]:
            w = _grid_weight(g, c["cout"], sum(cin_real), 3, 3)
        else:
            w = rnd(c["cout"], sum(cin_real), KH, KW, scale=(1.0 / (KH * KW * K)) ** 0.5).float()
        o["w"] = w
        # packed [rows][taps][K]: rows >= cout and the padding channels of every concat group are zero (falnet_pack_weights)
        wf = torch.zeros(sig["w_rows"], KH * KW, K)
        k_real = k_pad = 0
        for C in cin_real:
            wf[:c["cout"], :, k_pad:k_pad + C] = w[:, k_real:k_real + C].permute(0, 2, 3, 1).reshape(c["cout"], KH * KW, C)
            k_real, k_pad = k_real + C, k_pad + pad(C)
        o["weight"] = wf.to(dt)
        if c["bias"]:
            o["bias"] = torch.zeros(sig["w_rows"])
            o["bias"][:c["cout"]] = torch.randn(c["cout"], generator=g) * 0.3
        oshape = (B, c["cout"], sig["OH"], sig["OW"]) if c["planar"] else (B, sig["OH"], sig["OW"], sig["out_cstride"])
        if c["addend"]:
            o["addend"] = rnd(*oshape)
            o["addend"][..., c["cout"]:] = 0
        return o
    if c["op"] == "dgrad1":
        cin = sum(c["cin_groups"])
        o["w"] = w = rnd(c["K"], cin, 3, 3, scale=(1.0 / (9 * c["K"])) ** 0.5).float()
        wd = w.permute(1, 2, 3, 0).reshape(cin, 9, c["K"])  # [ci][tap][co]
        r0 = sum(c["cin_groups"][:c["group"]])
        rows = c["cin_groups"][c["group"]]
        o["weight_full"], o["row0"] = wd.to(dt).contiguous(), r0  # (the reshape of the permuted tensor is a VIEW: the launch reads memory)
        o["weight"] = o["weight_full"][r0:r0 + rows]
        o["srcs"] = [rnd(B, c["H"], c["W"], c["K"])]
        if c["pool"]:
            o["pool_actout"] = _elu(torch.randn(B, c["H"] // 2, c["W"] // 2, rows, generator=g)).to(dt)
        else:
            o["actout"] = _elu(torch.randn(B, c["H"], c["W"], rows, generator=g)).to(dt)
        return o
    if c["op"] == "dgrad2":
        GH, GW = (c["H"] + 1) // 2, (c["W"] + 1) // 2
        o["w"] = w = rnd(c["K"], c["cin"], 3, 3, scale=(1.0 / (4 * c["K"])) ** 0.5).float()
        o["weight"] = w.permute(1, 2, 3, 0).reshape(c["cin"], 9, c["K"]).to(dt).contiguous()
        o["srcs"] = [rnd(B, GH, GW, c["K"])]
        o["addend"] = rnd(B, c["H"], c["W"], c["cin"])
        o["actout"] = _elu(torch.randn(B, c["H"], c["W"], c["cin"], generator=g)).to(dt)
        return o
    if c["op"] == "up2d":
        Kp, rows = pad(c["cout"]), pad(c["cin"])
        o["w"] = w = _grid_weight(g, c["cout"], c["cin"], 3, 3)
        wd = torch.zeros(rows, 9, Kp)
        wd[:c["cin"], :, :c["cout"]] = w.permute(1, 2, 3, 0).reshape(c["cin"], 9, c["cout"])
        o["weight"] = wd.to(dt)  # the plain 3x3 data-gradient operand (PackedConv.wd); the launch reads PackedConv.wdd
        o["srcs"] = [rnd(B, 2 * c["h"], 2 * c["w"], Kp)]
        o["srcs"][0][..., c["cout"]:] = 0
        o["actout"] = _elu(torch.randn(B, c["h"], c["w"], rows, generator=g)).to(dt)
        o["actout"][..., c["cin"]:] = 0
        return o
    raise ValueError(c["op"])


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _elu_grad(y):
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def torch_ref(case, o):
    """The operation of `case` on the operands `o` composed from torch's own float64 ops; returns the tensors conv_ref's `ref` (NHWC over the real
    channels, or planar) and / or `pool_ref` must equal: dict(out=..., pool=...)."""
    c = case
    d = lambda t: t.to(f64)  # noqa: E731
    if c["op"] == "fwd":
        xs = []
        for (C, how), t in zip(c["srcs"], o["srcs"]):
            if how == "bcast":
                x = d(t)[:, :C].view(c["B"], C, 1, 1).expand(c["B"], C, c["H"], c["W"])
            else:
                x = _nchw(d(t))[:, :C]
                if how == "half":
                    x = F.interpolate(x, scale_factor=2, mode="nearest")
            xs.append(x)
        KH, KW = (c["ksize"], c["ksize"]) if isinstance(c["ksize"], int) else c["ksize"]
        w = d(o["w"].to(o["weight"].dtype))
        y = F.conv2d(torch.cat(xs, 1), w, None if o["bias"] is None else d(o["bias"])[:c["cout"]], stride=c["stride"], padding=(KH // 2, KW // 2))
        if o["addend"] is not None:
            y = y + (d(o["addend"]) if c["planar"] else _nchw(d(o["addend"]))[:, :c["cout"]])
        y = F.elu(y) if c["act"] == ELU else F.relu(y) if c["act"] == RELU else y
        res = {"out": y if c["planar"] else _nhwc(y)}
        if c["pool"]:
            res["pool"] = _nhwc(F.max_pool2d(y, 2, 2))
        return res
    w = d(o["w"].to(o["weight"].dtype))
    go = _nchw(d(o["srcs"][0]))[:, :w.shape[0]]
    if c["op"] == "dgrad1":
        cin, r0, rows = sum(c["cin_groups"]), o["row0"], c["cin_groups"][c["group"]]
        if c["pool"]:  # deconv: nearest 2x, then the conv
            x = torch.zeros(c["B"], cin, c["H"] // 2, c["W"] // 2, dtype=f64, requires_grad=True)
            (F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1) * go).sum().backward()
            return {"pool": _nhwc(x.grad[:, r0:r0 + rows]) * _elu_grad(d(o["pool_actout"]))}
        x = torch.zeros(c["B"], cin, c["H"], c["W"], dtype=f64, requires_grad=True)
        (F.conv2d(x, w, padding=1) * go).sum().backward()
        return {"out": _nhwc(x.grad[:, r0:r0 + rows]) * _elu_grad(d(o["actout"]))}
    if c["op"] == "dgrad2":
        x = torch.zeros(c["B"], c["cin"], c["H"], c["W"], dtype=f64, requires_grad=True)
        (F.conv2d(x, w, stride=2, padding=1) * go).sum().backward()
        return {"out": (_nhwc(x.grad) + d(o["addend"])) * _elu_grad(d(o["actout"]))}
    if c["op"] == "up2d":
        x = torch.zeros(c["B"], c["cin"], c["h"], c["w"], dtype=f64, requires_grad=True)
        (F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1) * go).sum().backward()
        return {"pool": _nhwc(x.grad) * _elu_grad(d(o["actout"]))[..., :c["cin"]]}
    raise ValueError(c["op"])


def launches(dtypes=None):
    """Every (case, dtype) of the table."""
    return [(c, dt) for c in CASES for dt in c["dtypes"] if dtypes is None or dt in dtypes]


def bits(dt):
    return 32 if dt == torch.float32 else 16


# Accepted variants per (launch label, operand width), as falnet_conv2d_kernel_name answers on the descriptor of sigs() with scratch set for
# variant 19 (ksplit = cin_total / 32, and / 64 where that is a multiple of 4 too).  The two 16-bit types always agree.
EXPECT = {
    ("A", 16): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21, 23, 24, 25],
    ("A", 32): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12],
    ("B", 16): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 17, 20, 21, 22, 23, 24, 25],
    ("C", 16): [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21, 23, 24, 25],
    ("C", 32): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12],
    ("D", 16): [0, 1, 4, 9, 10, 11, 16, 17, 20, 24, 25, 27],
    ("D2", 16): [0, 1, 4, 9, 10, 11, 16, 17, 24, 27],
    ("E", 16): [0, 1, 2, 3, 4, 5, 8, 9, 11, 12, 17, 24],
    ("E", 32): [0, 1, 2, 3, 4, 5, 8, 9, 11, 12],
    ("F", 16): [0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 17, 20, 21, 22, 23, 24, 25],
    ("Fb", 16): [0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 17, 20, 21, 22, 23, 24, 25],
    ("G", 16): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 16, 17, 20, 23, 29],
    ("G2", 16): [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 29],
    ("H", 16): [0, 1, 11, 12, 15],
    ("H", 32): [0, 1, 11, 12],
    ("I", 16): [0, 1, 11, 15],
    ("J", 16): [0, 1, 11, 12, 19],
    ("K", 16): [0, 1, 11, 12, 19],
    ("M", 16): [0, 2, 3, 4, 5, 6, 7, 10, 13, 16, 21, 23],
    ("Md", 16): [0, 2, 3, 4, 5, 6, 7, 10, 13, 16, 21, 23],
    ("N0", 16): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 16, 17, 20, 21, 23, 24, 25],
    ("N1", 16): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 16, 17, 20, 21, 23, 24, 25],
    ("O", 16): [0, 2, 3, 4, 5, 6, 7, 10, 13, 16, 21, 23],
    ("P/00", 16): [0, 1, 11],
    ("P/01", 16): [0, 1, 11],
    ("P/10", 16): [0, 1, 11],
    ("P/11", 16): [0, 1, 11],
    ("P14/00", 16): [0, 1, 11, 12],
    ("P14/01", 16): [0, 1, 11, 12],
    ("P14/10", 16): [0, 1, 11, 12],
    ("P14/11", 16): [0, 1, 11, 12],
    ("Q1", 16): [0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 17, 18, 20, 21, 23, 24, 25],
    ("Q2", 16): [0, 1, 2, 3, 4, 5, 8, 9, 11, 12, 17, 18, 20, 24, 25],
    ("R1", 16): [0, 1, 11, 26],
    ("R2", 16): [0, 1, 11, 12, 26],
    ("S1", 16): [0, 1, 11, 12],
    ("S1", 32): [0, 1, 11, 12],
    ("S2", 16): [0, 1, 11, 12],
    ("S2", 32): [0, 1, 11, 12],
    ("S3", 16): [0, 1, 11, 12],
    ("S3", 32): [0, 1, 11, 12],
}

SPLITK_CASES = ("E", "J", "K", "P", "P14")  # the gather variants also run with ksplit = 4: small maps with many channels, stride-2 data gradients
# variant 26's descriptor (w_taps = 4, cin_total = 4 C over ONE C-channel source) is the data gradient only as variant 26 reads it: the gather
# kernels accept the descriptor but walk C of every tap's 4 C weight columns -- another operation, which ops.deconv_dgrad_call never launches
RUN_ONLY = {"R1": (26,), "R2": (26,)}


def deep_ksplits(sig):
    """Variant 19's slice counts for this launch: cin_total / 32 and / 64 where that is a multiple of 4 (include/falnet_hip.h: ksplit)."""
    return [k for k in (sig["cin_total"] // 32, sig["cin_total"] // 64) if k >= 4 and k % 4 == 0]


def choices(case, label, sig, dt):
    """(variant, ksplit) launches the GPU test runs for one launch of the table: every EXPECT variant, the gather ones also split-K on
    SPLITK_CASES, variant 19 at every slice width."""
    out = []
    for v in EXPECT[(case["name"] + label, bits(dt))]:
        if case["name"] in RUN_ONLY and v not in RUN_ONLY[case["name"]]:
            continue
        if v == 19:
            out += [(19, k) for k in deep_ksplits(sig)]
            continue
        out.append((v, 1))
        if v in (1, 11, 12) and case["name"] in SPLITK_CASES:
            out.append((v, 4))
    return out
