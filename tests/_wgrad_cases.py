"""The exact weight-gradient cases of tests/test_gpu_wgrad.py and tests/_wgrad_det.py, and the runner that takes ONE falnet_wgrad launch
through the C ABI (fal_net_amd._lib.Wgrad filled by fal_net_amd.ops._fill_wgrad, the variant forced on the descriptor) and holds it to
tests/_wgrad_ref.py with torch.equal: operands are small integers, so every f32 sum is exact (see _wgrad_ref.py).

A case is a dict (see _c): the kernel instantiation it reaches (`kernel`, named in the test ids; KERNEL_TABLE), the variant forced, the
shape, the source forms and the split counts.  The module imports without a GPU; the CPU tests check the exactness condition of every
case and that every kernel has a case whose largest |dW| is at least 4096 (a 16-bit intermediate could not pass).

Source forms: "nhwc" at the launch size, "half" / "halfh" / "halfw" an NHWC source at half the launch size on both axes / rows only /
columns only (nearest upsampling on the fly), "bcast" a per-sample constant [B][C], "planar" the f32 image of variant 6.
"""
import ctypes as C
import functools
import types
import zlib

import torch

import _wgrad_ref as R

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
H16 = (BF16, F16)
ALL = (F32, BF16, F16)
PLAN = "plan"   # split count: what fal_net_amd.ops._wgrad_plan returns for the case (the variant must be the case's)
NPATCH = "npatch"        # halo-patch kernels: one 4 x 32 patch per split ...
NPATCH_MORE = "npatch+"  # ... and more splits than patches (empty ranges write zero slabs)
TAP_MORE = "tap+"        # per-tap kernel: more splits than ceil(M / 256) 64-position steps can fill
GUARD_FLOATS = 1024      # 4 KiB behind the workspace
NAN = float("nan")
DTYPE_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}


def pad32(c):
    return (c + 31) // 32 * 32


def _c(name, kernel, variant, B, groups, cout, H, W, nsplits, stride=1, k=3, forms=None, up2=False, dtypes=H16, **extra):
    d = dict(name=name, kernel=kernel, variant=variant, B=B, groups=list(groups), cout=cout, H=H, W=W, nsplits=tuple(nsplits),
             stride=stride, k=k, forms=list(forms or ["nhwc"] * len(groups)), up2=up2, dtypes=tuple(dtypes))
    d.update(extra)
    return d


TAP_SPLITS = (1, 3, TAP_MORE)
PATCH_SPLITS = (1, 3, NPATCH, NPATCH_MORE)
ROWS_SPLITS = (1, 3, 8, 16, 40, PLAN)
UP2_SPLITS = (4, 8, 12, 40, PLAN)
WAVE_SPLITS = (1, 3, 8, 40, 256, PLAN)

CASES = [
    # ---- per-tap kernel (wgrad_kernel<T>): variant 0 where the launch is not dense 3x3 stride 1, variant 1 forced where it is
    _c("tap_1x1_6x40_c49", "wgrad_kernel", 0, 1, [49], 49, 6, 40, TAP_SPLITS, k=1, dtypes=ALL),
    _c("tap_3x1_12x40", "wgrad_kernel", 0, 2, [64], 64, 12, 40, TAP_SPLITS, k=(3, 1), dtypes=ALL),
    _c("tap_1x3_12x40", "wgrad_kernel", 0, 2, [64], 64, 12, 40, TAP_SPLITS, k=(1, 3), dtypes=ALL),
    _c("tap_s2_11x15", "wgrad_kernel", 0, 1, [32], 64, 11, 15, TAP_SPLITS, stride=2, dtypes=ALL),
    _c("tap_two_sources_8x16", "wgrad_kernel", 1, 2, [64, 32], 49, 8, 16, TAP_SPLITS, dtypes=ALL),
    _c("tap_const_source_s2_12x20", "wgrad_kernel", 0, 3, [32, 1], 64, 12, 20, TAP_SPLITS, stride=2, forms=["nhwc", "bcast"], dtypes=ALL),
    _c("tap_half_source_16x40", "wgrad_kernel", 1, 2, [64], 32, 16, 40, TAP_SPLITS, forms=["half"], dtypes=ALL),
    # ---- halo-patch kernels: 32 x 32 (variant 0, every dtype), 32 x 64 (variant 3), 64 x 32 (variant 4) channels per workgroup
    _c("patch11_9x33", "wgrad3x3_patch_kernel<T,1,1>", 0, 2, [64], 64, 9, 33, PATCH_SPLITS, dtypes=ALL),
    _c("patch11_12x40_c49", "wgrad3x3_patch_kernel<T,1,1>", 0, 1, [64, 32], 49, 12, 40, PATCH_SPLITS, dtypes=ALL),
    _c("patch11_10x16", "wgrad3x3_patch_kernel<T,1,1>", 0, 2, [64, 32], 64, 10, 16, PATCH_SPLITS, dtypes=ALL),
    _c("patch11_37x64", "wgrad3x3_patch_kernel<T,1,1>", 0, 1, [128], 32, 37, 64, PATCH_SPLITS, dtypes=ALL),
    _c("patch12_9x33", "wgrad3x3_patch_kernel<T,1,2>", 3, 2, [64], 64, 9, 33, PATCH_SPLITS),
    _c("patch12_12x40_c49", "wgrad3x3_patch_kernel<T,1,2>", 3, 1, [64, 32], 49, 12, 40, PATCH_SPLITS),  # last 64-channel cout block: 49 real
    _c("patch12_10x16", "wgrad3x3_patch_kernel<T,1,2>", 3, 2, [64, 32], 64, 10, 16, PATCH_SPLITS),
    _c("patch12_37x64", "wgrad3x3_patch_kernel<T,1,2>", 3, 1, [64], 64, 37, 64, PATCH_SPLITS),
    _c("patch21_9x33", "wgrad3x3_patch_kernel<T,2,1>", 4, 2, [64], 64, 9, 33, PATCH_SPLITS),
    _c("patch21_12x40_c49", "wgrad3x3_patch_kernel<T,2,1>", 4, 1, [64], 49, 12, 40, PATCH_SPLITS),
    _c("patch21_10x16", "wgrad3x3_patch_kernel<T,2,1>", 4, 2, [32, 32], 64, 10, 16, PATCH_SPLITS),  # one 64-channel block over both sources
    _c("patch21_37x64", "wgrad3x3_patch_kernel<T,2,1>", 4, 1, [128], 32, 37, 64, PATCH_SPLITS),
    # ---- stride-2 parity-plane kernel (variant 5): <T,2> when the padded cout is a multiple of 64, else <T,1>
    _c("s2_24x71_two_sources", "wgrad3x3_s2_kernel<T,2>", 5, 2, [32, 32], 64, 24, 71, (1, 2, 5), stride=2),
    _c("s2_9x66_c96", "wgrad3x3_s2_kernel<T,1>", 5, 8, [128], 96, 9, 66, (1, 2, 5), stride=2),
    _c("s2_37x65", "wgrad3x3_s2_kernel<T,2>", 5, 1, [64], 64, 37, 65, (1, 2, 5), stride=2),
    _c("s2_12x40_tw20", "wgrad3x3_s2_kernel<T,1>", 5, 2, [64], 32, 12, 40, (1, 2, 5), stride=2),  # TW in [16, 32): accepted, never planned
    # ---- first layer (variant 6): widths that are a multiple of 4 take the wave form, the others the patch form
    _c("c3_wave_16x64", "wgrad3x3_c3wave_kernel<T>", 6, 2, [3], 32, 16, 64, (1, 3, PLAN), forms=["planar"], c3form="wave"),
    _c("c3_wave_5x32", "wgrad3x3_c3wave_kernel<T>", 6, 1, [3], 32, 5, 32, (1, 3, PLAN), forms=["planar"], c3form="wave"),
    _c("c3_patch_37x70", "wgrad3x3_c3_kernel<T>", 6, 1, [3], 32, 37, 70, (1, 3, PLAN), forms=["planar"], c3form="patch"),
    _c("c3_patch_75x250", "wgrad3x3_c3_kernel<T>", 6, 1, [3], 32, 75, 250, (1, 3, PLAN), forms=["planar"], c3form="patch"),
    _c("c3_misaligned_16x64", "wgrad3x3_c3_kernel<T>", 6, 2, [3], 32, 16, 64, (1, 3, 20, PLAN), forms=["planar"], c3form="patch", misalign=True,
       same_operands_as="c3_wave_16x64"),
    _c("c3_wave_odd_grid_5x32", "wgrad3x3_c3wave_kernel<T>", 6, 2, [3], 32, 5, 32, (1, 3), forms=["planar"], c3form="wave", image="odd_grid"),
    _c("c3_patch_odd_grid_6x35", "wgrad3x3_c3_kernel<T>", 6, 1, [3], 32, 6, 35, (1, 3), forms=["planar"], c3form="patch", image="odd_grid"),
    # ---- row-streaming kernel (variant 7): the seven ROWS_CASES shapes of test_gpu_ops.py
    _c("rows_9x33", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 2, [64], 64, 9, 33, ROWS_SPLITS),
    _c("rows_two_sources_16x32", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 1, [128, 256], 256, 16, 32, ROWS_SPLITS),
    _c("rows_straddle_12x40_c49", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 2, [32, 32], 49, 12, 40, ROWS_SPLITS),
    _c("rows_cin96_10x70_c49", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 1, [64, 32], 49, 10, 70, ROWS_SPLITS),
    _c("rows_half_source_16x40", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 2, [64], 32, 16, 40, ROWS_SPLITS, forms=["half"]),
    _c("rows_37x64", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 1, [64], 128, 37, 64, ROWS_SPLITS),
    _c("rows_many_units_24x64", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 8, [64], 64, 24, 64, ROWS_SPLITS),
    # accepted by falnet_wgrad_rows_applicable, never planned: TW < 32, a 32-channel source, a source half-sized on one axis only
    _c("rows_12x20_tw20", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 2, [64], 64, 12, 20, (1, 3, 8)),
    _c("rows_cin32_9x33", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 1, [32], 64, 9, 33, (1, 3, 8)),
    _c("rows_half_rows_only_16x40", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 2, [64], 64, 16, 40, (1, 3, 8), forms=["halfh"]),
    _c("rows_half_columns_only_9x40", "wgrad3x3_rows16_kernel<T,4,2,false>", 7, 2, [64], 64, 9, 40, (1, 3, 8), forms=["halfw"]),
    # up2: gout at 2 TH x 2 TW, the source at TH x TW
    _c("rows_up2_9x33", "wgrad3x3_rows16_kernel<T,4,2,true>", 7, 2, [64], 64, 9, 33, UP2_SPLITS, up2=True),
    _c("rows_up2_10x70_cin96_c49", "wgrad3x3_rows16_kernel<T,4,2,true>", 7, 1, [96], 49, 10, 70, UP2_SPLITS, up2=True),
    _c("rows_up2_8x24x64", "wgrad3x3_rows16_kernel<T,4,2,true>", 7, 8, [64], 64, 24, 64, UP2_SPLITS, up2=True),
    # ---- row-streaming kernel, stride 2 (variant 8)
    _c("rows_s2_16x64", "wgrad3x3_rows8s2_kernel<T,2>", 8, 2, [64], 128, 16, 64, (1, 2, 5, 16, PLAN), stride=2),
    _c("rows_s2_9x66_c96", "wgrad3x3_rows8s2_kernel<T,2>", 8, 1, [128], 96, 9, 66, (1, 2, 5, 16, PLAN), stride=2),
    _c("rows_s2_31x70", "wgrad3x3_rows8s2_kernel<T,2>", 8, 3, [256], 256, 31, 70, (1, 2, 5, 16, PLAN), stride=2),
    _c("rows_s2_11x30_tw15", "wgrad3x3_rows8s2_kernel<T,2>", 8, 2, [64], 64, 11, 30, (1, 2, 5), stride=2),   # TW < 32: accepted, never planned
    _c("rows_s2_cin32_16x64", "wgrad3x3_rows8s2_kernel<T,2>", 8, 2, [32], 64, 16, 64, (1, 2, 5), stride=2),  # 32-channel source: the same
    # ---- wave-streaming kernel (variant 9): the five WAVE_CASES (gC 32 and gC 64) and the four stride-2 shapes of test_gpu_ops.py
    _c("wave_9x33", "wgrad3x3_wave32_kernel<T,1,false>", 9, 2, [32], 32, 9, 33, WAVE_SPLITS),
    _c("wave_12x40_c49", "wgrad3x3_wave32_kernel<T,2,false>", 9, 1, [32], 49, 12, 40, WAVE_SPLITS),
    _c("wave_37x64", "wgrad3x3_wave32_kernel<T,1,false>", 9, 2, [32], 32, 37, 64, WAVE_SPLITS),
    _c("wave_many_units_24x96", "wgrad3x3_wave32_kernel<T,1,false>", 9, 8, [32], 32, 24, 96, WAVE_SPLITS),
    _c("wave_5x32_c64", "wgrad3x3_wave32_kernel<T,2,false>", 9, 1, [32], 64, 5, 32, WAVE_SPLITS),
    _c("wave_s2_24x80", "wgrad3x3_wave32_kernel<T,2,true>", 9, 2, [32], 64, 24, 80, WAVE_SPLITS, stride=2),
    _c("wave_s2_37x65", "wgrad3x3_wave32_kernel<T,2,true>", 9, 1, [32], 64, 37, 65, WAVE_SPLITS, stride=2),
    _c("wave_s2_many_units_32x128_c49", "wgrad3x3_wave32_kernel<T,2,true>", 9, 8, [32], 49, 32, 128, WAVE_SPLITS, stride=2),
    _c("wave_s2_6x64", "wgrad3x3_wave32_kernel<T,2,true>", 9, 1, [32], 64, 6, 64, WAVE_SPLITS, stride=2),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
KERNELS = sorted({c["kernel"] for c in CASES})
# `kernel` field -> (id falnet_wgrad_kernel_name returns: fal_net_amd._lib.WGK_*, the symbol with {T} = the mangled operand type, whether
# the kernel sums the bias gradient): what a case must reach, spelled out (tests/test_wgrad_plan_host.py)
KERNEL_TABLE = {
    "wgrad_kernel": (0, "_Z12wgrad_kernelI{T}Ev14falnet_wgrad_ti", False),
    "wgrad3x3_patch_kernel<T,1,1>": (1, "_Z21wgrad3x3_patch_kernelI{T}Li1ELi1EEv14falnet_wgrad_tiiii", True),
    "wgrad3x3_patch_kernel<T,1,2>": (1, "_Z21wgrad3x3_patch_kernelI{T}Li1ELi2EEv14falnet_wgrad_tiiii", True),
    "wgrad3x3_patch_kernel<T,2,1>": (1, "_Z21wgrad3x3_patch_kernelI{T}Li2ELi1EEv14falnet_wgrad_tiiii", True),
    "wgrad3x3_s2_kernel<T,1>": (2, "_Z18wgrad3x3_s2_kernelI{T}Li1EEv14falnet_wgrad_tiiii", True),
    "wgrad3x3_s2_kernel<T,2>": (2, "_Z18wgrad3x3_s2_kernelI{T}Li2EEv14falnet_wgrad_tiiii", True),
    "wgrad3x3_c3_kernel<T>": (3, "_Z18wgrad3x3_c3_kernelI{T}Ev14falnet_wgrad_tiiii", True),
    "wgrad3x3_c3wave_kernel<T>": (4, "_Z22wgrad3x3_c3wave_kernelI{T}Ev14falnet_wgrad_ti", True),
    "wgrad3x3_rows16_kernel<T,4,2,false>": (5, "_Z22wgrad3x3_rows16_kernelI{T}Li4ELi2ELb0EEv14falnet_wgrad_tiiii", True),
    "wgrad3x3_rows16_kernel<T,4,2,true>": (5, "_Z22wgrad3x3_rows16_kernelI{T}Li4ELi2ELb1EEv14falnet_wgrad_tiiii", True),
    "wgrad3x3_rows8s2_kernel<T,2>": (6, "_Z23wgrad3x3_rows8s2_kernelI{T}Li2EEv14falnet_wgrad_tiiii", True),
    "wgrad3x3_wave32_kernel<T,1,false>": (7, "_Z22wgrad3x3_wave32_kernelI{T}Li1ELb0EEv14falnet_wgrad_ti", True),
    "wgrad3x3_wave32_kernel<T,2,false>": (7, "_Z22wgrad3x3_wave32_kernelI{T}Li2ELb0EEv14falnet_wgrad_ti", True),
    "wgrad3x3_wave32_kernel<T,2,true>": (7, "_Z22wgrad3x3_wave32_kernelI{T}Li2ELb1EEv14falnet_wgrad_ti", True),
}
# one case per kernel for the deterministic-mode child (tests/_wgrad_det.py) and the mutation tests
DET_CASES = ["tap_two_sources_8x16", "patch11_12x40_c49", "patch12_9x33", "patch21_37x64", "s2_24x71_two_sources", "s2_9x66_c96",
             "c3_wave_16x64", "c3_patch_37x70", "rows_straddle_12x40_c49", "rows_up2_9x33", "rows_s2_9x66_c96", "wave_12x40_c49", "wave_9x33",
             "wave_s2_37x65"]
MUTATION_CASES = {"rows": "rows_9x33", "wave": "wave_9x33"}


# --------------------------------------------------------------------------------------------------------------- geometry
def taps_of(k):
    if k == 1:
        return [(0, 0)]
    KH, KW = (3, 3) if k == 3 else k
    return [(kh - KH // 2, kw - KW // 2) for kh in range(KH) for kw in range(KW)]


def geom(case):
    """Every derived size of a case: the dict tests/_wgrad_ref.py takes (`desc`), the operand shapes, the slab shape."""
    B, s, H, W = case["B"], case["stride"], case["H"], case["W"]
    planar = case["forms"] == ["planar"]
    groups = case["groups"]
    gpad = [32] if planar else [pad32(c) for c in groups]
    cin_total, cin, cout = sum(gpad), sum(groups), case["cout"]
    TH, TW = (H + s - 1) // s, (W + s - 1) // s
    two = len(groups) == 2
    shapes = []
    for f, cp in zip(case["forms"], gpad):
        shapes.append({"nhwc": (B, H, W, cp), "half": (B, H // 2, W // 2, cp), "halfh": (B, H // 2, W, cp), "halfw": (B, H, W // 2, cp),
                       "bcast": (B, cp), "planar": (B, 3, H, W)}[f])
    up = 2 if case["up2"] else 1
    desc = dict(B=B, TH=TH, TW=TW, IH=H, IW=W, stride=s, taps=taps_of(case["k"]), gC=pad32(cout), cout=cout, cin_total=cin_total,
                srcs=[{"C": cp, "form": f if f in ("bcast", "planar") else "nhwc"} for f, cp in zip(case["forms"], gpad)],
                up2=int(case["up2"]), cin=cin, c0_real=groups[0] if two else cin, c0_pad=gpad[0] if two else cin_total)
    return dict(desc=desc, src_shapes=shapes, gout_shape=(B, up * TH, up * TW, pad32(cout)), groups_pad=gpad,
                n=R.positions(desc), npatch=B * ((TH + 3) // 4) * ((TW + 31) // 32), M=B * TH * TW)


def g_range(case):
    return case.get("g_range", R.G_RANGE)


def exactness(case):
    """The exactness condition of _wgrad_ref.assert_exact for this case (raises when it does not hold)."""
    g = geom(case)
    lo, hi = g_range(case)
    if case.get("image") == "odd_grid":  # image values (2 k + 1) 2^-10 in (0, 2): rounded or not, every value is a multiple of 2^-10
        return R.assert_exact(g["n"], 2.0, max(abs(lo), abs(hi)), unit=2.0 ** -10)
    return R.assert_exact(g["n"], R.X_RANGE[1], max(abs(lo), abs(hi)))


def split_counts(case):
    """The case's split counts with the symbolic ones resolved (PLAN stays: it needs the library)."""
    g = geom(case)
    out = []
    for s in case["nsplits"]:
        if s == NPATCH:
            s = g["npatch"]
        elif s == NPATCH_MORE:
            s = g["npatch"] + 3
        elif s == TAP_MORE:
            s = (g["M"] + 255) // 256 + 4
        out.append(s)
    return out


def _seed(case):
    return zlib.crc32(case.get("same_operands_as", case["name"]).encode())


@functools.lru_cache(maxsize=None)
def _host_operands(name):
    """(sources, gout) of a case as f32 CPU tensors holding the integers (padding channels of the sources zero, as the NHWC contract
    says; every channel of gout filled: a kernel must not let the padding of gout reach the real outputs or the bias gradient)."""
    case = BY_NAME[name]
    g = geom(case)
    seed = _seed(case)
    srcs = []
    for i, (shape, f, c) in enumerate(zip(g["src_shapes"], case["forms"], case["groups"])):
        if f == "planar" and case.get("image") == "odd_grid":
            t = (2 * R.int_operand(shape, 0, 1023, seed + i) + 1) * 2.0 ** -10
        else:
            t = R.int_operand(shape, *R.X_RANGE, seed + i)
            if f != "planar":
                t[..., c:] = 0
        srcs.append(t)
    gout = R.int_operand(g["gout_shape"], *g_range(case), seed + 17)
    return srcs, gout


def host_operands(case):
    return _host_operands(case["name"])


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, device):
    case = BY_NAME[name]
    srcs, gout = host_operands(case)
    desc = geom(case)["desc"]
    srcs = [(t.to(dtype) if f == "planar" else t).to(device) for t, f in zip(srcs, case["forms"])]  # the image as the kernel converts it
    slab, oihw = R.wgrad_ref(desc, srcs, gout.to(device))
    return dict(slab=slab, oihw=oihw, bias=R.bias_ref(gout.to(device), desc["cout"]), max_abs=float(oihw.abs().max()))


def reference(case, dtype=F32, device="cpu"):
    """Float64 reference of a case (shared by every dtype: the integers are the same; an odd-grid image is rounded to `dtype`)."""
    return _reference(case["name"], dtype if case.get("image") == "odd_grid" else F32, str(device))


# --------------------------------------------------------------------------------------------------------------- the launch
def _first_bad(got, ref):
    bad = (got != ref) | torch.isnan(got)
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return f"{int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: got {float(got[idx])}, reference {float(ref[idx])}"


def sources(case, dtype, device):
    """Device tensors of the sources in `dtype` (the planar image stays f32; misalign: its pointer moved by one float)."""
    out = []
    for t, f in zip(host_operands(case)[0], case["forms"]):
        if f == "planar":
            if case.get("misalign"):
                buf = torch.empty(t.numel() + 1, dtype=F32, device=device)
                v = buf[1:].view(t.shape)
                v.copy_(t)
                assert v.data_ptr() % 16 == 4
                out.append(v)
            else:
                out.append(t.to(device).contiguous())
        else:
            out.append(t.to(dtype).to(device).contiguous())
    return out


def fill_desc(case, dtype, srcs_t, gout_t, nsplit, variant=None):
    """falnet_wgrad_t of a case over the given device tensors (no workspace, no bias pointer yet)."""
    from fal_net_amd import _lib as L
    from fal_net_amd import ops
    g = geom(case)
    desc = g["desc"]
    srcs = []
    for t, f in zip(srcs_t, case["forms"]):
        srcs.append(ops.planar_src(t) if f == "planar" else ops.bcast_src(t, desc["IH"], desc["IW"]) if f == "bcast" else ops.nhwc_src(t))
    d = L.Wgrad()
    pc = types.SimpleNamespace(cout=desc["cout"], cin_pad=desc["cin_total"])
    ops._fill_wgrad(d, dtype, srcs, desc["IH"], desc["IW"], gout_t, [(dy, dx, 0) for dy, dx in desc["taps"]], desc["stride"], desc["B"],
                    desc["TH"], desc["TW"], pc)
    d.variant, d.nsplit, d.up2 = case["variant"] if variant is None else variant, nsplit, desc["up2"]
    return d, srcs


def planned(case, dtype, device="cuda"):
    """(variant, nsplit) fal_net_amd.ops._wgrad_plan returns for the case's launch."""
    from fal_net_amd import ops
    g = geom(case)
    desc = g["desc"]
    srcs_t = sources(case, dtype, device)
    _, srcs = fill_desc(case, dtype, srcs_t, host_operands(case)[1].to(dtype).to(device), 1)
    slab = len(desc["taps"]) * desc["gC"] * desc["cin_total"] * 4
    variant, nsplit, _ = ops._wgrad_plan(dtype, srcs, desc["taps"], desc["stride"], desc["B"], desc["TH"], desc["TW"], desc["IH"], desc["IW"],
                                         desc["cin_total"], desc["gC"], max(1, ops.WgradBatch.SLAB_CAP // slab), up2=bool(desc["up2"]))
    return variant, nsplit


def run_case(case, dtype, nsplit, device="cuda", variant=None, zero_pixel=None, reduce_nsplit=None, strict=True):
    """One launch of the case with `nsplit` slabs, steps 1-7 of tests/test_gpu_wgrad.py.  Returns a dict of findings: `guard`, `slab`,
    `reduce`, `accumulate`, `bias` (True = as the reference says; `bias` None when the kernel does not fuse it), `fuses_bias`, `ws`
    (the raw slabs) and `desc`.  strict: assert every finding, naming the first element that differs.
    zero_pixel (b, y, x): the KERNEL's gout has that pixel zeroed while the reference keeps it -- a mutation that must be seen.
    reduce_nsplit: the slab count falnet_wgrad_reduce is told (default: nsplit)."""
    from fal_net_amd import _lib as L
    lib = L.lib()
    g = geom(case)
    desc = g["desc"]
    ref = reference(case, dtype, device)
    ntaps, gC, cin_total, cout, cin = len(desc["taps"]), desc["gC"], desc["cin_total"], desc["cout"], desc["cin"]
    srcs_t = sources(case, dtype, device)
    gout_t = host_operands(case)[1].to(dtype).to(device).contiguous()
    if zero_pixel is not None:
        b, y, x = zero_pixel
        assert bool((gout_t[b, y, x, :cout] != 0).any()), "the pixel to drop must carry a gradient"
        gout_t[b, y, x] = 0
    d, srcs = fill_desc(case, dtype, srcs_t, gout_t, nsplit, variant)
    what = f"{case['name']} {DTYPE_NAME[dtype]} nsplit={nsplit} variant={d.variant}"
    # 1. NaN over the workspace and a 4 KiB guard behind it
    nfl = nsplit * ntaps * gC * cin_total
    assert int(lib.falnet_wgrad_workspace_bytes(C.byref(d))) == 4 * nfl, what
    ws = torch.full((nfl + GUARD_FLOATS,), NAN, dtype=F32, device=device)
    d.partial = ws.data_ptr()
    fuses = int(lib.falnet_wgrad_fuses_bias(C.byref(d)))
    db = None
    if fuses:
        db = torch.zeros(gC + 32, dtype=F32, device=device)
        db[cout:] = 7.0
        d.bias_grad = db.data_ptr()
    # 2. the launch
    L.check(lib.falnet_wgrad(C.byref(d), L.stream_ptr()), what)
    out = dict(fuses_bias=fuses, desc=d, ws=ws, what=what)
    # 3. the guard
    out["guard"] = bool(torch.isnan(ws[nfl:]).all())
    # 4. float64 sum of the slabs at every (tap, co < cout, real input channel)
    cols = torch.tensor(R.unpack_columns(desc), device=device)
    got = R.slab_sum(ws, nsplit, ntaps, gC, cin_total)[:, :cout][:, :, cols]
    want = ref["slab"][:, :cout][:, :, cols]
    msg = {"slab": _first_bad(got, want)}
    # 5. / 6. the reduce: overwrite a NaN-filled gradient, then add onto 7
    rn = nsplit if reduce_nsplit is None else reduce_nsplit
    for key, fill, acc in (("reduce", NAN, 0), ("accumulate", 7.0, 1)):
        gw = torch.full((cout, cin, ntaps), fill, dtype=F32, device=device)
        L.check(lib.falnet_wgrad_reduce(L.ptr(ws), rn, ntaps, gC, cin_total, L.ptr(gw), cout, cin, desc["c0_real"], desc["c0_pad"], acc,
                                        L.stream_ptr()), what + " reduce")
        msg[key] = _first_bad(gw.to(torch.float64), ref["oihw"] + (7.0 if acc else 0.0))
    # 7. the fused bias gradient, added into zeros; elements >= cout untouched
    msg["bias"] = None
    if fuses:
        msg["bias"] = _first_bad(db[:cout].to(torch.float64), ref["bias"])
        if msg["bias"] is None and not bool((db[cout:] == 7.0).all()):
            msg["bias"] = f"bias gradient elements >= cout were written: {db[cout:].tolist()}"
    for k, m in msg.items():
        out[k] = (m is None) if (k != "bias" or fuses) else None
    out["messages"] = msg
    if strict:
        assert out["guard"], what + ": the guard behind the workspace was written"
        for k, m in msg.items():
            assert m is None, f"{what}: {k}: {m}"
    return out


def range_start_pixel(case, nranges, k=1):
    """(b, y, x) of the first gout pixel of pixel range k when the row / wave-streaming kernels cut the (sample, 32-pixel strip, row)
    units into `nranges` ranges (rows: nsplit; wave, stride 1: nsplit * 8 / (gC / 32); wave, stride 2: nsplit)."""
    desc = geom(case)["desc"]
    nstrips = (desc["TW"] + 31) // 32
    u = desc["B"] * nstrips * desc["TH"] * k // nranges
    bs, y = divmod(u, desc["TH"])
    return bs // nstrips, y, (bs % nstrips) * 32


def c3_form(case, out, nsplit):
    """Which form of variant 6 ran, from the slabs: the patch form gives split s the patches [s pps, (s + 1) pps), so with more splits
    than patches the slabs from npatch on are exact zeros; the wave form cuts (sample, strip, row) units and fills them.  With at most
    as many splits as patches (the patch form's planned count) the centre tap tells: in the patch form, and only there, every slab holds
    the products of exactly its patches' pixels (4 x 32 patches numbered sample, patch row, patch column; needs two slabs at least)."""
    g = geom(case)
    n = 9 * 32 * 32
    if nsplit > g["npatch"]:
        tail = out["ws"][g["npatch"] * n:nsplit * n].view(-1, 9, 32, 32)[..., :3]
        return "patch" if bool((tail == 0).all()) else "wave"
    assert nsplit >= 2 and case.get("image") != "odd_grid", "one slab holds the same sums in both forms"
    desc = g["desc"]
    B, TH, TW = desc["B"], desc["TH"], desc["TW"]
    (img,), gout = host_operands(case)
    ty, tx = (TH + 3) // 4, (TW + 31) // 32
    pps = (g["npatch"] + nsplit - 1) // nsplit
    owner = torch.arange(B).view(B, 1, 1) * ty * tx + (torch.arange(TH) // 4).view(1, TH, 1) * tx + (torch.arange(TW) // 32).view(1, 1, TW)
    centre = out["ws"][:nsplit * n].view(nsplit, 9, 32, 32)[:, 4, :, :3].to(torch.float64).cpu()
    for s in range(nsplit):
        mine = ((owner // pps) == s).to(torch.float64)
        want = torch.einsum("byxo,bcyx->oc", gout[..., :32].to(torch.float64) * mine.unsqueeze(-1), img.to(torch.float64))
        if not torch.equal(centre[s], want):
            return "wave"
    return "patch"
