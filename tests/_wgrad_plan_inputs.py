"""Inputs of tests/test_wgrad_plan_host.py: weight-gradient launches as plain lists (`spec`), the descriptor a spec stands for, and the switch
settings every input is planned under.  No GPU: pointers are 16-byte aligned stand-ins, falnet_wgrad_kernel_name dereferences none.

spec = [dtype, srcs, k, stride, B, TH, TW, IH, IW, cout, max_slabs, up2]
  dtype      "f32" | "bf16" | "f16"
  srcs       [[C, form], ...]: C padded channels; form "nhwc" (at IH x IW), "half" / "halfh" / "halfw" (half size on both axes / rows / columns),
             "bcast" (per-sample constant) or "planar" (the f32 image of variant 6, C = 3)
  k          1, 3 or [kh, kw]: the 'same'-padded taps of fal_net_amd.ops.fwd_taps
  max_slabs  the slab budget _wgrad_plan_desc gets
"""
import contextlib
import itertools
import os
import types

import torch

FAKE = 1 << 20
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPE_NAME = {v: k for k, v in DTYPES.items()}

# the sweep of the fixture, expanded in this order by sweep_specs()
CHANNELS = (32, 64, 96, 128, 256, 512)
SOURCE_FORMS = (("nhwc",), ("half",), ("bcast",), ("nhwc", "nhwc"), ("nhwc", "half"), ("nhwc", "bcast"))
SHAPES = ((4, 16), (5, 32), (9, 33), (16, 40), (37, 64), (128, 256))
SLAB_CAP = 32 << 20  # fal_net_amd.ops.WgradBatch.SLAB_CAP at its default

# (label, environment read through fal_net_amd._lib.ab, attributes of fal_net_amd.ops, deterministic mode): every setting _wgrad_plan_desc reads, flipped
SWITCHES = [("default", {}, {}, False)]
SWITCHES += [(f"{n}=0", {n: "0"}, {}, False) for n in ("FALNET_WGRAD_S2", "FALNET_WGRAD_WAVE", "FALNET_WGRAD_WAVE_S2", "FALNET_WGRAD_ROWS_S2",
                                                       "FALNET_WGRAD_ROWS", "FALNET_WGRAD_CO2")]
SWITCHES += [("FALNET_WGRAD_ROWS_S2_MINCIN=128", {"FALNET_WGRAD_ROWS_S2_MINCIN": "128"}, {}, False),
             ("FALNET_WGRAD_ROWS_SKIP_CIN=64,256", {"FALNET_WGRAD_ROWS_SKIP_CIN": "64,256"}, {}, False),
             ("FALNET_WGRAD_CO2_MAXCIN=64", {"FALNET_WGRAD_CO2_MAXCIN": "64"}, {}, False)]
# (read once at import: flipped on the module, as tools/bench_wgrad32.py does)
SWITCHES += [(f"{a}={v}", {}, {a: v}, False) for a, v in (("_WGRAD_WGS", 512), ("_WGRAD_ROWS_WGS", 256), ("_WGRAD_ROWS_MIN_ROWS", 4),
                                                          ("_WGRAD_WAVE_WGS", 128), ("_WGRAD_WAVE_MIN_ROWS", 4))]
SWITCHES += [("deterministic", {}, {}, True)]


def pad32(c):
    return (c + 31) // 32 * 32


def sweep_specs():
    """Canonical 3x3 taps, aligned pointers, bf16: every combination of the axes above that names a launch (two sources need two 32-channel
    groups; a stride-2 launch of TH x TW reads a 2 TH x 2 TW input; up2 forms for a deconv layer's launch only)."""
    for cin, cout, forms, stride, up2, (TH, TW), B, cap in itertools.product(CHANNELS, CHANNELS, SOURCE_FORMS, (1, 2), (0, 1, 2), SHAPES, (1, 8), (0, 1)):
        if len(forms) == 2 and cin < 64:
            continue
        if up2 and (stride == 2 or forms not in (("nhwc",), ("bcast",))):  # (a deconv layer: stride 1, ONE source at the launch size; the parent planned
            continue                                                      # kernels for the other forms that the library then refused to launch)
        c0 = cin if len(forms) == 1 else cin // 64 * 32
        srcs = [[c0, forms[0]]] + ([[cin - c0, forms[1]]] if len(forms) == 2 else [])
        slab = 9 * cout * cin * 4
        yield ["bf16", srcs, 3, stride, B, TH, TW, stride * TH, stride * TW, cout, SLAB_CAP // slab if cap else 4, up2]


def case_specs():
    """(label, spec) of every case of tests/_wgrad_cases.py and tests/_wgrad_up2q_cases.py (the latter in its three forms) in each of its dtypes,
    with the slab budget WgradBatch.add gives the launch."""
    import _wgrad_cases as K
    import _wgrad_up2q_cases as Q
    for c in K.CASES:
        g = K.geom(c)
        d = g["desc"]
        srcs = [[3 if f == "planar" else cp, f] for f, cp in zip(c["forms"], g["groups_pad"])]
        slab = len(d["taps"]) * d["gC"] * d["cin_total"] * 4
        k = c["k"] if isinstance(c["k"], int) else list(c["k"])
        for dt in c["dtypes"]:
            yield f"{c['name']}-{DTYPE_NAME[dt]}", [DTYPE_NAME[dt], srcs, k, c["stride"], c["B"], d["TH"], d["TW"], d["IH"], d["IW"], c["cout"],
                                                    max(1, SLAB_CAP // slab), int(c["up2"])]
    for c in Q.CASES:
        cin_pad, gC = pad32(c["cin"]), pad32(c["cout"])
        for up2, dt in itertools.product((2, 1, 0), ("bf16", "f16")):
            h, w = (c["H"], c["W"]) if up2 else (2 * c["H"], 2 * c["W"])
            yield f"up2q_{c['name']}-up2={up2}-{dt}", [dt, [[cin_pad, "nhwc"]], 3, 1, c["B"], h, w, h, w, c["cout"], max(1, SLAB_CAP // (9 * gC * cin_pad * 4)), up2]


def sources(L, spec, ptr=FAKE):
    """The falnet_src_t list of a spec over stand-in pointers (`ptr`: the first source's)."""
    _, srcs, _, _, B, _, _, IH, IW = spec[:9]
    out = []
    for i, (Cc, form) in enumerate(srcs):
        s = L.Src()
        s.ptr, s.C = (ptr if i == 0 else FAKE), Cc
        if form == "planar":
            s.H, s.W, s.sb, s.sy, s.sx = IH, IW, 3 * IH * IW, IW, 1
        elif form == "bcast":
            s.H, s.W, s.sb, s.sy, s.sx = IH, IW, Cc, 0, 0
        else:
            s.H = IH // 2 if form in ("half", "halfh") else IH
            s.W = IW // 2 if form in ("half", "halfw") else IW
            s.sb, s.sy, s.sx = s.H * s.W * Cc, s.W * Cc, Cc
        out.append(s)
    return out


def taps_of(spec, ops):
    k = spec[2]
    return [(dy, dx, 0) for dy, dx, _ in ops.fwd_taps(k if isinstance(k, int) else tuple(k))]


def descriptor(L, ops, spec, ptr=FAKE, taps=None):
    """The filled falnet_wgrad_t of a spec (fal_net_amd.ops._fill_wgrad over stand-in operands) -- what WgradBatch.add hands _wgrad_plan_desc."""
    dtype, srcs, _, stride, B, TH, TW, IH, IW, cout = spec[:10]
    cin_pad = sum(32 if f == "planar" else Cc for Cc, f in srcs)
    gout = types.SimpleNamespace(shape=(B, TH, TW, pad32(cout)), data_ptr=lambda: FAKE)
    d = L.Wgrad()
    ops._fill_wgrad(d, DTYPES[dtype], sources(L, spec, ptr), IH, IW, gout, taps_of(spec, ops) if taps is None else taps, stride, B, TH, TW,
                    types.SimpleNamespace(cout=cout, cin_pad=cin_pad))
    return d


def plan(L, ops, spec, **kw):
    """[variant, nsplit, symbol] fal_net_amd.ops._wgrad_plan_desc gives the spec, or ["ValueError"] where it refuses an up2 launch."""
    try:
        return list(ops._wgrad_plan_desc(descriptor(L, ops, spec, **kw), spec[10], up2=spec[11]))
    except ValueError:
        return ["ValueError"]


@contextlib.contextmanager
def switched(L, ops, env, attrs, deterministic):
    """One SWITCHES setting: the environment under FALNET_AB=1, module attributes of ops, the library's deterministic flag; all put back."""
    old_env = {n: os.environ.get(n) for n in list(env) + ["FALNET_AB"]}
    old_attrs = {a: getattr(ops, a) for a in attrs}
    old_det = L.lib().falnet_get_deterministic()
    try:
        if env:
            os.environ.update(env, FALNET_AB="1")
        for a, v in attrs.items():
            setattr(ops, a, v)
        L.lib().falnet_set_deterministic(1 if deterministic else old_det)
        yield
    finally:
        L.lib().falnet_set_deterministic(old_det)
        for a, v in old_attrs.items():
            setattr(ops, a, v)
        for n, v in old_env.items():
            os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)
