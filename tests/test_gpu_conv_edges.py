"""GPU: every falnet_conv2d kernel variant, per element against float64, at ragged shapes (tests/_conv_edge_cases.py).

tests/test_gpu_cache_choices.py holds the 675 launches the autotune cache pins (B = 8 / 16, even maps, one variant per signature) to
|got - ref| <= u |ref| + MAG_COEF mag; everything else -- odd and ragged maps, other batch sizes, every variant the autotuner or the heuristic
may pick at a shape outside the cache -- was held only by a max-norm bound that a wrong rounding mode, a wrong ELU branch or a wrong corner
element passes (tests/test_conv_edges_host.py shows it).  Here every (case, dtype) of the table is built through ops.conv_call /
ops.conv_multi_call / ops.deconv_dgrad_call with autotuning off, the float64 reference (tests/_conv_ref.py:conv_ref, BLAS GEMMs on the device)
is computed once from the signature of the descriptor actually launched, and EVERY variant the host test pins as applicable is launched once:
  * return code 0 (a refusal is a failure: EXPECT says the variant applies);
  * every mapped element within u |ref| + MAG_COEF mag -- the same u and the same coefficient as test_gpu_cache_choices.py --, every
    unmapped one still the NaN sentinel, padded output channels exactly 0, the max-norm error within test_gpu_ops.TOL;
  * the split-K workspace and variant 19's tile counters all zero afterwards; a second launch of variants 19 and 14 gives the same bits.
The bound can fail: per kernel family, one element of the KERNEL's copy of the packed weight is zeroed (the reference keeps it) -- violations
must appear, and only in that output channel.
FALNET_CONV_EDGES_REPORT=<path> appends one JSON line per launch (case, dtype, variant, ksplit, kernel, worst_ratio, maxnorm_rel)."""
import ctypes as C
import json
import os

import pytest
import torch

from fal_net_amd import _lib as L
from fal_net_amd import ops

import _conv_edge_cases as E
import _conv_ref as R
from test_gpu_cache_choices import MAG_COEF
from test_gpu_ops import TOL

pytestmark = pytest.mark.gpu

OWNER = ("test-conv-edges",)
REPORT = os.environ.get("FALNET_CONV_EDGES_REPORT")
NAN = float("nan")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _name(dt):
    return str(dt).replace("torch.", "")


def _report(case, dt, variant, ksplit, kernel, parts):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps({"case": case, "dtype": _name(dt), "variant": variant, "ksplit": ksplit, "kernel": kernel,
                                "worst_ratio": max(p["worst_ratio"] for p in parts.values()),
                                "maxnorm_rel": max(p["maxnorm_rel"] for p in parts.values())}) + "\n")


def _kernel_name(desc):
    buf = C.create_string_buffer(160)
    rc = L.lib().falnet_conv2d_kernel_name(C.byref(desc), buf, 160)
    assert rc == 0, (desc.variant, desc.ksplit, rc, L.lib().falnet_last_error())
    return buf.value.decode()


def _launch(call):
    rc = L.lib().falnet_conv2d(call.ref, L.stream_ptr())
    assert rc == 0, (call.desc.variant, call.desc.ksplit, rc, L.lib().falnet_last_error())
    torch.cuda.synchronize()


def _packed_deconv(case, o, dt, dev):
    """The library's own packing of a `deconv` layer's master weight (1/64 grid): wf / wd / wu / wdd."""
    cin = case["srcs"][0][0] if case["op"] == "fwd" else case["cin"]
    pc = ops.PackedConv("edge-" + case["name"], torch.nn.Parameter(o["w"].to(dev)), None, [cin], 1)
    pc.up2 = True
    pc.alloc(dt, dev)
    pc.pack_call()()
    ops.pack_up2_call([pc], dt, dev)()
    torch.cuda.synchronize()
    assert pc.wu is not None and pc.wdd is not None
    return pc


def _zero_one_weight(w, row):
    """Copy of a packed weight [rows][taps][K] with the largest element of `row` zeroed."""
    wk = w.clone()
    flat = wk[row].reshape(-1)
    i = int(flat.float().abs().argmax())
    assert float(flat[i]) != 0.0
    flat[i] = 0
    return wk


class Built:
    """One launch of the table on the device: operands, the call (variant 0, autotune off) and the float64 reference."""

    def __init__(self, case, dt, label="", fault_row=None, shared=None):
        dev = _dev()
        self.case, self.dt, self.label = case, dt, label
        sig = dict(E.sigs(case, dt))[label]
        o = shared if shared is not None else {k: (v.to(dev) if torch.is_tensor(v) else [t.to(dev) for t in v] if isinstance(v, list) else v)
                                               for k, v in E.operands(case, dt).items()}
        self.o = o
        B, OH, OW, Cout, cst = sig["B"], sig["OH"], sig["OW"], sig["Cout"], sig["out_cstride"]
        planar = sig["out_layout"] == R.OUT_PLANAR_F32
        self.out_dt = torch.float32 if planar else dt
        oshape = (B, Cout, OH, OW) if planar else (B, OH, OW, cst)
        if shared is not None and "out" in shared:
            self.out = shared["out"]  # the parity classes of one data gradient write one tensor
        else:
            self.out = torch.full(oshape, NAN, dtype=self.out_dt, device=dev) if sig["out"] else None
        self.pool_out = torch.full((B, OH // 2, OW // 2, cst), NAN, dtype=dt, device=dev) if sig["pool"] else None
        self.alias = case.get("addend") == "alias"
        addend = self.out if self.alias else o["addend"]
        srcs = [ops.bcast_src(t, s["H"], s["W"]) if s["bcast"] else ops.nhwc_src(t) for t, s in zip(o["srcs"], sig["srcs"])]
        weight, woff, wu, self.pc = o["weight"], 0, None, None
        ref_weight = o["weight"]
        if case["op"] == "dgrad1":
            weight, woff = o["weight_full"], o["row0"] * 9 * sig["cin_total"]
        if case.get("up2") or case["op"] == "up2d":
            self.pc = _packed_deconv(case, o, dt, dev)
            plain = self.pc.wf if case["op"] == "fwd" else self.pc.wd
            assert torch.equal(plain, o["weight"]), "falnet_pack_weights disagrees with the table's packing of the master weight"
            weight, wu = (self.pc.wf, self.pc.wu) if case["op"] == "fwd" else (self.pc.wdd, None)
        if fault_row is not None:  # the kernel's copy (of the operand the variant under test reads) loses one element; the reference keeps it
            if case["op"] == "dgrad1":
                weight = weight.clone()
                weight[o["row0"]:o["row0"] + sig["w_rows"]] = _zero_one_weight(o["weight"], fault_row)
            elif wu is not None:
                wu = _zero_one_weight(wu, fault_row)
            else:
                weight = _zero_one_weight(weight, fault_row)
        for t in (weight, wu, addend, o["bias"], o["actout"], o["pool_actout"]):  # (launches read memory, not strides)
            assert t is None or t.is_contiguous()
        old = ops.AUTOTUNE
        ops.AUTOTUNE = False
        try:
            if case["op"] == "up2d":
                pc = self.pc
                if fault_row is not None:
                    pc = ops.PackedConv("edge-fault", self.pc.weight, None, [case["cin"]], 1)
                    pc.wdd, pc.cin_pad, pc.cout_pad = weight, self.pc.cin_pad, self.pc.cout_pad
                self.call = ops.deconv_dgrad_call(dt, o["srcs"][0], pc, B, self.out, o["actout"], name=case["name"], ws_owner=OWNER)
            else:
                self.call = ops.conv_call(
                    dt, srcs, sig["IH"], sig["IW"], weight, sig["cin_total"], sig["taps"], sig["w_taps"], sig["w_rows"], sig["stride"], B, sig["TH"],
                    sig["TW"], self.out, OH, OW, Cout, cst, out_layout=sig["out_layout"], out_step=(sig["osy"], sig["osy"], sig["ooy"], sig["oox"]),
                    bias=o["bias"], addend=addend, act=sig["act"], actout=o["actout"], actout_kind=sig["actout_kind"], weight_offset_elems=woff,
                    name=case["name"] + label, autotune=False, ws_owner=OWNER, pool_out=self.pool_out, pool_mode=sig["pool_mode"],
                    pool_actout=o["pool_actout"], pool_actout_kind=sig["pool_actout_kind"], weight_up2=wu)
        finally:
            ops.AUTOTUNE = old
        self.keep = (weight, wu, srcs)
        # the reference sees the launch: its signature is read back from the descriptor
        self.sig = R.parse_signature(ops.conv_signature(self.call.desc))
        assert self.sig == {k: sig[k] for k in self.sig}, (self.sig, sig)
        self.ws = ops._splitk_workspace(dev, OWNER) if self.sig["ws"] else None
        assert (self.call.desc.splitk_ws or 0) == (0 if self.ws is None else self.ws.data_ptr())
        if case["op"] == "up2d":
            res = R.conv_ref(E.up2d_plain_sig(self.sig), o["srcs"], ref_weight, pool_actout=o["actout"])
            self.ref = {"out": (res["pool_ref"], res["pool_mag"])}
        else:
            res = R.conv_ref(self.sig, o["srcs"], ref_weight, o["bias"], o["addend"], o["actout"], o["pool_actout"])
            self.ref = {}
            if self.sig["out"]:
                self.ref["out"] = (res["ref"], res["mag"])
            if self.sig["pool"]:
                self.ref["pool"] = (res["pool_ref"], res["pool_mag"])
        self.nreal = case.get("cout", Cout) if case["op"] == "fwd" else case.get("cin", Cout) if case["op"] == "up2d" else Cout

    def refill(self):
        if self.out is not None:
            if self.alias:
                self.out.copy_(self.o["addend"])
            else:
                self.out.fill_(NAN)
        if self.pool_out is not None:
            self.pool_out.fill_(NAN)

    def got(self):
        g = {}
        if "out" in self.ref:
            g["out"] = self.out
        if "pool" in self.ref:
            g["pool"] = self.pool_out
        return g

    def compare(self):
        return {k: R.compare(t, *self.ref[k], self.out_dt if k == "out" else self.dt, MAG_COEF) for k, t in self.got().items()}

    def bad_mask(self):
        return {k: R.violations(t, *self.ref[k], self.out_dt if k == "out" else self.dt, MAG_COEF) for k, t in self.got().items()}

    def check(self, variant, ksplit, what=""):
        """The per-launch assertions on what the last launch left."""
        parts = self.compare()
        ctx = (self.case["name"] + self.label, _name(self.dt), variant, ksplit, what)
        assert parts, ctx
        for part, r in parts.items():
            assert r["mapped"] > 0, (part, ctx)
            assert r["bad"] == 0, (part, ctx, r)
            assert r["unmapped_written"] == 0, (part, ctx, "writes outside the mapped elements", r)
            assert r["maxnorm_rel"] <= TOL[self.dt], (part, ctx, r)
        if self.sig["out_layout"] == R.OUT_NHWC and self.nreal < self.sig["Cout"]:  # zero weight rows, zero bias: exact zeros
            for t in self.got().values():
                assert float(t[..., self.nreal:self.sig["Cout"]].float().abs().max()) == 0.0, (ctx, "padded channels not zero")
        if self.ws is not None:
            assert int((self.ws != 0).sum()) == 0, (ctx, "split-K workspace / tile counters not returned to zero")
        return parts

    def run(self, variant, ksplit):
        d = self.call.desc
        d.variant, d.ksplit = variant, ksplit
        kernel = _kernel_name(d)
        self.refill()
        _launch(self.call)
        parts = self.check(variant, ksplit, kernel)
        if variant == 19:  # the K slices are summed in slice order whichever arrives last: the same bits again
            first = self.out.clone()
            self.refill()
            _launch(self.call)
            assert torch.equal(first.view(torch.int16), self.out.view(torch.int16)), (variant, ksplit, "run-to-run difference")
            self.check(variant, ksplit, kernel)
        _report(self.case["name"] + self.label, self.dt, variant, ksplit, kernel, parts)
        return parts


SINGLE = [(c, dt) for c, dt in E.launches() if c["op"] != "dgrad2"]


@pytest.mark.parametrize("case,dt", SINGLE, ids=[f"{c['name']}-{_name(dt)}" for c, dt in SINGLE])
def test_every_applicable_variant_per_element(case, dt):
    b = Built(case, dt)
    todo = E.choices(case, "", b.sig, dt)
    assert todo
    for variant, ksplit in todo:
        b.run(variant, ksplit)


def _expected_codes(out):
    """include/falnet_hip.h, pool_code: per pooled element the one-hot bit 2 * row + column of the FIRST maximum of its 2x2 window in row-major
    order (strict >, on the stored values), 0 when the maximum is not > 0; channel c in byte c / 2, low nibble for even c."""
    B, H, W, Cc = out.shape
    w = out.float().view(B, H // 2, 2, W // 2, 2, Cc)
    a, b_, c, d = w[:, :, 0, :, 0], w[:, :, 0, :, 1], w[:, :, 1, :, 0], w[:, :, 1, :, 1]
    top, low = torch.maximum(a, b_), torch.maximum(c, d)
    idx = torch.where(low > top, torch.where(d > c, 3, 2), torch.where(b_ > a, 1, 0))
    nib = torch.where(torch.maximum(top, low) > 0, 1 << idx, 0).to(torch.uint8)
    return nib[..., 0::2] | (nib[..., 1::2] << 4)


@pytest.mark.parametrize("dt", E.H16, ids=_name)
def test_fused_max_pool_argmax_codes(dt):
    """Case M on variant 23 with pool_code and `out` kept: the pooled map and `out` hold the bound, and the codes are the header's definition
    evaluated on the kernel's OWN stored full-resolution output."""
    b = Built(E.BY_NAME["M"], dt)
    s = b.sig
    codes = torch.full((s["B"], s["OH"] // 2, s["OW"] // 2, s["out_cstride"] // 2), 0xFF, dtype=torch.uint8, device=_dev())
    b.call.desc.pool_code = codes.data_ptr()
    b.call.desc.variant, b.call.desc.ksplit = 23, 1
    kernel = _kernel_name(b.call.desc)
    assert "PoolCodes" in kernel
    b.refill()
    _launch(b.call)
    parts = b.check(23, 1, kernel)
    assert torch.equal(codes, _expected_codes(b.out))
    assert torch.equal(b.pool_out.float(), b.out.float().view(s["B"], s["OH"] // 2, 2, s["OW"] // 2, 2, -1).amax(dim=(2, 4)))
    _report("M+codes", dt, 23, 1, kernel, parts)


class Classes:
    """The four output-parity classes of one stride-2 data gradient: one output tensor, one set of operands, four launches of the table."""

    def __init__(self, case, dt, fault_row=None):
        self.case, self.dt = case, dt
        first = Built(case, dt, "/00", fault_row=fault_row)
        shared = dict(first.o, out=first.out)
        self.members = [first]
        for label in ("/01", "/10", "/11"):
            m = Built(case, dt, label, shared=shared)
            if fault_row is not None:  # (variant 14 wants ONE weight pointer)
                m.call.desc.weight = first.call.desc.weight
            self.members.append(m)
        self.out = first.out
        # the union of the classes maps every element exactly once
        ref = torch.full_like(first.ref["out"][0], NAN)
        mag = torch.full_like(ref, NAN)
        count = torch.zeros_like(ref)
        for m in self.members:
            r, g = m.ref["out"]
            mp = ~torch.isnan(r)
            count += mp
            ref[mp], mag[mp] = r[mp], g[mp]
        assert bool((count == 1).all()), "the four classes do not cover the output exactly once"
        self.ref, self.mag = ref, mag

    def check_union(self, what):
        r = R.compare(self.out, self.ref, self.mag, self.dt, MAG_COEF)
        ctx = (self.case["name"], _name(self.dt), what)
        assert r["mapped"] == self.out.numel() and not bool(torch.isnan(self.out.float()).any()), (ctx, "a sentinel remains")
        assert r["bad"] == 0 and r["maxnorm_rel"] <= TOL[self.dt], (ctx, r)
        ws = self.members[0].ws
        assert int((ws != 0).sum()) == 0, (ctx, "split-K workspace not returned to zero")
        return {"out": r}


DGRAD2 = [(c, dt) for c, dt in E.launches() if c["op"] == "dgrad2"]


@pytest.mark.parametrize("case,dt", DGRAD2, ids=[f"{c['name']}-{_name(dt)}" for c, dt in DGRAD2])
def test_stride2_dgrad_classes_per_element(case, dt):
    cl = Classes(case, dt)
    # (a) four single launches per gather variant: each class alone leaves the other three classes' elements untouched
    for m in cl.members:
        for variant, ksplit in E.choices(case, m.label, m.sig, dt):
            m.run(variant, ksplit)
    # (b) one fused gather launch, (c) the LDS-DMA form on even maps
    forms = [("multi", dict(ksplit=1)), ("multi", dict(ksplit=4)), ("multi-bn32", dict(bn=32))]
    if case["H"] % 2 == 0 and case["W"] % 2 == 0:
        forms.append(("s2d", dict(s2d=True)))
    for what, kw in forms:
        call = ops.conv_multi_call([m.call for m in cl.members], name=case["name"], **kw)
        cl.out.fill_(NAN)
        call()
        torch.cuda.synchronize()
        parts = cl.check_union(what)
        if what == "s2d":
            first = cl.out.clone()
            cl.out.fill_(NAN)
            call()
            torch.cuda.synchronize()
            assert torch.equal(first.view(torch.int16), cl.out.view(torch.int16)), "variant 14: run-to-run difference"
        _report(case["name"], dt, 14 if what == "s2d" else {"multi-bn32": 11}.get(what, 1), kw.get("ksplit", 1), call.tag, parts)
    assert case["name"] != "P14" or forms[-1][0] == "s2d"


# one variant of each kernel family: (family, case, variant, ksplit)
FAULTS = [("gather", "A", 1, 1), ("halo-patch", "A", 4, 1), ("weight-stationary", "A", 10, 1), ("dma", "A", 13, 1), ("dma2", "A", 21, 1),
          ("dma16", "A", 23, 1), ("stride-2 dma", "I", 15, 1), ("deep", "K", 19, 4), ("wave32", "D", 27, 1), ("wave64p", "G", 29, 1),
          ("up2", "Q1", 18, 1), ("up2d", "R1", 26, 1), ("s2d-multi", "P14", 14, 1)]
FAULT_ROW = 1


@pytest.mark.parametrize("family,name,variant,ksplit", FAULTS, ids=[f[0] for f in FAULTS])
def test_bound_catches_one_zeroed_weight_element(family, name, variant, ksplit):
    """One (row, tap, channel) element of the kernel's packed weight zeroed, the reference on the full weight: the element-wise bound must report
    violations, all of them in output channel `row`."""
    dt, case = torch.bfloat16, E.BY_NAME[name]
    if variant == 14:
        cl = Classes(case, dt, fault_row=FAULT_ROW)
        cl.out.fill_(NAN)
        ops.conv_multi_call([m.call for m in cl.members], s2d=True)()
        torch.cuda.synchronize()
        masks = {"out": R.violations(cl.out, cl.ref, cl.mag, dt, MAG_COEF)}
        planar = False
    else:
        b = Built(case, dt, fault_row=FAULT_ROW)
        assert variant in E.EXPECT[(name, 16)]
        b.call.desc.variant, b.call.desc.ksplit = variant, ksplit
        b.refill()
        _launch(b.call)
        masks = b.bad_mask()
        planar = b.sig["out_layout"] == R.OUT_PLANAR_F32
        if b.ws is not None:
            assert int((b.ws != 0).sum()) == 0
    for part, m in masks.items():
        per_channel = m.sum(dim=(0, 2, 3)) if planar else m.sum(dim=(0, 1, 2))
        assert int(per_channel[FAULT_ROW]) > 0, (family, part, "the zeroed weight element went unnoticed")
        per_channel[FAULT_ROW] = 0
        assert int(per_channel.sum()) == 0, (family, part, "violations outside the faulted output channel", per_channel.nonzero().flatten().tolist())


@pytest.mark.parametrize("dt", E.ALL, ids=_name)
@pytest.mark.parametrize("B,H,W,cout,act", E.C3_CASES)
def test_first_layer_c3_per_element(B, H, W, cout, act, dt):
    """falnet_conv3x3_c3 (planar f32 image and f32 OIHW master weights -> NHWC `dt`) under the same bound.  In the 16-bit types the kernel rounds
    BOTH the image and the weights to `dt` (round to nearest) when it builds its MFMA fragments (csrc/conv.hip: conv3x3_c3_kernel, H16<T>::bits
    on the patch element and on the weight) and accumulates in f32; in f32 it multiplies the f32 values as they are.  The reference gets exactly
    those operands: image and weights rounded to `dt`, the bias in f32."""
    dev = _dev()
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + cout)
    x = torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(cout, 3, 3, 3, generator=g) * 0.2
    bias = torch.randn(cout, generator=g) * 0.1
    pc = ops.PackedConv("edge-c3", torch.nn.Parameter(w.to(dev)), torch.nn.Parameter(bias.to(dev)), [3], 1)
    out = torch.full((B, H, W, cout), NAN, dtype=dt, device=dev)
    call = ops.conv_c3_call(dt, x.to(dev), pc, out, act)
    call()
    torch.cuda.synchronize()
    src = {"C": 3, "H": H, "W": W, "bcast": False}
    sig = E.base_sig(dt, [src], H, W, ops.fwd_taps(3), 9, cout, 1, B, H, W, H, W, cout, cout, bias=True, act=act, ws=False)
    xr = x.to(dev).to(dt).permute(0, 2, 3, 1).contiguous()
    wr = w.to(dev).to(dt).permute(0, 2, 3, 1).reshape(cout, 9, 3)
    res = R.conv_ref(sig, [xr], wr, bias.to(dev))
    r = R.compare(out, res["ref"], res["mag"], dt, MAG_COEF)
    assert r["mapped"] == out.numel() and r["bad"] == 0 and r["unmapped_written"] == 0 and r["maxnorm_rel"] <= TOL[dt], r
    _report(f"T-{B}x{H}x{W}-{cout}", dt, -1, 1, call.tag, {"out": r})
