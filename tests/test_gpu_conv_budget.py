"""GPU: the workgroup budget of the conv launch path (falnet_conv2d_wgs / falnet_conv2d_multi_wgs, include/falnet_hip.h).

Every persistent conv kernel strides its tile loop by the grid width, so which workgroup computes a tile does not enter the arithmetic: a
budgeted launch must give the SAME BITS as the full grid.  Every budgeted family runs through a forced variant on the smallest shapes that
still give several tiles per workgroup -- B = 2, a 32 x 64 map, 64 input channels, 64 / 128 output channels: 8 tiles of 16 x 32, 16 of
8 x 32, 32 of 4 x 32, one or more output-channel blocks; the deconv kernels on their own geometry (variant 26: upstream gradient at twice the
map, variant 18: source at half a 64 x 128 map, the stride-2 kernels between a 64 x 128 and a 32 x 64 map) -- with budgets 1 (all tiles
through one workgroup column), 3 and 5 (uneven tile counts), the tile count and 4096 (= no budget), compared with torch.equal on every output.
Budget 0 is also held to the float64 reference of tests/_conv_ref.py once per family, so that identical is not identically wrong.  A
family without a persistent grid ignores the budget, a negative one is refused before anything is launched, and a fused Stage-1 step
with the label pass under a budget gives the bits of the step without one (tests/_label_budget_step.py, fresh processes)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from fal_net_amd import _lib as L
from fal_net_amd import ops

import _conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, W, CIN = 2, 32, 64, 64
BUDGETS = (1, 3, 5, "ntiles", 4096)
# family -> (kind, variant, tile rows, output channels per block)
FAMILIES = {
    "v23": ("plain", 23, 16, 64), "v23_pool": ("pool", 23, 16, 64), "v23_codes": ("codes", 23, 16, 64), "v23_planar": ("planar", 23, 16, 64),
    "v24": ("plain", 24, 4, 64), "v25": ("plain", 25, 8, 64), "v13": ("plain", 13, 16, 64), "v17": ("plain", 17, 4, 64), "v20": ("plain", 20, 8, 64),
    "v26": ("up2d", 26, 16, 64), "v18": ("up2", 18, 16, 32), "v15": ("s2f", 15, 8, 64), "s2d": ("s2d", 14, 8, 32),
    "v10": ("plain", 10, 8, 64), "v16": ("plain", 16, 4, 64),
}


class Case:
    """One launch on seeded operands: run(budget) -> return code, outs = the buffers it writes, ref() = [(got, ref, mag, dtype)] in float64."""

    def __init__(self, family, dt, cout, variant=None, ksplit=None, cin=CIN, h=H, w=W):
        kind, v, th, bn = FAMILIES.get(family, ("plain", None, 16, 64))  # (not in the table: built on the gather kernel, variant / ksplit set below)
        self.kind, self.dt, self.cout = kind, dt, cout
        g = torch.Generator(device=DEV).manual_seed(1000 * len(family) + cout + (7 if dt == torch.float16 else 0))
        rnd = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g, device=DEV) * scale).to(dt)  # noqa: E731
        nan = lambda *shape, dtype=dt: torch.full(shape, float("nan"), dtype=dtype, device=DEV)  # noqa: E731
        self.bias = torch.randn(max(cout, 32), generator=g, device=DEV) * 0.3
        kw = dict(bias=self.bias, act=L.ACT_RELU, variant=v)
        self.outs, self.members, self.call = {}, None, None
        self.ny = (cout + bn - 1) // bn
        self.ntiles = B * ((w + 31) // 32) * ((h + th - 1) // th)
        if kind in ("plain", "pool", "codes"):
            self.x, self.w = rnd(B, h, w, cin), rnd(cout, 9, cin, scale=(9 * cin) ** -0.5)
            if kind != "codes":
                self.outs["out"] = nan(B, h, w, cout)
            if kind != "plain":
                self.outs["pool"] = nan(B, h // 2, w // 2, cout)
                kw["pool_out"] = self.outs["pool"]
            if kind == "codes":
                self.outs["codes"] = torch.full((B, h // 2, w // 2, cout // 2), 0xFF, dtype=torch.uint8, device=DEV)  # (a code byte never has all bits set)
                kw["pool_code"] = self.outs["codes"]
            if v is None:
                kw.update(autotune=False)
            self.call = ops.conv_call(dt, [ops.nhwc_src(self.x)], h, w, self.w, cin, ops.fwd_taps(3), 9, cout, 1, B, h, w, self.outs.get("out"), h, w,
                                      cout, cout, **kw)
            if variant is not None:
                self.call.desc.variant, self.call.desc.ksplit = variant, ksplit or 1
        elif kind == "planar":  # three planar f32 channels from a 32-row packed weight (the VGG adjoint's last launch)
            self.cout, self.ny = 3, 1
            self.x, self.w = rnd(B, h, w, cin), rnd(32, 9, cin, scale=(9 * cin) ** -0.5)
            self.outs["out"] = nan(B, 3, h, w, dtype=torch.float32)
            self.call = ops.conv_call(dt, [ops.nhwc_src(self.x)], h, w, self.w, cin, ops.fwd_taps(3), 9, 32, 1, B, h, w, self.outs["out"], h, w, 3, 0,
                                      out_layout=L.OUT_PLANAR_F32, bias=self.bias, variant=v)
        elif kind == "up2d":  # deconv data gradient on the low-resolution grid: upstream gradient at twice the map, 2x2 taps over pair pixels
            self.x, self.w = rnd(B, 2 * h, 2 * w, cin), rnd(cout, 4, 4 * cin, scale=(16 * cin) ** -0.5)
            self.outs["out"] = nan(B, h, w, cout)
            self.call = ops.conv_call(dt, [ops.nhwc_src(self.x)], 2 * h, 2 * w, self.w, 4 * cin, ops.UP2D_TAPS, 4, cout, 1, B, h, w, self.outs["out"], h, w,
                                      cout, cout, variant=v)
        elif kind == "up2":  # deconv forward in sub-pixel form: source at half a 64 x 128 map; tiles are counted on the source grid
            # OIHW weights in multiples of 1/64 below 1/4: the plain (wf) and the summed sub-pixel (wu) operands hold them exactly in 16 bits
            wt = torch.randint(-16, 17, (cout, cin, 3, 3), generator=g, device=DEV).float() / 64
            pc = ops.PackedConv("budget-up2", torch.nn.Parameter(wt), None, [cin], 1)
            pc.up2 = True
            pc.alloc(dt, torch.device(DEV, torch.cuda.current_device()))
            pc.pack_call()()
            ops.pack_up2_call([pc], dt, torch.device(DEV, torch.cuda.current_device()))()
            assert (pc.cout_pad, pc.cin_pad) == (cout, cin)
            self.pc, self.x, self.w = pc, rnd(B, h, w, cin), pc.wf
            self.outs["out"] = nan(B, 2 * h, 2 * w, cout)
            self.call = ops.conv_call(dt, [ops.nhwc_src(self.x)], 2 * h, 2 * w, pc.wf, cin, ops.fwd_taps(3), 9, cout, 1, B, 2 * h, 2 * w, self.outs["out"],
                                      2 * h, 2 * w, cout, cout, weight_up2=pc.wu, bias=self.bias, act=L.ACT_ELU, variant=v)
        elif kind == "s2f":  # forward 3x3 stride 2: a 64 x 128 source, the 32 x 64 map out
            self.x, self.w = rnd(B, 2 * h, 2 * w, cin), rnd(cout, 9, cin, scale=(9 * cin) ** -0.5)
            self.outs["out"] = nan(B, h, w, cout)
            self.call = ops.conv_call(dt, [ops.nhwc_src(self.x)], 2 * h, 2 * w, self.w, cin, ops.fwd_taps(3), 9, cout, 2, B, h, w, self.outs["out"], h, w,
                                      cout, cout, **kw)
        elif kind == "s2d":  # the four parity classes of a stride-2 data gradient in one launch: upstream gradient 32 x 64, gradient 64 x 128
            self.x, self.w = rnd(B, h, w, cin), rnd(cout, 9, cin, scale=(9 * cin) ** -0.5)
            self.outs["out"] = nan(B, 2 * h, 2 * w, cout)
            self.members = [ops.conv_call(dt, [ops.nhwc_src(self.x)], h, w, self.w, cin, ops.dgrad_taps_s2(py, px), 9, cout, 1, B, h, w, self.outs["out"],
                                          2 * h, 2 * w, cout, cout, out_step=(2, 2, py, px), autotune=False) for py in range(2) for px in range(2)]
            assert B * 2 * 2 * self.ny < 256  # fewer sixteen-row tiles than CUs: the launcher takes eight-row tiles (th above)
        else:
            raise AssertionError(kind)

    def run(self, budget):
        for name, t in self.outs.items():
            t.fill_(0xFF if name == "codes" else float("nan"))
        if self.members is not None:
            arr = (L.Conv * 4)()
            for i, m in enumerate(self.members):
                C.memmove(C.byref(arr[i]), C.byref(m.desc), C.sizeof(L.Conv))
                arr[i].variant = 14
            rc = L.lib().falnet_conv2d_multi_wgs(arr, 4, budget, L.stream_ptr())
        else:
            rc = L.lib().falnet_conv2d_wgs(self.call.ref, budget, L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def fetch(self, budget):
        rc = self.run(budget)
        assert rc == 0, (budget, rc, L.lib().falnet_last_error().decode(errors="replace"))
        return {k: t.clone() for k, t in self.outs.items()}

    def workgroups(self, budget):
        return None if self.call is None else L.lib().falnet_conv2d_workgroups(self.call.ref, budget)

    def ref(self):
        """[(name, got, ref, mag, stored dtype)] of the CURRENT buffers against tests/_conv_ref.conv_ref."""
        out = self.outs.get("out")
        if self.kind == "s2d":
            ref = mag = None
            for m in self.members:
                r = R.conv_ref(R.parse_signature(ops.conv_signature(m.desc)), [self.x], self.w)
                ref = r["ref"] if ref is None else torch.where(torch.isnan(ref), r["ref"], ref)
                mag = r["mag"] if mag is None else torch.where(torch.isnan(mag), r["mag"], mag)
            return [("out", out, ref, mag, self.dt)]
        if self.kind == "up2d":
            # pair pixel (u, v) holds the four upstream pixels (2u - 1 + e, 2v - 1 + f) as channels e 2C + f C + c (zero outside the map); the launch is
            # the dense 2x2-tap convolution out[i, j] = sum_(du, dv) W[:, 2 du + dv, :] . pair[i + du, j + dv] over them (csrc/conv_dma.hip)
            g, (h, w, c) = self.x, self.outs["out"].shape[1:3] + (self.x.shape[3],)
            gp = torch.nn.functional.pad(g.double(), (0, 0, 1, 1, 1, 1))
            pair = gp.view(B, h + 1, 2, w + 1, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(B, h + 1, w + 1, 4 * c)
            sig = R.parse_signature(ops.conv_signature(self.call.desc))
            sig.update(srcs=[{"C": 4 * c, "H": h + 1, "W": w + 1, "bcast": False}], IH=h + 1, IW=w + 1)
            r = R.conv_ref(sig, [pair], self.w)
            return [("out", out, r["ref"], r["mag"], self.dt)]
        sig = R.parse_signature(ops.conv_signature(self.call.desc))
        r = R.conv_ref(sig, [self.x], self.w, self.bias)
        res = []
        if out is not None:
            res.append(("out", out, r["ref"], r["mag"], torch.float32 if self.kind == "planar" else self.dt))
        if "pool" in self.outs:
            res.append(("pool", self.outs["pool"], r["pool_ref"], r["pool_mag"], self.dt))
        return res


def _expected_wgs(c, budget):
    full = 256 if not budget else min(budget, 256)
    return min(max(1, full // c.ny), c.ntiles) * c.ny


# (the planar form has three output channels whatever `cout` says: one case per type)
FAMILY_COUT = [(f, co) for f in sorted(FAMILIES) for co in (64, 128) if not (f == "v23_planar" and co == 128)]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("family,cout", FAMILY_COUT)
def test_budgeted_launch_gives_the_bits_of_the_full_grid(family, cout, dt):
    c = Case(family, dt, cout)
    base = c.fetch(0)
    for name, t in base.items():  # every element written: the sentinel is gone
        assert (not bool((t == 0xFF).any())) if name == "codes" else bool(torch.isfinite(t.float()).all()), name
    if c.call is not None:
        assert c.workgroups(0) == _expected_wgs(c, 0), (c.workgroups(0), c.ntiles, c.ny)
    for b in BUDGETS:
        b = c.ntiles if b == "ntiles" else b
        if c.call is not None:  # the launch really runs on the budgeted grid
            assert c.workgroups(b) == _expected_wgs(c, b), (b, c.workgroups(b), c.ntiles, c.ny)
        got = c.fetch(b)
        for name in base:
            assert torch.equal(got[name], base[name]), (family, name, b)
    assert c.ntiles >= 8 and (c.call is None or c.workgroups(1) == c.ny)  # budget 1: all tiles through one workgroup column


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_full_grid_against_float64(family):
    c = Case(family, torch.bfloat16, 64)
    c.fetch(0)
    parts = c.ref()
    assert parts
    for name, got, ref, mag, dt in parts:
        r = R.compare(got, ref, mag, dt)
        assert r["mapped"] > 0 and r["bad"] == 0 and r["unmapped_written"] == 0, (family, name, r)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("which", ["gather", "deep"])
def test_a_family_without_a_persistent_grid_ignores_the_budget(which, dt):
    if which == "gather":
        c = Case("gather", dt, 64, variant=1)
    else:  # variant 19 on an 8 x 16 map: 128 input channels in four K slices of 32
        c = Case("deep", dt, 64, variant=19, ksplit=4, cin=128, h=8, w=16)
    name = C.create_string_buffer(160)
    assert L.lib().falnet_conv2d_kernel_name(c.call.ref, name, 160) == 0, L.lib().falnet_last_error()
    assert (b"conv_igemm_kernel" if which == "gather" else b"conv3x3_deep_kernel") in name.value
    base = c.fetch(0)
    assert bool(torch.isfinite(base["out"].float()).all())
    got = c.fetch(3)
    assert torch.equal(got["out"], base["out"])
    assert c.workgroups(3) == c.workgroups(0) > 3
    for nm, o, ref, mag, d in c.ref():
        r = R.compare(o, ref, mag, d)
        assert r["bad"] == 0 and r["unmapped_written"] == 0, (which, r)


@pytest.mark.parametrize("family", ["v23", "v1", "s2d"])
def test_a_negative_budget_is_refused_before_the_launch(family):
    c = Case("gather", torch.bfloat16, 64, variant=1) if family == "v1" else Case(family, torch.bfloat16, 64)
    rc = c.run(-1)
    assert rc != 0
    assert b"budget" in L.lib().falnet_last_error()
    assert bool(torch.isnan(c.outs["out"].float()).all())  # nothing was launched
    if c.call is not None:
        assert c.workgroups(-1) < 0
    assert c.run(0) == 0 and bool(torch.isfinite(c.outs["out"].float()).all())


def _step_child(budget):
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_label_budget_step.py"), str(budget)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_step_is_bit_identical_under_a_label_budget():
    """Four fused Stage-1 steps (bf16, B = 2, 64 x 128, deterministic mode; the third and fourth through falnet_replay) with the label pass
    on three workgroups against the same steps without a budget: loss, flat gradients, flat parameters and disparity bit-equal after every step."""
    on, off = _step_child(3), _step_child(0)
    assert on["replayed"] and off["replayed"]
    assert on["label_plan_keys"] == [[2, 64, 128, False, 3]] and off["label_plan_keys"] == [[2, 64, 128, False]]
    assert on["budgeted"] >= 6 and on["cut"] >= 6 and off["budgeted"] == 0  # the label convs behind the first layer run on fewer workgroups
    assert len(on["steps"]) == 4 and len({tuple(s) for s in on["steps"]}) == 4  # (the steps differ from each other: the digests see the update)
    assert on["steps"] == off["steps"]
