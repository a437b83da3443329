"""Every weight-gradient kernel behind falnet_wgrad, both slab reduces, the three bias-gradient entry points and
falnet_wgrad_const_plane, through the C ABI, held to the float64 references of tests/_wgrad_ref.py with torch.equal: the operands are
small integers (sources in [0, 15], output gradient in [-7, 8]), so every f32 product and partial sum is an integer below 2^24 and the
result does not depend on summation order, split count, MFMA shape or the order of f32 atomics.  Any dropped, doubled or misplaced
pixel, tap, channel or slab fails the comparison, and the message names the first element that differs.

Per case (tests/_wgrad_cases.py: run_case): NaN over the workspace plus a 4 KiB guard; the launch with the variant forced; the guard
still NaN; the float64 sum of the slabs equal to the reference at every (tap, co < cout, real input channel); falnet_wgrad_reduce into
a NaN-filled gradient (accumulate 0) and onto 7 (accumulate 1); where the kernel fuses it, the bias gradient added into zeros with the
elements >= cout untouched.

Kernel instantiations reached (bf16 and f16 each; f32 too where it exists): wgrad_kernel<T> (f32), wgrad3x3_patch_kernel<T,1,1> (f32),
<T,1,2>, <T,2,1>, wgrad3x3_s2_kernel<T,1> and <T,2>, wgrad3x3_c3_kernel<T>, wgrad3x3_c3wave_kernel<T>,
wgrad3x3_rows16_kernel<T,4,2,false> and <T,4,2,true>, wgrad3x3_rows8s2_kernel<T,2>, wgrad3x3_wave32_kernel<T,1,false>, <T,2,false>,
<T,2,true>, wgrad_reduce_kernel, wgrad_reduce_batched_kernel (1, 3, 9 taps), bias_grad_kernel<T>, bias_grad_batched_kernel<T> (atomic
and deterministic form) with bias_grad_finish_kernel, and the kernels of falnet_wgrad_const_plane.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import _wgrad_cases as K  # noqa: E402
import _wgrad_ref as R  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402

DEV = "cuda"
NAN = float("nan")
F32, F64 = torch.float32, torch.float64
RUNS = [(c, dt) for c in K.CASES for dt in c["dtypes"]]


@pytest.mark.parametrize("case,dtype", RUNS, ids=[f"{c['name']}-{K.DTYPE_NAME[dt]}" for c, dt in RUNS])
def test_wgrad_exact(case, dtype):
    """Every split count of the case; PLAN = the (variant, nsplit) fal_net_amd.ops._wgrad_plan returns, whose variant must be the case's."""
    K.exactness(case)
    for nsplit in K.split_counts(case):
        planned = nsplit == K.PLAN
        if planned:
            variant, nsplit = K.planned(case, dtype, DEV)
            assert variant == case["variant"], (case["name"], variant)
        out = K.run_case(case, dtype, nsplit, DEV)
        if case["variant"] in (3, 4, 5, 6, 7, 8, 9) or (case["variant"] == 0 and case["kernel"].startswith("wgrad3x3_patch")):
            assert out["fuses_bias"] == 1, out["what"]  # (not deterministic mode: every halo / streaming kernel sums the bias gradient)
        else:
            assert out["fuses_bias"] == 0, out["what"]
        if case["forms"] == ["planar"] and nsplit > K.geom(case)["npatch"]:
            assert K.c3_form(case, out, nsplit) == case["c3form"], out["what"]
        if planned and case.get("misalign"):  # the plan asked the library: the patch form's split count, and the patch form in the slabs
            assert nsplit == min(256, K.geom(case)["npatch"]) >= 2 and K.c3_form(case, out, nsplit) == "patch", out["what"]


def test_first_layer_forms():
    """Variant 6: an aligned image of width % 4 == 0 takes the wave form, the same image with its pointer moved by one float the patch
    form (seen in the slabs), and both give the integers of the same reference."""
    wave, patch = K.BY_NAME["c3_wave_16x64"], K.BY_NAME["c3_misaligned_16x64"]
    assert all(torch.equal(a, b) for a, b in zip(K.host_operands(wave)[0], K.host_operands(patch)[0]))
    for dtype in K.H16:
        assert K.c3_form(wave, K.run_case(wave, dtype, 20, DEV), 20) == "wave"
        assert K.c3_form(patch, K.run_case(patch, dtype, 20, DEV), 20) == "patch"
        assert torch.equal(K.reference(wave, dtype, DEV)["oihw"], K.reference(patch, dtype, DEV)["oihw"])


# ------------------------------------------------------------------------------------------ mutations that must fail
@pytest.mark.parametrize("kind", sorted(K.MUTATION_CASES))
def test_mutations_are_seen(kind):
    """One gout pixel zeroed for the kernel only (at the last valid column of a ragged strip, at row 0, at the first pixel of the second
    split range), and the reduce told one slab too few: each must produce a mismatch."""
    case = K.BY_NAME[K.MUTATION_CASES[kind]]
    desc = K.geom(case)["desc"]
    nsplit = 3
    assert desc["TW"] % 32 == 1  # a ragged second strip with one valid column
    nranges = nsplit if kind == "rows" else nsplit * 8 // (desc["gC"] // 32)
    pixels = {"last column of the ragged strip": (1, 4, desc["TW"] - 1), "row 0": (0, 0, 5),
              "first pixel of the second range": K.range_start_pixel(case, nranges)}
    assert pixels["first pixel of the second range"] != (0, 0, 0)
    for dtype in case["dtypes"]:
        K.run_case(case, dtype, nsplit, DEV)  # unmutated: passes
        for name, px in pixels.items():
            out = K.run_case(case, dtype, nsplit, DEV, zero_pixel=px, strict=False)
            assert out["guard"] and not out["slab"] and not out["reduce"] and not out["accumulate"] and out["bias"] is False, (name, out["messages"])
        out = K.run_case(case, dtype, nsplit, DEV, reduce_nsplit=nsplit - 1, strict=False)
        assert out["slab"] and not out["reduce"] and not out["accumulate"], out["messages"]


# ------------------------------------------------------------------------------------------ the batched slab reduce
# ntaps, cin_total, cin, c0_real, c0_pad, cout, w_rows, nsplit, groups
REDUCE_ENTRIES = [
    (9, 32, 32, 32, 32, 32, 32, 5, 1),
    (3, 96, 96, 96, 96, 49, 64, 13, 3),       # cob 10: cout is no multiple of it; 13 slabs in 3 groups
    (1, 384, 384, 384, 384, 7, 32, 8, 2),     # groups = nsplit / 4
    (9, 1024, 1024, 1024, 1024, 5, 32, 4, 1),
    (9, 1056, 1056, 1056, 1056, 3, 32, 6, 1),  # two trips of 1024 packed channels
    (9, 64, 20, 3, 32, 33, 64, 18, 4),        # padded first channel group: c0_real 3, c0_pad 32; 18 slabs in 4 groups
    (3, 1056, 1030, 1000, 1024, 2, 32, 9, 2),  # two trips, two groups of channels and slabs
]
GAP = 5  # floats between the entries' gradients


def reduce_table(entries, dev, accumulate, seed=3):
    """Device slabs (integers in [-8, 8] everywhere, padding rows and columns included), one flat gradient buffer with GAP sentinel
    floats between the entries, the descriptor table and the float64 reference of every entry."""
    descs = (L.ReduceDesc * len(entries))()
    slabs, refs, spans = [], [], []
    off = GAP
    for (ntaps, cin_total, cin, c0_real, c0_pad, cout, w_rows, nsplit, groups) in entries:
        spans.append((off, cout * cin * ntaps, groups))
        off += cout * cin * ntaps + GAP
    flat = torch.full((off,), 123.0, dtype=F32, device=dev)
    blk = 0
    for i, (ntaps, cin_total, cin, c0_real, c0_pad, cout, w_rows, nsplit, groups) in enumerate(entries):
        R.assert_exact(nsplit, 8, 1)
        ws = R.int_operand((nsplit, ntaps, w_rows, cin_total), -8, 8, seed + i, device=dev)
        slabs.append(ws)
        cols = torch.tensor(R.unpack_columns(dict(cin=cin, c0_real=c0_real, c0_pad=c0_pad)), device=dev)
        refs.append(R.slab_sum(ws.view(-1), nsplit, ntaps, w_rows, cin_total)[:, :cout][:, :, cols].permute(1, 2, 0).reshape(-1))
        o, n, _ = spans[i]
        flat[o:o + n] = 7.0 if accumulate else (NAN if groups == 1 else 0.0)
        d = descs[i]
        d.partial, d.grad = ws.data_ptr(), flat.data_ptr() + 4 * o
        d.nsplit, d.ntaps, d.w_rows, d.cin_total, d.cout, d.cin, d.c0_real, d.c0_pad, d.groups, d.block_begin = (
            nsplit, ntaps, w_rows, cin_total, cout, cin, c0_real, c0_pad, groups, blk)
        blk += L.lib().falnet_wgrad_reduce_blocks(cout, cin_total, groups)
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    return dict(table=table, n=len(entries), blocks=blk, flat=flat, spans=spans, refs=refs, keep=slabs)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_wgrad_reduce_batched_exact(accumulate):
    """ONE launch over seven entries (1, 3 and 9 taps; cin_total 32 ... 1056; groups 1, 2, 3, 4 with slab counts they do not divide; a
    padded first channel group).  accumulate 0: groups == 1 overwrites NaN, groups > 1 adds into zeros; accumulate 1: everything adds
    onto 7.  The floats between the gradients keep their sentinel."""
    t = reduce_table(REDUCE_ENTRIES, DEV, accumulate)
    assert t["n"] >= 6 and {e[0] for e in REDUCE_ENTRIES} == {1, 3, 9} and {e[8] for e in REDUCE_ENTRIES} >= {1, 3}
    L.check(L.lib().falnet_wgrad_reduce_batched(L.ptr(t["table"]), t["n"], t["blocks"], accumulate, L.stream_ptr()), "wgrad_reduce_batched")
    flat = t["flat"].to(F64)
    mask = torch.ones_like(flat, dtype=torch.bool)
    for i, ((o, n, groups), ref) in enumerate(zip(t["spans"], t["refs"])):
        msg = K._first_bad(flat[o:o + n], ref + (7.0 if accumulate else 0.0))
        assert msg is None, (REDUCE_ENTRIES[i], msg)
        mask[o:o + n] = False
    assert bool((flat[mask] == 123.0).all())


def test_batched_tables_of_more_than_64_entries_are_refused():
    """n = 65 is refused on the host, before any launch (the kernels stage block_begin in a 64-int LDS array)."""
    lib = L.lib()
    dummy = torch.zeros(65 * 64, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(512 * 65, device=DEV)
    assert lib.falnet_wgrad_reduce_batched(L.ptr(dummy), 65, 65, 0, L.stream_ptr()) < 0
    assert "64" in lib.falnet_last_error().decode()
    assert lib.falnet_bias_grad_batched(L.ptr(dummy), 65, 65, 1, L.stream_ptr()) < 0
    assert "64" in lib.falnet_last_error().decode()
    assert lib.falnet_bias_grad_batched_det(L.ptr(dummy), 65, 65, 1, L.ptr(ws), ws.numel(), L.stream_ptr()) < 0
    assert "64" in lib.falnet_last_error().decode()
    torch.cuda.synchronize()
    assert float(ws.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ bias gradients
# gC, cout, npix, blocks: npix below, at and just above eight strides of blocks * rows pixels (rows = 256 / (gC / 8)), and the tail alone
BIAS_ENTRIES = [(32, 17, 8 * 64 * 2 - 3, 2), (32, 32, 8 * 64 * 2, 2), (64, 49, 8 * 32 * 3 + 5, 3), (64, 33, 40, 1), (96, 70, 8 * 21 * 5 + 1, 5),
                (256, 200, 8 * 8 * 2 + 9, 2), (512, 300, 8 * 4 * 3, 3), (512, 511, 7, 1)]


def bias_table(entries, dtype, dev, db_fill):
    descs = (L.BiasGradDesc * len(entries))()
    gs, refs = [], []
    dbs = torch.full((len(entries), 512 + 8), 7.0, dtype=F32, device=dev)
    blk = 0
    for i, (gC, cout, npix, blocks) in enumerate(entries):
        R.assert_exact(npix, 1, 8)
        g = R.int_operand((npix, gC), *R.G_RANGE, 50 + i, dtype, dev)
        gs.append(g)
        refs.append(R.bias_ref(g, cout))
        dbs[i, :cout] = db_fill
        d = descs[i]
        d.g, d.db, d.npix, d.gC, d.cout, d.blocks, d.block_begin = g.data_ptr(), dbs[i].data_ptr(), npix, gC, cout, blocks, blk
        blk += blocks
    return dict(table=torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev), n=len(entries), blocks=blk, dbs=dbs, refs=refs, keep=gs)


def check_bias(t, entries, db_fill):
    for i, (gC, cout, npix, blocks) in enumerate(entries):
        msg = K._first_bad(t["dbs"][i, :cout].to(F64), t["refs"][i] + db_fill)
        assert msg is None, (entries[i], msg)
        assert bool((t["dbs"][i, cout:] == 7.0).all()), entries[i]


@pytest.mark.parametrize("dtype", K.ALL, ids=[K.DTYPE_NAME[d] for d in K.ALL])
def test_bias_grad_batched_exact(dtype):
    """falnet_bias_grad_batched adds (atomics) into a non-zero db; falnet_bias_grad_batched_det adds the same integers through its
    per-block workspace and refuses a workspace that is too small; elements >= cout keep their sentinel."""
    assert {e[0] for e in BIAS_ENTRIES} == {32, 64, 96, 256, 512} and len({e[3] for e in BIAS_ENTRIES}) >= 4
    lib, code = L.lib(), L.dtype_code(dtype)
    t = bias_table(BIAS_ENTRIES, dtype, DEV, 3.0)
    L.check(lib.falnet_bias_grad_batched(L.ptr(t["table"]), t["n"], t["blocks"], code, L.stream_ptr()), "bias_grad_batched")
    check_bias(t, BIAS_ENTRIES, 3.0)
    t = bias_table(BIAS_ENTRIES, dtype, DEV, 3.0)
    ws = torch.full((512 * t["blocks"] + 64,), NAN, dtype=F32, device=DEV)
    assert lib.falnet_bias_grad_batched_det(L.ptr(t["table"]), t["n"], t["blocks"], code, L.ptr(ws), 512 * t["blocks"] - 1, L.stream_ptr()) < 0
    assert bool((t["dbs"][:, :17] == 3.0).all())  # (the refused call launched nothing)
    L.check(lib.falnet_bias_grad_batched_det(L.ptr(t["table"]), t["n"], t["blocks"], code, L.ptr(ws), 512 * t["blocks"], L.stream_ptr()), "bias_grad_batched_det")
    check_bias(t, BIAS_ENTRIES, 3.0)
    assert bool(torch.isnan(ws[512 * t["blocks"]:]).all())


@pytest.mark.parametrize("dtype", K.ALL, ids=[K.DTYPE_NAME[d] for d in K.ALL])
def test_bias_grad_exact(dtype):
    """falnet_bias_grad on the same shapes: accumulate 0 overwrites NaN, accumulate 1 adds onto 7; elements >= cout untouched."""
    lib, code = L.lib(), L.dtype_code(dtype)
    for i, (gC, cout, npix, _) in enumerate(BIAS_ENTRIES):
        g = R.int_operand((npix, gC), *R.G_RANGE, 50 + i, dtype, DEV)
        ref = R.bias_ref(g, cout)
        for acc, fill in ((0, NAN), (1, 7.0)):
            db = torch.full((gC + 8,), 9.0, dtype=F32, device=DEV)
            db[:cout] = fill
            L.check(lib.falnet_bias_grad(L.ptr(g), npix, gC, cout, L.ptr(db), acc, code, L.stream_ptr()), "bias_grad")
            msg = K._first_bad(db[:cout].to(F64), ref + (7.0 if acc else 0.0))
            assert msg is None, ((gC, cout, npix, acc), msg)
            assert bool((db[cout:] == 9.0).all()), (gC, cout, npix, acc)


# ------------------------------------------------------------------------------------------ the constant input plane
@pytest.mark.parametrize("B,IH,IW,stride,gC,cout", [(2, 64, 128, 2, 64, 64), (3, 75, 250, 2, 64, 49), (2, 20, 36, 1, 32, 32), (1, 9, 11, 2, 32, 17)])
@pytest.mark.parametrize("dtype", K.ALL, ids=[K.DTYPE_NAME[d] for d in K.ALL])
def test_wgrad_const_plane_exact(B, IH, IW, stride, gC, cout, dtype):
    """Integer plane values 1 .. 3: the nine masked sums are exact.  The kernel ADDS (twice: 7 + 2 ref), leaves its workspace zero and
    the other columns of the gradient untouched."""
    TH, TW = (IH + stride - 1) // stride, (IW + stride - 1) // stride
    R.assert_exact(2 * B * TH * TW, 3, 8)
    plane = torch.zeros(B, 32, dtype=dtype, device=DEV)
    plane[:, 0] = (torch.arange(B) % 3 + 1).to(dtype).to(DEV)
    gout = R.int_operand((B, TH, TW, gC), *R.G_RANGE, B * 1000 + IW, dtype, DEV)
    desc = dict(B=B, TH=TH, TW=TW, IH=IH, IW=IW, stride=stride, taps=K.taps_of(3), gC=gC, cout=cout, cin_total=1, srcs=[{"C": 1, "form": "bcast"}],
                cin=1, c0_real=1, c0_pad=1)
    ref = R.wgrad_ref(desc, [plane[:, :1].float()], gout)[1][:, 0]  # [cout][9]
    cin = 5
    grad = torch.full((cout, cin, 3, 3), 7.0, device=DEV)
    ws = torch.zeros(B * 9 * gC + 64, device=DEV)
    ws[B * 9 * gC:] = NAN
    for rep in range(2):
        L.check(L.lib().falnet_wgrad_const_plane(L.ptr(gout), L.ptr(plane), plane.stride(0), L.ptr(grad[:, 3:]), cin * 9, L.ptr(ws), B, TH, TW, gC, cout,
                                                 IH, IW, stride, L.dtype_code(dtype), L.stream_ptr()))
    assert float(ws[:B * 9 * gC].abs().max()) == 0.0 and bool(torch.isnan(ws[B * 9 * gC:]).all())
    msg = K._first_bad(grad[:, 3].reshape(cout, 9).to(F64), 7.0 + 2 * ref)
    assert msg is None, msg
    assert float((grad[:, [0, 1, 2, 4]] - 7.0).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ deterministic mode
def test_deterministic_mode_child():
    """FALNET_DETERMINISTIC=1 in a child process (the switch is read when the library loads; tests/_wgrad_det.py): one case per kernel
    gives the same integers, no kernel fuses the bias gradient, falnet_bias_grad_batched is refused, variant 6 takes the patch form, and
    the batched reduce / bias tables with groups 1 give the same integers."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "_wgrad_det.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["deterministic"] == 1 and res["cases"] >= len(K.DET_CASES) and set(res["kernels"]) == set(K.KERNELS)
    assert res["fused_bias"] == 0 and res["bias_grad_batched_refused"] == 1 and res["c3_form"] == "patch"
    assert res["reduce_entries"] == len(REDUCE_ENTRIES) and res["bias_entries"] == len(BIAS_ENTRIES)
