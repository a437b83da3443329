"""GPU: every kernel choice the committed autotune cache pins, at its own launch signature, against a float64 reference.

fal_net_amd/autotune_cache.json decides which (variant, ksplit) every conv launch of the benchmark's plans runs; _autotune_conv picked
them by speed alone.  Here each `conv|...` entry is rebuilt from its key (tests/_conv_ref.py: parse_signature / fill_desc) on seeded
operands, launched ONCE with the cached choice, and held element-wise to tests/_conv_ref.py:conv_ref evaluated in torch float64 on the
device (BLAS GEMMs, no code shared with the kernels):
  * every element the descriptor maps: |got - ref| <= u |ref| + 1e-5 mag (u: unit roundoff of the stored output, mag: the same sums
    over |x| |w| -- one dropped K slice, tap or tile moves an element far beyond 1e-5 mag, f32 accumulation stays below it);
  * every element it does not map (other parity classes of a sub-pixel store, channels >= Cout, rows beyond the tile space) is still the
    NaN sentinel;
  * the max-norm relative error is within test_gpu_ops.TOL;
  * the split-K workspace (and variant 19's tile counters in its last 16 KiB) is all zero again (include/falnet_hip.h: splitk_ws).
FALNET_CACHE_CHOICES_REPORT=<path> appends one JSON line per entry (worst ratio, max-norm error) for reporting."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

from fal_net_amd import _lib as L
from fal_net_amd import ops

import _conv_ref as R
from test_gpu_ops import TOL

pytestmark = pytest.mark.gpu

CACHE = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "autotune_cache.json")
with open(CACHE) as _f:
    _DATA = json.load(_f)
ENTRIES = sorted((k, tuple(v)) for k, v in _DATA.items() if k.startswith("conv|"))
OWNER = ("test-cache-choices",)
MAG_COEF = 1e-5
REPORT = os.environ.get("FALNET_CACHE_CHOICES_REPORT")


def _short(key):
    return hashlib.sha1(key.encode()).hexdigest()[:10]


def test_committed_cache_is_current():
    """The committed cache is replayed only while its header matches the kernel sources (ops._cache); a stale one would be silently
    ignored and the benchmark would re-tune at start-up.  Read from the file itself: FALNET_AUTOTUNE_CACHE cannot mask it."""
    assert _DATA["_meta"] == ops.cache_meta(), "fal_net_amd/autotune_cache.json was tuned with other kernel sources: regenerate it"
    assert len(ENTRIES) > 600


def _elu_out(t):
    return torch.where(t > 0, t, torch.expm1(t))


def run_entry(key, choice, zero_k_slice=None):
    """Build the launch of one cache entry, run it once with `choice` = (variant, ksplit) and compare with conv_ref.
    zero_k_slice = j: the KERNEL's packed weight has input channels [32 j, 32 j + 32) zeroed (the reference keeps them) -- the
    comparison must then report violations.  Returns the report dict."""
    sig = R.parse_signature(key)
    dt = R.DTYPE_CODE[sig["dtype"]]
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(int(_short(key), 16) & 0x7FFFFFFF)
    B, OH, OW, Cout, cst = sig["B"], sig["OH"], sig["OW"], sig["Cout"], sig["out_cstride"]
    planar = sig["out_layout"] == R.OUT_PLANAR_F32
    K, wr, wt = sig["cin_total"], sig["w_rows"], sig["w_taps"]

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, device=dev) * scale).to(dt)

    srcs = [rnd(B, s["C"]) if s["bcast"] else rnd(B, s["H"], s["W"], s["C"]) for s in sig["srcs"]]
    wu = None
    if sig["up2"]:
        # a `deconv` layer: OIHW 3x3 master weight packed by the library into the plain (wf) and the sub-pixel (wu) operands; the values
        # are multiples of 1/64 below 1/4, so wf and the summed taps of wu hold them exactly in 16 bits and one reference serves both
        assert wt == 9 and len(sig["srcs"]) == 1 and dt != torch.float32
        w = torch.randint(-16, 17, (wr, K, 3, 3), generator=g, device=dev).float() / 64
        pc = ops.PackedConv("cache-choice", torch.nn.Parameter(w), None, [K], 1)
        pc.up2 = True
        pc.alloc(dt, dev)
        pc.pack_call()()
        ops.pack_up2_call([pc], dt, dev)()
        assert tuple(pc.wf.shape) == (wr, wt, K) and pc.wu is not None
        weight, wu = pc.wf, pc.wu
        assert torch.equal(weight.double(), w.double().permute(0, 2, 3, 1).reshape(wr, 9, K))
    else:
        weight = rnd(wr, wt, K, scale=(1.0 / (len(sig["taps"]) * K)) ** 0.5)
    wk = weight
    if zero_k_slice is not None:
        assert 32 * (zero_k_slice + 1) <= K and wu is None
        wk = weight.clone()
        wk[:, :, 32 * zero_k_slice:32 * (zero_k_slice + 1)] = 0
    bias = torch.randn(max(wr, Cout), generator=g, device=dev) * 0.3 if sig["bias"] else None
    out_shape = (B, Cout, OH, OW) if planar else (B, OH, OW, cst)
    out_dt = torch.float32 if planar else dt
    out = torch.full(out_shape, float("nan"), dtype=out_dt, device=dev) if sig["out"] else None
    assert not (planar and (sig["addend"] or sig["actout"] or sig["pool"]))
    addend = rnd(*out_shape) if sig["addend"] else None
    actout = None
    if sig["actout"]:
        actout = _elu_out(torch.randn(*out_shape, generator=g, device=dev)).to(dt) if sig["actout_kind"] == R.ACT_ELU else rnd(*out_shape)
    pshape = (B, OH // 2, OW // 2, cst)
    pool_out = torch.full(pshape, float("nan"), dtype=dt, device=dev) if sig["pool"] else None
    pool_actout = _elu_out(torch.randn(*pshape, generator=g, device=dev)).to(dt) if sig["pool_actout"] else None
    # workspace / scratch as ops.conv_call sizes them
    ws = ops._splitk_workspace(dev, OWNER) if sig["ws"] else None
    scratch = ops._deep_scratch(dev, OWNER) if (ws is not None and dt in ops.H16 and sig["TH"] * sig["TW"] <= 128 and len(sig["taps"]) == 9) else None
    ptrs = {"weight": wk.data_ptr(), "out": 0 if out is None else out.data_ptr(), "bias": 0 if bias is None else bias.data_ptr(),
            "addend": 0 if addend is None else addend.data_ptr(), "actout": 0 if actout is None else actout.data_ptr(),
            "pool_out": 0 if pool_out is None else pool_out.data_ptr(), "pool_actout": 0 if pool_actout is None else pool_actout.data_ptr(),
            "weight_up2": 0 if wu is None else wu.data_ptr(), "splitk_ws": 0 if ws is None else ws.data_ptr(),
            "splitk_ws_bytes": 0 if ws is None else ws.numel() * 4}
    for i, t in enumerate(srcs):
        ptrs[f"src{i}"] = t.data_ptr()
    d = R.fill_desc(L.Conv(), sig, ptrs)
    if scratch is not None:
        d.scratch, d.scratch_bytes = scratch.data_ptr(), scratch.numel() * 4
    assert ops.conv_signature(d) == key  # the descriptor launched is the one the cache entry was tuned for
    d.variant, d.ksplit = choice
    lib = L.lib()
    buf = C.create_string_buffer(160)
    rc = lib.falnet_conv2d_kernel_name(C.byref(d), buf, 160)
    assert rc == 0, f"cached choice {choice} does not apply: {lib.falnet_last_error().decode(errors='replace')}"
    rc = lib.falnet_conv2d(C.byref(d), L.stream_ptr())
    assert rc == 0, f"falnet_conv2d {choice} failed: rc {rc} {lib.falnet_last_error().decode(errors='replace')}"
    torch.cuda.synchronize()
    ref = R.conv_ref(sig, srcs, weight, bias, addend, actout, pool_actout)
    rep = {"key": key, "choice": list(choice), "kernel": buf.value.decode(), "dtype": str(dt).replace("torch.", ""), "parts": {}}
    if out is not None:
        rep["parts"]["out"] = R.compare(out, ref["ref"], ref["mag"], out_dt, MAG_COEF)
        rep["parts"]["out"]["out_dtype"] = str(out_dt).replace("torch.", "")
    if pool_out is not None:
        rep["parts"]["pool"] = R.compare(pool_out, ref["pool_ref"], ref["pool_mag"], dt, MAG_COEF)
        rep["parts"]["pool"]["out_dtype"] = rep["dtype"]
    rep["ws_nonzero"] = 0 if ws is None else int((ws != 0).sum())
    rep["counters_nonzero"] = 0 if ws is None else int((ws[-4096:] != 0).sum())
    return rep


@pytest.mark.parametrize("key,choice", ENTRIES, ids=[_short(k) for k, _ in ENTRIES])
def test_cache_choice_vs_float64_reference(key, choice):
    rep = run_entry(key, choice)
    dt = R.DTYPE_CODE[R.parse_signature(key)["dtype"]]
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(rep) + "\n")
    assert rep["parts"], key
    for part, r in rep["parts"].items():
        assert r["mapped"] > 0, (part, key)
        assert r["bad"] == 0, (part, rep["kernel"], choice, r, key)
        assert r["unmapped_written"] == 0, (part, rep["kernel"], choice, "writes outside the mapped elements", r, key)
        assert r["maxnorm_rel"] <= TOL[dt], (part, rep["kernel"], choice, r, key)
    assert rep["ws_nonzero"] == 0 and rep["counters_nonzero"] == 0, ("split-K workspace / tile counters not returned to zero", rep, key)


@pytest.mark.parametrize("variant", [1, 19])
def test_comparator_catches_a_dropped_k_slice(variant):
    """The bound can fail: the first split-K gather entry and the first variant-19 entry of the cache with one 32-channel K slice of the
    weight zeroed for the kernel only -- the comparison must report violations."""
    key, choice = next((k, c) for k, c in ENTRIES if c[0] == variant and c[1] > 1 and not k.endswith("|up2"))
    rep = run_entry(key, choice, zero_k_slice=1)
    assert rep["parts"]["out"]["bad"] > 0, rep
    assert rep["ws_nonzero"] == 0 and rep["counters_nonzero"] == 0, rep
