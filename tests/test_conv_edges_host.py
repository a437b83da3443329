"""CPU: the ragged-shape conv cases of tests/_conv_edge_cases.py before they reach a GPU.

  * Applicability is pinned: for every launch of the table, falnet_conv2d_kernel_name accepts exactly the variants of EXPECT (no device call) --
    a variant that starts refusing a ragged shape fails here instead of being skipped on the GPU, and every variant is reached by at least two
    16-bit launches with a partial last tile.
  * The reference is the operation: tests/_conv_ref.py:conv_ref, on the signatures and packed operands the launches get, equals the same
    operation composed from torch's own float64 ops (F.conv2d, F.interpolate, autograd) to 1e-12 of the result's scale.
  * The comparator sees what the max-norm bound misses: four faults injected into the exact result of case A all pass
    max|got - ref| / max|ref| < TOL[bf16] and all violate the element-wise bound; the correctly rounded result violates nothing."""
import ctypes as C

import pytest
import torch

from fal_net_amd import _lib as L
from fal_net_amd import ops

import _conv_edge_cases as E
import _conv_ref as R
from test_gpu_cache_choices import MAG_COEF
from test_gpu_ops import TOL

f64 = torch.float64
_FAKE = {n: 1 << 20 for n in ("src0", "src1", "weight", "out", "bias", "addend", "actout", "pool_out", "pool_actout", "weight_up2", "splitk_ws")}
_FAKE["splitk_ws_bytes"] = 32 << 20  # (aligned stand-ins: the query checks the arguments like a launch and dereferences nothing)
LAUNCHES = [(c, dt, label, sig) for c, dt in E.launches() for label, sig in E.sigs(c, dt)]
_ID = lambda c, dt, label: f"{c['name']}{label}-{str(dt).replace('torch.', '')}"  # noqa: E731


def _accepts(sig, variant, ksplit=1):
    d = R.fill_desc(L.Conv(), sig, _FAKE)
    d.variant, d.ksplit = variant, ksplit
    if variant == 19:
        d.scratch, d.scratch_bytes = 1 << 20, 32 << 20
    rc = L.lib().falnet_conv2d_kernel_name(C.byref(d), C.create_string_buffer(160), 160)
    assert rc in (0, -2), (variant, ksplit, rc, L.lib().falnet_last_error())
    return rc == 0


@pytest.mark.parametrize("case,dt,label,sig", LAUNCHES, ids=[_ID(c, dt, label) for c, dt, label, _ in LAUNCHES])
def test_applicability_is_pinned(case, dt, label, sig):
    assert E.UP2D_TAPS == ops.UP2D_TAPS
    d = R.fill_desc(L.Conv(), sig, _FAKE)
    back = R.parse_signature(ops.conv_signature(d))
    assert back == {k: sig[k] for k in back}, "the table's signature is not a launch signature"
    assert case["B"] in (1, 2, 3, 6)
    got = []
    for v in E.VARIANTS:
        ks = (E.deep_ksplits(sig) or [sig["cin_total"] // 32]) if v == 19 else [1]
        ok = [_accepts(sig, v, k) for k in ks]
        assert all(ok) or not any(ok), (v, ks, ok)
        if ok[0]:
            got.append(v)
    assert got == E.EXPECT[(case["name"] + label, E.bits(dt))], (case["name"] + label, dt)
    for v, k in E.choices(case, label, sig, dt):  # what the GPU test launches is accepted as launched (split-K factors included)
        assert _accepts(sig, v, k), (v, k)


def test_every_variant_is_reached_by_ragged_launches():
    ragged16 = {v: set() for v in E.VARIANTS}
    f32 = set()
    for c, dt, label, sig in LAUNCHES:
        for v in E.EXPECT[(c["name"] + label, E.bits(dt))]:
            if v not in E.RUN_ONLY.get(c["name"], (v,)):
                continue
            th = E.TILE_H[v]
            if dt == torch.float32:
                f32.add(v)
            elif (th is not None and sig["TH"] % th != 0) or sig["TW"] % 32 != 0:
                ragged16[v].add(c["name"] + label)  # (a case counts once, in whichever 16-bit type)
    assert all(len(s) >= 2 for s in ragged16.values()), {v: sorted(s) for v, s in ragged16.items() if len(s) < 2}
    assert set(range(1, 10)) | {11, 12} <= f32, sorted(f32)
    assert any(E.deep_ksplits(sig) == [8, 4] for _, _, _, sig in LAUNCHES)  # variant 19 at both slice widths


def _rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("case", E.CASES, ids=[c["name"] for c in E.CASES])
def test_reference_is_the_operation(case):
    dt = case["dtypes"][0]
    o = E.operands(case, dt)
    want = E.torch_ref(case, o)
    ss = E.sigs(case, dt)
    if case["op"] == "dgrad2":  # the four parity classes: each maps its own class, together the whole map once
        acc = torch.full_like(want["out"], float("nan"))
        for _, sig in ss:
            r = R.conv_ref(sig, o["srcs"], o["weight"], addend=o["addend"], actout=o["actout"])["ref"]
            m = ~torch.isnan(r)
            assert int(m.sum()) == sig["B"] * sig["TH"] * sig["TW"] * sig["Cout"] and torch.isnan(acc[m]).all()
            acc[m] = r[m]
        assert not torch.isnan(acc).any()
        assert _rel(acc, want["out"]) < 1e-12
        return
    sig = E.up2d_plain_sig(ss[0][1]) if case["op"] == "up2d" else ss[0][1]
    pa = o["actout"] if case["op"] == "up2d" else o["pool_actout"]
    res = R.conv_ref(sig, o["srcs"], o["weight"], o["bias"], o["addend"], None if case["op"] == "up2d" else o["actout"], pa)
    nreal = want["out"].shape[-1] if "out" in want else want["pool"].shape[-1]
    if "out" in want and sig["out"]:
        got = res["ref"] if case.get("planar") else res["ref"][..., :nreal]
        assert not torch.isnan(got).any()
        assert _rel(got, want["out"]) < 1e-12
        if not case.get("planar") and nreal < sig["Cout"]:  # zero weight rows: the padded channels are exact zeros (act(0) = 0)
            assert float(res["ref"][..., nreal:sig["Cout"]].abs().max()) == 0.0
    else:
        assert res["ref"] is None
    if "pool" in want:
        assert _rel(res["pool_ref"][..., :nreal], want["pool"]) < 1e-12
    assert ("pool" in want) == sig["pool"]


def _bf16_truncate(t):
    return (t.float().view(torch.int32) & -65536).view(torch.float32)


def test_comparator_sees_what_the_norm_misses():
    """Case A in bf16 (64 -> 64, bias + addend + ELU at 2 x 21 x 75): what the fault does to max|got - ref| / max|ref| and to the per-element bound
    u |ref| + MAG_COEF mag.  Every fault stays below TOL[bf16] = 3e-2 -- the bound of test_gpu_ops.py's conv tests is blind to it."""
    dt = torch.bfloat16
    case = E.BY_NAME["A"]
    sig = E.sigs(case, dt)[0][1]
    o = E.operands(case, dt)
    res = R.conv_ref(sig, o["srcs"], o["weight"], o["bias"], o["addend"])
    ref, mag = res["ref"], res["mag"]
    pre = R.conv_ref(dict(sig, act=R.ACT_NONE), o["srcs"], o["weight"], o["bias"], o["addend"], want_mag=False)["ref"]
    assert torch.equal(R.act_fwd(pre, R.ACT_ELU), ref)

    def check(got):
        rep = R.compare(got, ref, mag, dt, MAG_COEF)
        assert rep["mapped"] == ref.numel() and rep["maxnorm_rel"] < TOL[dt], rep
        return rep["bad"]

    assert check(ref.to(dt)) == 0  # round-to-nearest store of the exact value
    assert check(_bf16_truncate(ref)) > 1000  # truncating convert
    wrong_elu = torch.where(pre > 0, pre, 1.01 * torch.exp(pre) - 1)  # ELU negative branch with a 1 % error in exp
    assert check(wrong_elu.to(dt)) > 1000
    corner = ref.clone()  # the bottom-right corner element of each sample (last row, column and channel) 10 % off
    corner[:, -1, -1, -1] *= 1.1
    assert check(corner.to(dt)) == sig["B"]
    dropped = pre.clone()  # one input channel of one tap (dy, dx) = (-1, -1) dropped at the ragged bottom-right pixel
    x, w = o["srcs"][0].to(f64), o["weight"].to(f64)
    dropped[:, -1, -1, :] -= x[:, -2, -2, 5].view(-1, 1) * w[:, 0, 5].view(1, -1)
    bad = check(R.act_fwd(dropped, R.ACT_ELU).to(dt))
    assert 0 < bad <= sig["B"] * sig["Cout"]
