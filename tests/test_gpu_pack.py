"""GPU: the five entry points of fal_net_amd/csrc/pack.hip -- falnet_pack_weights (element per thread), falnet_pack_weights_batched
(pack_tile), falnet_pack_up2_batched (sub-pixel weights), falnet_adam_pack_batched and falnet_adam_pack_batched_wd (Adam folded into the
tile pass) -- through the C ABI, against tests/_pack_ref.py.

Operands are compared BIT FOR BIT (int16 / int32 views): every operand lives between two 256-element guard zones, operand and guards are
pre-filled with a NaN sentinel (0x7fc1; 0x7fc00001 in f32), so the kernel must have written every position itself -- +0 in the padding --
and nothing beside it.  A failure names layer, operand and (row, tap, column) of the first mismatch.  The fused Adam is held per step and per
element to a float64 step from the device's own pre-step state (bounds: _pack_ref's docstring), its operands exactly to the reference of the
master the kernel left; gaps between the masters, the gradient row, the derived layer's master and the guards must not change by one bit.
Every test prints its worst ratio / its element count before it asserts (run with -s)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import _adam_decay_ref as AR  # noqa: E402
import _pack_ref as R  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import loss_functions as LF  # noqa: E402
from fal_net_amd import synthetic, train  # noqa: E402

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
GUARD = 256
SENT = {F32: 0x7fc00001, BF16: 0x7fc1, F16: 0x7fc1}
LR, BETAS, EPS = 1e-4, (0.5, 0.999), 1e-8
COUNT = {"f32": 0, "bf16": 0, "f16": 0}      # operand elements compared bit for bit
WORST = {"m": 0.0, "v": 0.0, "p": 0.0}       # worst ratios to the Adam bounds
DT_IDS = [R.DTYPE_NAME[d] for d in R.DTYPES]


@pytest.fixture(autouse=True)
def _f32_losses_afterwards():
    yield
    LF.set_compute_dtype(torch.float32)


class Guarded:
    """An operand of `shape` between two guard zones, everything pre-filled with the sentinel of its dtype."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype
        self.itype = torch.int32 if dtype == F32 else torch.int16
        self.n = 1
        for s in shape:
            self.n *= s
        self.raw = torch.full((self.n + 2 * GUARD,), SENT[dtype], dtype=self.itype, device=DEV)

    def refill(self):
        self.raw.fill_(SENT[self.dtype])

    def ptr(self):
        return self.raw.data_ptr() + GUARD * self.raw.element_size()

    def bits(self):
        return self.raw[GUARD:GUARD + self.n].cpu().view(self.shape)

    def guards_intact(self):
        r = self.raw.cpu()
        return bool((r[:GUARD] == SENT[self.dtype]).all()) and bool((r[GUARD + self.n:] == SENT[self.dtype]).all())

    def untouched(self):
        return bool((self.raw == SENT[self.dtype]).all())


def check_operand(g, ref, layer, operand):
    """The guarded operand equals `ref` as raw bits at every position (padding +0 included) and its guards kept the sentinel."""
    assert ref.dtype == g.dtype and tuple(ref.shape) == g.shape, (layer, operand, ref.shape, g.shape)
    got, want = g.bits(), R.bits_of(ref)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, t, c = (int(x) for x in bad[0])
        mask = 0xffffffff if g.dtype == F32 else 0xffff
        pytest.fail(f"layer {layer} operand {operand} ({R.DTYPE_NAME[g.dtype]}): {bad.shape[0]} of {got.numel()} positions differ, first at (row, tap, column) = "
                    f"({r}, {t}, {c}): got 0x{int(got[r, t, c]) & mask:x}, reference 0x{int(want[r, t, c]) & mask:x}")
    assert g.guards_intact(), f"layer {layer} operand {operand}: a guard zone was written"
    COUNT[R.DTYPE_NAME[g.dtype]] += got.numel()


class Entry:
    """One layer of a batched launch: its own master on the device and its own guarded operands."""

    def __init__(self, case, dtype, kind, seed=0, with_wd=True, w=None):
        self.case, self.dtype = case, dtype
        self.w_host = R.master(case, kind, dtype, seed) if w is None else w
        self.w = self.w_host.to(DEV).contiguous()
        self.wf = Guarded((case["cout_pad"], case["taps"], case["cin_pad"]), dtype)
        self.wd = Guarded((case["cin_pad"], case["taps"], case["cout_pad"]), dtype) if with_wd else None
        self.no_update = 0
        self.w_ptr = None  # (an Adam launch points the entry into the flat buffer instead)

    def check(self, what, master=None):
        wf, wd, _ = R.ref_case(self.case, self.w_host if master is None else master, self.dtype)
        check_operand(self.wf, wf, f"{what} {self.case['name']}", "wf")
        if self.wd is not None:
            check_operand(self.wd, wd, f"{what} {self.case['name']}", "wd")


def desc_table(entries):
    descs = (L.PackDesc * max(1, len(entries)))()
    blk = 0
    for d, e in zip(descs, entries):
        c = e.case
        d.w = e.w.data_ptr() if e.w_ptr is None else e.w_ptr
        d.wf, d.wd = e.wf.ptr(), (0 if e.wd is None else e.wd.ptr())
        d.cout, d.cin, d.taps, d.c0_real, d.c0_pad, d.cin_pad, d.cout_pad, d.block_begin = (
            c["cout"], c["cin"], c["taps"], c["c0_real"], c["c0_pad"], c["cin_pad"], c["cout_pad"], blk)
        d.no_update = e.no_update
        blk += R.n_blocks(c)
    return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV), blk


def last_error():
    return L.lib().falnet_last_error().decode(errors="replace")


def pack_one(case, dtype, w_dev, wf, wd, **over):
    a = dict(case, **over)
    return L.lib().falnet_pack_weights(L.ptr(w_dev), a["cout"], a["cin"], a["taps"], a["c0_real"], a["c0_pad"], a["cin_pad"], a["cout_pad"],
                                       L.C.c_void_p(wf.ptr() if wf is not None else 0), L.C.c_void_p(wd.ptr() if wd is not None else 0),
                                       L.dtype_code(dtype), L.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------ falnet_pack_weights
@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", R.LAYER_CASES, ids=[c["name"] for c in R.LAYER_CASES])
def test_pack_weights_exact(case, dtype, kind):
    e = Entry(case, dtype, kind)
    what = f"pack_weights {kind}"
    L.check(pack_one(case, dtype, e.w, e.wf, e.wd), what)
    e.check(what)
    wf, wd, _ = R.ref_case(case, e.w_host, dtype)
    e.wf.refill()
    e.wd.refill()
    L.check(pack_one(case, dtype, e.w, e.wf, None), what)  # wd = NULL: the wd buffer keeps its sentinel
    torch.cuda.synchronize()
    check_operand(e.wf, wf, f"{what} (wd = NULL) {case['name']}", "wf")
    assert e.wd.untouched()
    e.wf.refill()
    L.check(pack_one(case, dtype, e.w, None, e.wd), what)  # wf = NULL
    torch.cuda.synchronize()
    check_operand(e.wd, wd, f"{what} (wf = NULL) {case['name']}", "wd")
    assert e.wf.untouched()


@pytest.mark.parametrize("name,over,msg", [("a", {"cout_pad": 40}, "multiples of 32"), ("c", {"cin_pad": 32}, "do not fit"),
                                           ("e", {"c0_real": 49, "c0_pad": 32}, "do not fit")],
                         ids=["cout_pad_not_a_multiple_of_32", "cin_pad_total_too_small", "c0_real_above_c0_pad"])
def test_pack_weights_refusals(name, over, msg):
    case = R.BY_NAME[name]
    e = Entry(case, BF16, "normal")
    rc = pack_one(case, BF16, e.w, e.wf, e.wd, **over)
    assert rc != 0 and "pack_weights" in last_error() and msg in last_error(), (rc, last_error())
    torch.cuda.synchronize()
    assert e.wf.untouched() and e.wd.untouched()


# ------------------------------------------------------------------------------------------------------------------ falnet_pack_weights_batched
def run_batched(entries, dtype, what, n=None):
    dev, total = desc_table(entries)
    L.check(L.lib().falnet_pack_weights_batched(L.ptr(dev), len(entries) if n is None else n, total, L.dtype_code(dtype), L.stream_ptr()), what)
    torch.cuda.synchronize()
    for e in entries:
        e.check(what)


@pytest.mark.parametrize("order", ["listed", "reversed"])
@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
def test_batched_all_cases_in_one_launch(dtype, kind, order):
    """Block ranges of 9-, 3- and 1-tap layers side by side, in both orders."""
    cases = R.LAYER_CASES if order == "listed" else R.LAYER_CASES[::-1]
    run_batched([Entry(c, dtype, kind, seed=1) for c in cases], dtype, f"batched {order}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
def test_batched_full_table_of_64_entries(dtype):
    """The descriptor table at its limit: 64 entries (cases a, c, g, i, j repeated), each with its own master and operands."""
    names = "acgij"
    entries = [Entry(R.BY_NAME[names[i % 5]], dtype, "ties" if i % 2 else "normal", seed=10 + i) for i in range(64)]
    run_batched(entries, dtype, "batched n = 64")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", R.LAYER_CASES, ids=[c["name"] for c in R.LAYER_CASES])
def test_batched_single_entry(case, dtype):
    """A table of one entry, every case on its own: a defect of the tile kernel names the cases it shows in."""
    run_batched([Entry(case, dtype, "ties", seed=2)], dtype, "batched n = 1")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
def test_batched_entry_without_wd(dtype):
    """wd = 0 in the middle entry: its wf is right, and so is everything of its neighbours."""
    entries = [Entry(R.BY_NAME["e"], dtype, "ties", 3), Entry(R.BY_NAME["c"], dtype, "ties", 3, with_wd=False), Entry(R.BY_NAME["g"], dtype, "normal", 3)]
    run_batched(entries, dtype, "batched, wd = 0")


@pytest.mark.parametrize("n", [0, 65])
def test_batched_refuses_tables_beyond_its_limits(n):
    entries = [Entry(R.BY_NAME["j"], BF16, "normal", seed=i) for i in range(max(n, 1))]
    dev, total = desc_table(entries)
    lib = L.lib()
    scaler = torch.zeros(4, device=DEV)
    state = torch.tensor([LR, 0.0], device=DEV)
    up = Guarded((32, 16, 32), BF16)
    rcs = {"pack_weights_batched": lib.falnet_pack_weights_batched(L.ptr(dev), n, total, L.BF16, L.stream_ptr())}
    assert rcs["pack_weights_batched"] != 0 and "pack_weights_batched" in last_error()
    rcs["adam_pack_batched"] = lib.falnet_adam_pack_batched(L.ptr(dev), n, total, L.BF16, 1 << 20, 2 << 20, 3 << 20, L.ptr(state), BETAS[0], BETAS[1], EPS, 1.0,
                                                            L.ptr(scaler), L.stream_ptr())
    assert rcs["adam_pack_batched"] != 0 and "adam_pack_batched" in last_error()
    rcs["adam_pack_batched_wd"] = lib.falnet_adam_pack_batched_wd(L.ptr(dev), n, total, L.BF16, 1 << 20, 2 << 20, 3 << 20, L.ptr(state), BETAS[0], BETAS[1], EPS,
                                                                  1.0, 1e-2, L.ptr(scaler), L.stream_ptr())
    assert rcs["adam_pack_batched_wd"] != 0 and "adam_pack_batched_wd" in last_error()
    updev, uptotal = up2_table([(torch.zeros(1, 1, 3, 3, device=DEV), 1, 1, up, None)] * max(n, 1))
    rcs["pack_up2_batched"] = lib.falnet_pack_up2_batched(L.ptr(updev), n, uptotal, L.BF16, L.stream_ptr())
    assert rcs["pack_up2_batched"] != 0 and "pack_up2_batched" in last_error()
    torch.cuda.synchronize()
    assert all(e.wf.untouched() and e.wd.untouched() for e in entries) and up.untouched()
    assert all(torch.equal(e.w.cpu(), e.w_host) for e in entries)


# ------------------------------------------------------------------------------------------------------------------ element kernel against tile kernel
@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
def test_element_kernel_and_tile_kernel_agree_bit_for_bit(dtype):
    """Follows from both matching the reference; asserted once so that a later divergence names itself."""
    tile = [Entry(c, dtype, "ties", seed=4) for c in R.LAYER_CASES]
    dev, total = desc_table(tile)
    L.check(L.lib().falnet_pack_weights_batched(L.ptr(dev), len(tile), total, L.dtype_code(dtype), L.stream_ptr()), "batched")
    for t in tile:
        e = Entry(t.case, dtype, "ties", w=t.w_host)
        L.check(pack_one(t.case, dtype, e.w, e.wf, e.wd), "pack_weights")
        torch.cuda.synchronize()
        assert torch.equal(e.wf.raw, t.wf.raw) and torch.equal(e.wd.raw, t.wd.raw), t.case["name"]


# ------------------------------------------------------------------------------------------------------------------ falnet_pack_up2_batched
def up2_table(layers):
    """layers: (w_dev, cout, cin, wu Guarded, wdd Guarded or None)."""
    descs = (L.PackUp2Desc * len(layers))()
    blk = 0
    for d, (w, cout, cin, wu, wdd) in zip(descs, layers):
        d.w, d.wu, d.wdd = w.data_ptr(), wu.ptr(), (0 if wdd is None else wdd.ptr())
        d.cout, d.cin, d.cin_pad, d.cout_pad, d.block_begin = cout, cin, R.pad_c(cin), R.pad_c(cout), blk
        blk += (R.pad_c(cout) // 32) * (R.pad_c(cin) // 32)
    return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV), blk


def up2_master(kind, dtype, shape, seed):
    if kind == "normal":
        return R.normal(shape, seed)
    if kind == "dyadic":
        return R.dyadic(shape, seed)
    return R.fill_from(R.ties(dtype, seed, moderate=True), shape, seed)


@pytest.mark.parametrize("with_wdd", [True, False], ids=["wdd", "no_wdd"])
@pytest.mark.parametrize("kind", ["normal", "dyadic", "ties"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_pack_up2_exact(dtype, kind, with_wdd):
    """The three sub-pixel cases in one launch.  A mismatch on `dyadic` means wrong taps (its sums are exact in any order); one on `normal`
    alone another order of the f32 additions."""
    hosts, layers = [], []
    for k, (cout, cin) in enumerate(R.UP2_CASES):
        w = up2_master(kind, dtype, (cout, cin, 3, 3), 20 + k)
        hosts.append(w)
        layers.append((w.to(DEV).contiguous(), cout, cin, Guarded((R.pad_c(cout), 16, R.pad_c(cin)), dtype), Guarded((R.pad_c(cin), 4, 4 * R.pad_c(cout)), dtype)))
    dev, total = up2_table([(w, co, ci, wu, wdd if with_wdd else None) for w, co, ci, wu, wdd in layers])
    L.check(L.lib().falnet_pack_up2_batched(L.ptr(dev), len(layers), total, L.dtype_code(dtype), L.stream_ptr()), "pack_up2_batched")
    torch.cuda.synchronize()
    for w, (_, cout, cin, wu, wdd) in zip(hosts, layers):
        check_operand(wu, R.ref_wu(w, dtype), f"up2 {cout}x{cin} {kind}", "wu")
        if with_wdd:
            check_operand(wdd, R.ref_wdd(w, dtype), f"up2 {cout}x{cin} {kind}", "wdd")
        else:
            assert wdd.untouched()


def test_pack_up2_refuses_f32():
    wu = Guarded((32, 16, 32), F32)
    dev, total = up2_table([(torch.ones(32, 32, 3, 3, device=DEV), 32, 32, wu, None)])
    rc = L.lib().falnet_pack_up2_batched(L.ptr(dev), 1, total, L.F32, L.stream_ptr())
    assert rc != 0 and "16-bit" in last_error()
    torch.cuda.synchronize()
    assert wu.untouched()


# ------------------------------------------------------------------------------------------------------------------ Adam fused with the re-pack
ADAM_CASES, ADAM_GAPS, DERIVED = "acdfgij", (3, 33, 4), "e"


def adam_layout():
    """Masters at ascending offsets (each padded to 16 B like the model's flat buffer), separated by gaps of 3, 33, 4 elements (padded to
    16 B) that stand for biases.  Returns {name: (offset, numel)} and the row length."""
    spans, off = {}, 0
    for k, name in enumerate(ADAM_CASES):
        c = R.BY_NAME[name]
        n = c["cout"] * c["cin"] * c["taps"]
        spans[name] = (off, n)
        off += (n + 3) // 4 * 4 + (ADAM_GAPS[k % 3] + 3) // 4 * 4
    return spans, off


def hand_gradient(numel, step, amp=1e-3):
    """A gradient that changes in size and sign with every step (test_gpu_adam_decay.py: hand_gradient)."""
    i = torch.arange(numel, dtype=torch.float32)
    return torch.sin(i * 0.37 + 1.3 * step) * amp * (1 + step) * (-1) ** step


@pytest.mark.parametrize("rows", ["pgmv", "vmgp"])
@pytest.mark.parametrize("gs,scaler", [(1.0, None), (0.125, [4.0, 0.0, 0.0, 0.0])], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("decay", [0.0, 1e-2])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
def test_adam_pack_step_by_step(dtype, decay, gs, scaler, rows):
    lib = L.lib()
    K = 3
    spans, n_flat = adam_layout()
    row = {ch: i for i, ch in enumerate(rows)}
    sent = SENT[F32]
    raw = torch.full((4 * n_flat + 2 * GUARD,), sent, dtype=torch.int32)  # guard | 4 rows | guard, all sentinel (NaN)
    flat = raw[GUARD:GUARD + 4 * n_flat].view(4, n_flat)
    real = torch.zeros(n_flat, dtype=torch.bool)
    fview = flat.view(torch.float32)
    masters = {}
    for k, name in enumerate(ADAM_CASES):
        off, n = spans[name]
        real[off:off + n] = True
        masters[name] = R.master(R.BY_NAME[name], "normal", dtype, seed=30)
        fview[row["p"], off:off + n] = masters[name].reshape(-1)
        fview[row["m"], off:off + n] = 0.0
        fview[row["v"], off:off + n] = 0.0
        fview[row["g"], off:off + n] = 0.0
    dev_raw = raw.to(DEV)
    base = dev_raw.data_ptr() + 4 * (GUARD + row["p"] * n_flat)
    g_off, m_off, v_off = ((row[ch] - row["p"]) * n_flat for ch in "gmv")
    entries = []
    for name in ADAM_CASES:
        e = Entry(R.BY_NAME[name], dtype, "normal", w=masters[name])
        e.w_ptr = base + 4 * spans[name][0]
        entries.append(e)
    derived = Entry(R.BY_NAME[DERIVED], dtype, "ties", seed=31)  # its master lies outside the flat tensor
    derived.no_update = 1
    entries.insert(3, derived)
    table, total = desc_table(entries)
    sc = None if scaler is None else torch.tensor(scaler, device=DEV)
    named = {f"{n}.weight": masters[n] for n in ADAM_CASES}
    ref = AR.RefAdam64(named, LR, BETAS, EPS, weight_decay=decay)
    ref0 = AR.RefAdam64(named, LR, BETAS, EPS)
    gs_eff = R.f32c(gs) / (scaler[0] if scaler else 1.0)

    def launch(state):
        if decay:
            L.check(lib.falnet_adam_pack_batched_wd(L.ptr(table), len(entries), total, L.dtype_code(dtype), g_off, m_off, v_off, L.ptr(state), BETAS[0], BETAS[1],
                                                    EPS, gs, decay, L.ptr(sc), L.stream_ptr()), "adam_pack_batched_wd")
        else:
            L.check(lib.falnet_adam_pack_batched(L.ptr(table), len(entries), total, L.dtype_code(dtype), g_off, m_off, v_off, L.ptr(state), BETAS[0], BETAS[1],
                                                 EPS, gs, L.ptr(sc), L.stream_ptr()), "adam_pack_batched")
        torch.cuda.synchronize()

    def rows_of(r):
        return r[GUARD:GUARD + 4 * n_flat].view(4, n_flat)

    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    what = f"adam-pack {R.DTYPE_NAME[dtype]} decay={decay} gs={gs} scaler={scaler is not None} rows={rows}"
    for k in range(K):
        g = hand_gradient(n_flat, k)
        grow = torch.full((n_flat,), sent, dtype=torch.int32)
        grow[real] = g.view(torch.int32)[real]
        dev_raw[GUARD + row["g"] * n_flat:GUARD + (row["g"] + 1) * n_flat] = grow.to(DEV)
        for e in entries:
            e.wf.refill()
            e.wd.refill()
        state = torch.tensor([LR, float(k)], device=DEV)
        before = dev_raw.cpu()
        launch(state)
        after = dev_raw.cpu()
        b, a = rows_of(before), rows_of(after)
        bf, af = b.view(torch.float32), a.view(torch.float32)
        # 5. nothing between or beside the masters changed: gaps of p, m, v; the whole gradient row; the guards; the derived layer's master
        for ch in "pmv":
            assert torch.equal(a[row[ch]][~real], b[row[ch]][~real]), f"{what} step {k + 1}: a gap of row {ch} was written"
        assert torch.equal(a[row["g"]], b[row["g"]]), f"{what} step {k + 1}: the gradient row was written"
        assert torch.equal(after[:GUARD], before[:GUARD]) and torch.equal(after[GUARD + 4 * n_flat:], before[GUARD + 4 * n_flat:])
        assert torch.equal(derived.w.cpu(), derived.w_host)
        assert float(state[1]) == k  # (t is advanced by falnet_adam_tick, not here)
        got_all, nodecay_all = [], []
        for e in entries:
            name = e.case["name"]
            if e.no_update:
                e.check(f"{what} step {k + 1} (no_update)")
                continue
            off, n = spans[name]
            sl = slice(off, off + n)
            pre = [bf[row[ch], sl] for ch in "pgmv"]
            kw = dict(steps=k, lr=LR, betas=BETAS, eps=EPS, grad_scale=gs, scaler=scaler)
            # 1. p, m, v of every real element against one float64 step from the device's own pre-step state
            r = R.adam_ratios(af[row["p"], sl], af[row["m"], sl], af[row["v"], sl], R.ref_adam_step(*pre, decay=decay, **kw), LR)
            for key in worst:
                worst[key] = max(worst[key], r[key])
            assert r["m"] <= 1.0 and r["v"] <= 1.0 and r["p"] <= 1.0, (what, k + 1, name, r)
            if decay:
                got_all.append(af[row["p"], sl])
                nodecay_all.append(R.ref_adam_step(*pre, decay=0.0, **kw)[0])
            # 4. the operands are the reference of the master as the kernel left it, bit for bit
            e.check(f"{what} step {k + 1}", master=af[row["p"], sl].reshape(e.w_host.shape))
        if decay:  # 2. the decay is seen
            AR.check_decay_seen(torch.cat(got_all), torch.cat(nodecay_all), 1, LR, f"{what} step {k + 1}")
        grads = {f"{n}.weight": g[spans[n][0]:spans[n][0] + spans[n][1]] for n in ADAM_CASES}
        ref.step(grads, gs_eff)
        ref0.step(grads, gs_eff)
    print(f"{what}: worst ratio to the bound over {K} steps: m {worst['m']:.3f}  v {worst['v']:.3f}  p {worst['p']:.3f}")
    for key in WORST:
        WORST[key] = max(WORST[key], worst[key])
    # 3. over the three steps together, against the reference the other optimiser paths answer to
    final = rows_of(dev_raw.cpu()).view(torch.float32)
    for n in ADAM_CASES:
        off, cnt = spans[n]
        AR.check(final[row["p"], off:off + cnt], ref.p[f"{n}.weight"].detach().reshape(-1), K, LR, f"{what} {n}")
    if decay:
        AR.check_decay_seen(torch.cat([final[row["p"], spans[n][0]:spans[n][0] + spans[n][1]] for n in ADAM_CASES]),
                            torch.cat([ref0.p[f"{n}.weight"].detach().reshape(-1) for n in ADAM_CASES]), K, LR, f"{what} {K} steps")
    # 6. a raised overflow flag: one more launch changes nothing at all
    if sc is not None:
        sc[2] = 1.0
        snap = [dev_raw.clone()] + [t.raw.clone() for e in entries for t in (e.wf, e.wd)]
        launch(torch.tensor([LR, float(K)], device=DEV))
        for s, t in zip(snap, [dev_raw] + [t.raw for e in entries for t in (e.wf, e.wd)]):
            assert torch.equal(s, t), f"{what}: a skipped step wrote something"


# The pairs of (a) pack-fused, (b) range and (c) flat kernel that give an element the same bits, by bool(decay): measured, not designed.  The
# kernels share one update (csrc/adam.h), but the compiler fuses multiplies into adds per kernel: the decayed range and flat kernels come
# out alike, every other pair differs in the last place of v (and of a few p) -- figures in the test's docstring.
PATHS_THAT_AGREE = {True: ("bc",), False: ()}


@pytest.mark.parametrize("t0", [0, 6])
@pytest.mark.parametrize("gs,scaler", [(1.0, None), (0.125, [4.0, 0.0, 0.0, 0.0])], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("decay", [0.0, 1e-2])
def test_adam_paths_agree_bit_for_bit(decay, gs, scaler, t0):
    """One FlatAdam.step() sends a weight through the pack-fused kernel, a bias through the range kernel and, without a plan or under stream
    capture, the same parameters through the flat kernel: an element must get the same bits whichever path updates it (csrc/adam.h holds the
    one update they all call).  Three copies of one (p, g, m, v) buffer -- the masters of adam_layout(), zeros in the gaps because the flat
    kernel walks them -- take two consecutive steps each, (a) falnet_adam_pack_batched[_wd], (b) falnet_adam_ranges[_wd] with one range per
    master, (c) falnet_adam_step_dev / _guarded / _wd over the whole row; p, m and v are compared as int32.  falnet_adam_step is no part of
    it: it forms its coefficients on the host in double.
    Measured on MI355X, the same before and after the update moved into adam.h (94 402 elements, two steps): decayed, (b) and (c) agree in
    every bit, (a) differs from both in v on 12 448 .. 38 280 elements by <= 3 ulp, in p on <= 30 by <= 32 ulp (values near 0), in m on <= 1
    by 1 ulp; undecayed, every pair differs: v on 5 .. 38 382 elements by <= 3 ulp, p on <= 50 by <= 2 ulp, m nowhere.  So only (b) == (c)
    of the decayed form is asserted (PATHS_THAT_AGREE); every figure is printed (run with -s)."""
    lib = L.lib()
    K = 2
    spans, n_flat = adam_layout()
    host = torch.zeros(4, n_flat)  # rows p, g, m, v
    real = torch.zeros(n_flat, dtype=torch.bool)
    masters = {}
    for name in ADAM_CASES:
        off, n = spans[name]
        real[off:off + n] = True
        masters[name] = R.master(R.BY_NAME[name], "normal", BF16, seed=30)
        host[0, off:off + n] = masters[name].reshape(-1)
    if t0:  # moments as a run that is t0 steps old would hold them
        host[2][real] = 0.5 * hand_gradient(n_flat, 7)[real]
        host[3][real] = hand_gradient(n_flat, 8)[real] ** 2
    bufs = {k: host.to(DEV) for k in "abc"}
    states = {k: torch.tensor([LR, float(t0)], device=DEV) for k in "abc"}
    sc = None if scaler is None else torch.tensor(scaler, device=DEV)
    g_off, m_off, v_off = n_flat, 2 * n_flat, 3 * n_flat
    entries = []
    for name in ADAM_CASES:
        e = Entry(R.BY_NAME[name], BF16, "normal", w=masters[name])
        e.w_ptr = bufs["a"].data_ptr() + 4 * spans[name][0]
        entries.append(e)
    table, total = desc_table(entries)
    ranges = torch.tensor([x for name in ADAM_CASES for x in spans[name]], dtype=torch.int64, device=DEV)
    decays = torch.full((len(ADAM_CASES),), decay, dtype=torch.float64, device=DEV)
    seg_end = torch.tensor([n_flat], dtype=torch.int64, device=DEV)
    hyper = (BETAS[0], BETAS[1], EPS, gs)
    st = L.stream_ptr()
    for k in range(K):
        g = torch.where(real, hand_gradient(n_flat, k), torch.zeros(n_flat)).to(DEV)
        for b in bufs.values():
            b[1].copy_(g)
        a, r, c = bufs["a"], bufs["b"], bufs["c"]
        if decay:
            L.check(lib.falnet_adam_pack_batched_wd(L.ptr(table), len(entries), total, L.BF16, g_off, m_off, v_off, L.ptr(states["a"]), *hyper, decay,
                                                    L.ptr(sc), st), "adam_pack_batched_wd")
            L.check(lib.falnet_adam_ranges_wd(L.ptr(r), g_off, m_off, v_off, L.ptr(ranges), L.ptr(decays), len(ADAM_CASES), L.ptr(states["b"]), *hyper,
                                              L.ptr(sc), st), "adam_ranges_wd")
            L.check(lib.falnet_adam_step_wd(L.ptr(c[0]), L.ptr(c[1]), L.ptr(c[2]), L.ptr(c[3]), n_flat, L.ptr(seg_end), L.ptr(decays), 1,
                                            L.ptr(states["c"]), *hyper, L.ptr(sc), st), "adam_step_wd")
        else:
            L.check(lib.falnet_adam_pack_batched(L.ptr(table), len(entries), total, L.BF16, g_off, m_off, v_off, L.ptr(states["a"]), *hyper, L.ptr(sc), st),
                    "adam_pack_batched")
            L.check(lib.falnet_adam_ranges(L.ptr(r), g_off, m_off, v_off, L.ptr(ranges), len(ADAM_CASES), L.ptr(states["b"]), *hyper, L.ptr(sc), st),
                    "adam_ranges")
            if sc is None:
                L.check(lib.falnet_adam_step_dev(L.ptr(c[0]), L.ptr(c[1]), L.ptr(c[2]), L.ptr(c[3]), n_flat, L.ptr(states["c"]), *hyper, st), "adam_step_dev")
            else:
                L.check(lib.falnet_adam_step_guarded(L.ptr(c[0]), L.ptr(c[1]), L.ptr(c[2]), L.ptr(c[3]), n_flat, L.ptr(states["c"]), *hyper, L.ptr(sc), st),
                        "adam_step_guarded")
        for k2 in "ab":  # (step_dev / _guarded / _wd tick their state themselves)
            L.check(lib.falnet_adam_tick(L.ptr(states[k2]), L.ptr(sc), st), "adam_tick")
    torch.cuda.synchronize()
    got = {k: b.cpu().view(torch.int32) for k, b in bufs.items()}
    what = f"adam paths decay={decay} gs={gs} scaler={scaler is not None} t0={t0}"

    def ordered(bits):  # int32 view -> integers in the order of the floats: a difference of two is a distance in ulps
        b = bits.to(torch.int64)
        return torch.where(b < 0, -(b & 0x7fffffff), b)

    differ = {}
    for x, y in ("ab", "ac", "bc"):
        for i, ch in ((0, "p"), (2, "m"), (3, "v")):
            d = (ordered(got[x][i][real]) - ordered(got[y][i][real])).abs()
            differ[f"{x}{y} {ch}"] = (int((d != 0).sum()), int(d.max()))
    print(f"{what}: {int(real.sum())} elements, {K} steps; (elements that differ, most ulps) between (a) pack, (b) ranges, (c) flat: {differ}")
    assert all(float(s[1]) == t0 + K for s in states.values()), states
    assert not torch.equal(got["a"][0][real], host[0].view(torch.int32)[real])  # (the steps moved the weights)
    for pair in (PATHS_THAT_AGREE[bool(decay)]):
        assert not any(n for key, (n, _) in differ.items() if key.startswith(pair)), (what, pair, differ)
    for i, ch in ((0, "p"), (2, "m"), (3, "v")):
        assert not got["c"][i][~real].any(), f"{what}: the flat kernel left a gap of row {ch} other than +0"


# ------------------------------------------------------------------------------------------------------------------ the model's own tables
def check_model_operands(m, what):
    seen = {"wf": 0, "wu": 0, "wdd": 0, "taps": set()}
    for key, pc in m._packed.items():
        if pc.wf is None:
            continue  # (a factor of the composed logits layer: never packed)
        w = pc.weight.detach().float().cpu().contiguous()
        c0_real, c0_pad = pc.group_channels()
        wf, wd, _ = R.ref_wf_wd(w, c0_real, c0_pad, pc.cin_pad, pc.cout_pad, BF16)
        refs = {"wf": wf, "wd": wd}
        if pc.wu is not None:
            refs["wu"] = R.ref_wu(w, BF16, pc.cin_pad, pc.cout_pad)
        if pc.wdd is not None:
            refs["wdd"] = R.ref_wdd(w, BF16, pc.cin_pad, pc.cout_pad)
        for name, r in refs.items():
            got = getattr(pc, name)
            assert got.dtype == BF16 and got.shape == r.shape, (what, key, name)
            gb, rb = R.bits_of(got.cpu()), R.bits_of(r)
            if not torch.equal(gb, rb):
                bad = (gb != rb).nonzero()
                pytest.fail(f"{what}: layer {key} operand {name}: {bad.shape[0]} positions differ, first at (row, tap, column) = {tuple(int(x) for x in bad[0])}")
            COUNT["bf16"] += gb.numel()
            seen[name if name != "wd" else "wf"] += 1
        seen["taps"].add(pc.taps)
    return seen


@pytest.mark.parametrize("arch", ["B", "A"])
def test_model_descriptor_tables(arch):
    """FAL_netB / FAL_netA, N = 7, 1 x 64 x 128, bf16: every PackedConv after the plan's first pack (ops.pack_all_call / pack_up2_call) and
    after one FlatAdam.step (ops.adam_pack_call with the composed logits layer as its derived entry)."""
    from fal_net_amd import models as M
    LF.set_compute_dtype(BF16)
    sd = synthetic.seeded_falnetb_state_dict(7) if arch == "B" else synthetic.seeded_state_dict("A", 7)
    m = getattr(M, "FAL_net" + arch)({"state_dict": sd}, no_levels=7, compute_dtype=BF16).to(DEV).train()
    opt = train.FlatAdam(m, LR, BETAS, EPS)
    left, right, mn, mx = synthetic.synthetic_pair(1, 64, 128, seed=9)
    train.stage1_step(m, opt, left.to(DEV), right.to(DEV), mx.to(DEV), optimize=False)  # builds the plan: packs from the masters
    assert m._plans and train._ADAM_PACK
    torch.cuda.synchronize()
    seen = check_model_operands(m, f"FAL_net{arch} first pack")
    assert seen["wf"] >= 30 and seen["wu"] >= 1 and seen["wdd"] >= 1, seen
    assert "logits" in m._packed and m._packed["logits"].wf is not None  # (the composed layer: the derived entry of the Adam launch)
    assert 9 in seen["taps"] and (arch != "A" or 3 in seen["taps"]), seen["taps"]  # (FAL_netA: the 3x1 / 1x3 layers)
    before = m.flat_parameters().detach().clone()
    pad = torch.ones(before.numel(), dtype=torch.bool)
    for (n, p), off in zip(m._trainable_named(), m._offsets):
        pad[off:off + p.numel()] = False
    g = hand_gradient(before.numel(), 0).to(DEV)
    g[pad.to(DEV)] = 0  # (backward never writes the padding)
    m.flat_gradients().copy_(g)
    opt.step()
    torch.cuda.synchronize()
    assert m._packed_is_fresh() and float(opt.state[1]) == 1.0
    assert float((m.flat_parameters().detach() - before).abs().max()) > 0.5 * LR
    check_model_operands(m, f"FAL_net{arch} after FlatAdam.step")


def test_zz_report():
    """The totals of this run (the figures recorded in tests/_pack_ref.py)."""
    print(f"pack: operand elements compared bit for bit: {COUNT}; worst Adam ratios: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
