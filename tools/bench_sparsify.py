#!/usr/bin/env python3
"""Time of one frame's sparsification curves at 375 x 1242 with four scores and S = 50 (kitti2015 mode, about 30 % of the ground truth valid):
(a) the sort alone (falnet_sort_u32): 7 segments of the frame's n keys, and 7 segments of H W keys -- what falnet_sparsify sorts, because n stays
    on the device -- next to its byte floor, 4 passes x (8 B read + 8 B written) per element and segment, at 8 TB/s;
(b) the whole falnet_sparsify call (compaction, keys, sort, interval sums, curves);
(c) on the host, copies of the six maps included: the numpy definition (tests/_sparsify_ref.py, math.fsum) and the same orderings with np.cumsum
    in the place of fsum (what a user would write; not exactly rounded).
(a) and (b) by HIP events around single calls into preallocated buffers, REPS repetitions with the three candidates ALTERNATING call by call and
two frames alternating beneath them, after WARM warm-up rounds; (c) by wall clock on the same box.  The device row is checked against the
definition before anything is timed.  Nothing on the parent commit does this job, so there is no ratio to hold: the figures are recorded.
usage: python tools/bench_sparsify.py [--out profiles/sparsify_timing.txt]  (on an MI355X)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _sparsify_ref as SR  # noqa: E402
from fal_net_amd import _lib as L  # noqa: E402
from fal_net_amd import metrics as M  # noqa: E402
from fal_net_amd import sparsification as SP  # noqa: E402

H, W, S, REPS, WARM, HOST_REPS = 375, 1242, 50, 100, 10, 2
HBM = 8e12  # bytes per second
MODE = "kitti2015"


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:9.4f}   min {ms[0]:9.4f}   max {ms[-1]:9.4f}"


def seeded_frame(seed):
    rng = np.random.default_rng(seed)
    pred = (rng.random((H, W)) ** 2 * 87 + 0.5).astype(np.float32)
    noise = 0.15 * rng.standard_normal((H, W))
    gt = np.maximum(pred.astype(np.float64) * (1 + noise), 0.05).astype(np.float32)
    gt[rng.random((H, W)) >= 0.3] = 0
    maps = [(np.abs(noise) + 0.05 * rng.standard_normal((H, W))).astype(np.float32), rng.random((H, W), dtype=np.float32),
            (np.abs(noise) * pred).astype(np.float32), (1 / (1 + 8 * np.abs(noise))).astype(np.float32)]
    return pred, gt, list(zip(maps, (1, 1, 1, -1)))


def cumsum_curves(mode, pred, gt, scores, steps):
    """The same orderings and cuts with np.cumsum over the reversed order in the place of the exactly rounded sums."""
    g, p, idx = SR.pairs(mode, pred, gt)
    e_abs, e_sq, t = SR.errors(g, p)
    lt = (t < 1.25).astype(np.float64)
    n = len(g)
    r = np.array(SR.cut_ranks(n, steps))
    row = [float(n)]
    for perm, which in [(SR.order(x), (0, 1, 2)) for x in SR.score_values(scores, idx)] + [(SR.order(x.astype(np.float32)), (k,)) for k, x in enumerate((e_abs, e_sq, t))]:
        for k in which:
            suffix = np.cumsum((e_abs, e_sq, lt)[k][perm][::-1])[::-1]
            v = suffix[r] / (n - r)
            row += (v if k == 0 else (np.sqrt(v) if k == 1 else 1 - v)).tolist()
    return np.array(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparsify_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lib, st = L.lib(), L.stream_ptr()
    frames = [seeded_frame(s) for s in (11, 12)]
    dev = [(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), [(torch.from_numpy(m).cuda(), s) for m, s in sc]) for p, g, sc in frames]
    fb = float(M.focal_baseline(MODE, W))
    # check before timing: n and d1 exactly, the sums within the derived bound
    ns = []
    for (p, g, sc), (pt, gt, sct) in zip(frames, dev):
        want = SR.sparsify_ref(MODE, p, g, sc, steps=S)
        got = SP.curves(pt, gt, MODE, {str(i): ms for i, ms in enumerate(sct)}, steps=S).cpu().numpy()
        body_g, body_w = got[1:].reshape(5, 3, S), want[1:].reshape(5, 3, S)
        ok = got[0] == want[0] and np.array_equal(body_g[:, 2], body_w[:, 2]) and (np.abs(body_g[:, :2] - body_w[:, :2]) <= SR.curve_bound(want[0], S, body_w[:, :2])).all()
        assert ok, "the device row differs from the definition: nothing timed"
        ns.append(int(want[0]))
    n, N, seg = ns[0], H * W, 7
    lines = [f"{H} x {W} seeded frames ({MODE}, n = {ns[0]} and {ns[1]} counted pixels of {N}), four scores, S = {S}; milliseconds",
             f"device: {torch.cuda.get_device_name(0)}; device figures by HIP events over {REPS} calls of each candidate, the candidates alternating call by call and two "
             f"frames alternating beneath them, after {WARM} warm-up rounds; host figures by wall clock over {HOST_REPS} calls after one",
             "checked: n and every d1 value equal the definition's, abs_rel and rms within (n_j + 2) 2^-53 of it"]
    rng = np.random.default_rng(5)
    keys = {m: [torch.from_numpy(rng.integers(0, 1 << 32, (seg, m), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda() for _ in range(2)] for m in (n, N)}
    perm = {m: torch.empty((seg, m), dtype=torch.int32, device="cuda") for m in (n, N)}
    sort_ws = torch.empty(int(lib.falnet_sort_u32_workspace_bytes(N, seg)) // 8, dtype=torch.int64, device="cuda")
    sp_ws = torch.empty(int(lib.falnet_sparsify_workspace_bytes(H, W, 4)) // 8, dtype=torch.int64, device="cuda")
    rows = [torch.empty(SP.row_length(4, S), dtype=torch.float64, device="cuda") for _ in dev]
    structs = []
    for _, _, sct in dev:
        sc = L.Scores()
        sc.n = 4
        for i, (m, s) in enumerate(sct):
            sc.map[i], sc.sign[i] = m.data_ptr(), s
        structs.append(sc)

    def sort(m, f):
        L.check(lib.falnet_sort_u32(L.ptr(keys[m][f]), m, seg, L.ptr(perm[m]), L.ptr(sort_ws), st), "sort_u32")

    def sparsify(f):
        pt, gt, _ = dev[f]
        L.check(lib.falnet_sparsify(L.ptr(pt), L.ptr(gt), H, W, M.MODES[MODE], fb, None, 1.0, 80.0, structs[f], S, L.ptr(rows[f]), L.ptr(sp_ws), st), "sparsify")

    cands = {"sort_n": lambda f: sort(n, f), "sort_N": lambda f: sort(N, f), "sparsify": sparsify}
    for i in range(WARM):
        for fn in cands.values():
            fn(i % 2)
    torch.cuda.synchronize()
    ev = {k: [] for k in cands}
    for i in range(REPS):
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(i % 2)
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    for k, m, what in (("sort_n", n, "the frame's n"), ("sort_N", N, "H W, as inside falnet_sparsify")):
        floor = 4 * 16 * m * seg
        lines.append(f"{'falnet_sort_u32, 7 segments of ' + str(m) + ' random keys (' + what + '), 12 launches':92s} {stats(ms[k])}")
        lines.append(f"{'  byte floor: 4 passes x (8 B read + 8 B written) per element and segment':92s} {floor / 1e6:9.3f} MB -> {floor / HBM * 1e3:9.5f} ms at 8 TB/s; "
                     f"the sort takes {med[k] / (floor / HBM * 1e3):6.1f} x that")
    lines.append(f"{'falnet_sparsify, the whole call (one memset, 17 launches)':92s} {stats(ms['sparsify'])}")

    def wall(fn, reps):
        fn()
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def host(curves):
        pt, gt, sct = dev[0]
        torch.cuda.synchronize()
        p, g = pt.cpu().numpy(), gt.cpu().numpy()
        return curves(MODE, p, g, [(m.cpu().numpy(), s) for m, s in sct], steps=S)

    assert np.allclose(host(cumsum_curves), host(SR.sparsify_ref), rtol=1e-9, atol=0)
    lines.append(f"{'host: six copies + argsort + np.cumsum (not exactly rounded), wall':92s} {stats(wall(lambda: host(cumsum_curves), HOST_REPS))}")
    lines.append(f"{'host: six copies + the definition (tests/_sparsify_ref.py: argsort + math.fsum per cut), wall':92s} {stats(wall(lambda: host(SR.sparsify_ref), HOST_REPS))}")
    lines.append(f"{'SP.curves (wrapper: struct, workspace of a fresh one-row table), wall, synchronised':92s} "
                 f"{stats(wall(lambda: (SP.curves(dev[0][0], dev[0][1], MODE, {str(i): ms_ for i, ms_ in enumerate(dev[0][2])}, steps=S), torch.cuda.synchronize()), HOST_REPS))}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
