#!/usr/bin/env python3
"""Time of the distribution statistics (csrc/med_stats.hip): the all-six launch and the conf-only launch against falnet_med_head_fwd
disparity-only (the kernel every forward already runs over the same logits), at 375 x 1242 (N = 49, B = 1) and 256 x 512 (N = 49, B = 8), on
the same box in the same process, ALTERNATED pass by pass; and the ordered compaction (csrc/compact.hip) of a 375 x 1242 packed point cloud at
50 % kept.  HIP events around ITERS launches; the launches cycle over COPIES buffers of logits that together exceed the 256 MiB last-level
cache, so every launch reads its logits from HBM.  The HBM floor is (N + K) 4 B H W bytes (every logit read once, K planes written) over the
bandwidth of the data sheet, 8 TB/s.
usage: python tools/bench_med_stats.py [out.txt]   (on an MI355X; profiles/med_stats_timing.txt)"""
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from fal_net_amd import _lib as L  # noqa: E402

ITERS, REPS, WARM = 20, 7, 2
PEAK = 8.0e12  # bytes / s


def timed(fns):
    """{name: (median, min, max) microseconds per launch}; the named loops alternate inside every repetition."""
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def main():
    assert torch.cuda.is_available(), "needs an MI355X"
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "med_stats_timing.txt"), "w")

    def emit(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    lib, st = L.lib(), L.stream_ptr()
    emit(f"# {torch.cuda.get_device_name(0)}; microseconds per launch, median (min .. max) over {REPS} alternated passes of {ITERS} launches after {WARM} warm-up passes")
    fmt = lambda v: f"{v[0]:8.1f} ({v[1]:7.1f} ..{v[2]:8.1f})"  # noqa: E731
    for B, N, H, W in ((1, 49, 375, 1242), (8, 49, 256, 512)):
        nbytes = B * N * H * W * 4
        copies = max(2, -(-(320 << 20) // nbytes))
        g = torch.Generator(device="cuda").manual_seed(1)
        logits = [torch.randn(B, N, H, W, device="cuda", generator=g) * 2 for _ in range(copies)]
        mx = torch.full((B,), 300.0, device="cuda")
        mn = mx * 2 / 300
        o6 = torch.empty(B, 6, H, W, device="cuda")
        disp = torch.empty(B, 1, H, W, device="cuda")

        def stats(which):
            def run():
                for i in range(ITERS):
                    L.check(lib.falnet_med_stats_fwd(L.ptr(logits[i % copies]), L.ptr(mn), L.ptr(mx), which, L.ptr(o6), B, N, H, W, st))
            return run

        def head():
            for i in range(ITERS):
                L.check(lib.falnet_med_head_fwd(L.ptr(logits[i % copies]), None, L.ptr(mn), L.ptr(mx), L.ptr(disp), None, None, B, N, H, W, st))

        r = timed({"stats all six": stats(0b111111), "stats conf only": stats(0b010000), "head disparity only": head})
        emit(f"## B={B} N={N} {H}x{W}: {nbytes / 2 ** 20:.0f} MiB of logits, {copies} buffers in rotation")
        for name, k in (("stats all six", 6), ("stats conf only", 1), ("head disparity only", 1)):
            floor = (N + k) * 4 * B * H * W / PEAK * 1e6
            emit(f"{name:22s} {fmt(r[name])}   HBM floor {floor:6.1f} us ({(N + k) * 4 * B * H * W / 2 ** 20:.0f} MiB)   floor / time {floor / r[name][0]:.2f}"
                 f"   x head {r[name][0] / r['head disparity only'][0]:.2f}")
        del logits
    H, W = 375, 1242
    n = H * W
    g = torch.Generator(device="cuda").manual_seed(2)
    rec = torch.randint(0, 256, (n, 15), dtype=torch.uint8, device="cuda", generator=g)
    score = torch.rand(n, device="cuda", generator=g)
    dst = torch.empty_like(rec)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.falnet_compact_workspace_bytes(n)) // 8, dtype=torch.int64, device="cuda")

    def compact():
        for _ in range(ITERS):
            L.check(lib.falnet_compact_records(L.ptr(rec), 15, L.ptr(score), 0.5, n, L.ptr(dst), L.ptr(count), L.ptr(ws), st))

    r = timed({"compact": compact})
    emit(f"## ordered compaction of a {H}x{W} packed cloud ({n} records of 15 bytes, {int(count.item())} kept = {int(count.item()) / n:.3f}): three launches per call")
    emit(f"{'compact_records':22s} {fmt(r['compact'])}")


if __name__ == "__main__":
    main()
