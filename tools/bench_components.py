#!/usr/bin/env python3
"""Time of the connected components of a disparity map (csrc/components.hip: falnet_components, four launches and the clearing of info):
(a) at 375 x 1242 on the disparity of a forward on seeded structured stereo (fal_net_amd/synthetic.py) and on the `spiral`, `checker` and `percolation`
    families of tests/_components_ref.py, with and without the label output, by HIP events around single calls into preallocated buffers;
(b) with B = 1 and B = 8 at 256 x 512 (`percolation`, one seed per image);
(c) next to the byte floor -- the map read once, two int32 maps written -- at 8 TB/s;
(d) where scipy is installed, next to scipy.ndimage.label on the host, the copies of the map down and of the labels up included, on the families whose
    edges depend on validity alone (wall clock).
Sizes and info are checked against the numpy definition before anything is timed (the small families; the 375 x 1242 maps against scipy's partition
where it applies).  Nothing on the parent commit labels components, so there is no ratio to hold: the figures are recorded.
usage: python tools/bench_components.py [--out profiles/components_timing.txt]     (on an MI355X)
       python tools/bench_components.py --resource-usage [--out ...]                 (anywhere with hipcc: appends what the compiler reports per kernel)"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, REPS, WARM, HOST_REPS = 375, 1242, 100, 10, 3
HBM = 8e12  # bytes per second
MAX_JUMP = 0.05


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:9.4f}   min {ms[0]:9.4f}   max {ms[-1]:9.4f}"


def resource_usage():
    """What -Rpass-analysis=kernel-resource-usage says of every kernel of components.hip, with the build's flags."""
    from fal_net_amd import _build
    cmd = [_build.HIPCC] + _build.FLAGS + _build.FILE_FLAGS.get("components.hip", []) + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c",
                                                                                         os.path.join(_build.CSRC, "components.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    lines, name = ["--- hipcc -Rpass-analysis=kernel-resource-usage, csrc/components.hip (gfx950, -O3)"], None
    row = {}
    for ln in text.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name, row = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ", ""), {}
        else:
            row[m.group(1).split(" ")[0]] = m.group(2)
        if name and len(row) == 5:
            lines.append(f"{name:22s} VGPRs {row['VGPRs']:>3s}  SGPRs {row['TotalSGPRs']:>3s}  LDS {row['LDS']:>5s} B  scratch {row['ScratchSize']} B/lane  occupancy {row['Occupancy']} waves/SIMD")
            name = None
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_timing.txt"))
    ap.add_argument("--resource-usage", action="store_true", help="append the compiler's per-kernel report to --out and stop (needs no GPU)")
    a = ap.parse_args()
    if a.resource_usage:
        text = "\n".join(resource_usage()) + "\n"
        print(text, end="")
        with open(a.out, "a") as f:
            f.write(text)
        return
    import numpy as np
    import torch
    import _components_ref as R
    from fal_net_amd import _lib as L
    from fal_net_amd import components, synthetic
    from fal_net_amd.models import FAL_netB
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = L.lib()
    dev = torch.device("cuda", 0)
    st_ptr = L.stream_ptr()

    # the check, before any timing: the device against the definition on every family at a size the host labels quickly
    for name in R.FAMILIES:
        f = R.family(name, 75, 250)
        kw = {k: (torch.from_numpy(np.array(v)).to(dev) if k == "score" else v) for k, v in f["kw"].items()}
        labels, sizes, info = components.label(torch.from_numpy(np.array(f["map"])).to(dev), **kw)
        want = R.reference(name, 75, 250)
        assert info == [want[2]] and np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(sizes.cpu().numpy(), want[1]), name + ": nothing timed"

    model = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(49)}, no_levels=49, compute_dtype=torch.float32).to(dev).eval()
    left, _, mn, mx = synthetic.structured_stereo(1, H, W, seed=7)[:4]
    with torch.no_grad():
        disp = model(left.to(dev), mn.to(dev), mx.to(dev), ret_disp=True, ret_subocc=False, ret_pan=False)
    maps = {"synthetic frame": disp[0, 0].float().contiguous()}
    for name in ("spiral", "checker", "percolation"):
        maps[name] = torch.from_numpy(np.array(R.family(name, H, W)["map"])).to(dev)
    batch = {B: torch.stack([torch.from_numpy(np.array(R.family("percolation", 256, 512 + b)["map"][:, :512])).to(dev) for b in range(B)]) for B in (1, 8)}

    def prepare(m):
        B = 1 if m.dim() == 2 else m.shape[0]
        h, w = m.shape[-2:]
        return dict(m=m, B=B, H=h, W=w, label=torch.empty(B * h * w, dtype=torch.int32, device=dev), size=torch.empty(B * h * w, dtype=torch.int32, device=dev),
                    info=torch.empty(3 * B + 1, dtype=torch.int64, device=dev),
                    ws=torch.empty(int(lib.falnet_components_workspace_bytes(B, h, w)) // 8, dtype=torch.int64, device=dev))

    def call(c, with_labels=True):
        L.check(lib.falnet_components(L.ptr(c["m"]), None, 0.0, 0.0, float("inf"), 1.0 + MAX_JUMP, c["B"], c["H"], c["W"], L.ptr(c["label"]) if with_labels else None,
                                      L.ptr(c["size"]), L.ptr(c["info"]), L.ptr(c["ws"]), st_ptr), "components")

    cands = {}
    for name, m in maps.items():
        cands[f"{H} x {W} {name}"] = (prepare(m), True)
        cands[f"{H} x {W} {name}, sizes only"] = (cands[f"{H} x {W} {name}"][0], False)
    for B, m in batch.items():
        cands[f"256 x 512 percolation, B = {B}"] = (prepare(m), True)
    facts = {}
    for k, (c, wl) in cands.items():
        call(c, wl)
        words = c["info"].cpu().tolist()
        assert words[-1] == 0, k
        facts[k] = words[:-1]
    if ndimage is not None:  # the full-size maps whose edges depend on validity alone: scipy's partition
        for name in ("spiral", "percolation"):
            c = cands[f"{H} x {W} {name}"][0]
            call(c)
            valid = np.isfinite(maps[name].cpu().numpy())
            theirs, n = ndimage.label(valid)
            first = np.full(n + 1, H * W, np.int64)
            np.minimum.at(first, theirs.reshape(-1), np.arange(H * W))
            assert np.array_equal(np.where(valid, first[theirs], -1).reshape(-1), c["label"].cpu().numpy()), name + ": differs from scipy's partition"
    for r in range(WARM):
        for c, wl in cands.values():
            call(c, wl)
    torch.cuda.synchronize()
    ev = {k: [] for k in cands}
    for r in range(REPS):
        for k, (c, wl) in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(c, wl)
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
    lines = [f"falnet_components, max_jump {MAX_JUMP}, every positive value valid; milliseconds per call (the clearing of info, then tile, border merge, flatten + count, sizes)",
             f"device: {torch.cuda.get_device_name(0)}; HIP events around single calls, {REPS} rounds after {WARM} warm-up rounds, the candidates alternating inside a round; "
             f"host figures over {HOST_REPS} calls after one",
             "checked before timing: labels, sizes and info == tests/_components_ref.py on every family at 75 x 250; the 375 x 1242 spiral and percolation labels == "
             + ("scipy.ndimage.label's partition" if ndimage is not None else "(scipy is not installed: not checked at full size)"),
             "synthetic frame: the f32 disparity of FAL_netB (seeded weights, 49 planes) on structured stereo, seed 7"]
    for k, (c, wl) in cands.items():
        n = c["B"] * c["H"] * c["W"]
        floor = (4 * n + 4 * n * (2 if wl else 1)) / HBM * 1e3
        med = sorted(ms[k])[len(ms[k]) // 2]
        info = facts[k]
        lines.append(f"{k:48s} {stats(ms[k])}   floor {floor:.5f} ms at 8 TB/s, the call takes {med / floor:6.1f} x that   components/valid/largest {info[:3]}")
    if ndimage is not None:
        for name in ("spiral", "percolation"):
            m = maps[name]

            def host():
                valid = np.isfinite(m.cpu().numpy())
                lab, _ = ndimage.label(valid)
                return torch.from_numpy(lab).to(dev)

            host()
            out = []
            for _ in range(HOST_REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            lines.append(f"{'host: scipy.ndimage.label, ' + name + ', copies included':48s} {stats(out)}   (labels only: no smallest index, no sizes)")
    else:
        lines.append("scipy is not installed: no host figure")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
