#!/usr/bin/env python3
"""Time of one frame's depth mesh at 375 x 1242: the disparity of a forward on seeded structured stereo (fal_net_amd/synthetic.py: structured_stereo, two
seeds) triangulated, cut, re-indexed and written as PLY records by falnet_mesh_build (csrc/mesh.hip: six launches),
(a) with and without normals, by HIP events around single calls into preallocated buffers;
(b) against the existing 3-D export of the same frame: falnet_point_cloud (packed records) plus one falnet_compact_records by the confidence map (four
    launches), timed in the same loop -- the candidates alternate call by call and map by map, REPS rounds after WARM warm-up rounds;
(c) against the numpy definition (tests/_mesh_ref.py: build_ref) on the same box, wall clock;
(d) the bytes each form moves and the HBM floor at 8 TB/s.
The device meshes are checked against the definition byte for byte before anything is timed.  Nothing on the parent commit builds a mesh, so there is no
ratio to hold: the figures are recorded.
usage: python tools/bench_mesh.py [--out profiles/mesh_timing.txt]     (on an MI355X)
       python tools/bench_mesh.py --resource-usage [--out ...]           (anywhere with hipcc: appends what the compiler reports per kernel)"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, REPS, WARM, HOST_REPS = 375, 1242, 200, 20, 3
HBM = 8e12  # bytes per second
MAX_JUMP, MIN_CONF = 0.05, 0.5


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:9.4f}   min {ms[0]:9.4f}   max {ms[-1]:9.4f}"


def resource_usage():
    """What -Rpass-analysis=kernel-resource-usage says of every kernel of mesh.hip, with the build's flags."""
    from fal_net_amd import _build
    cmd = [_build.HIPCC] + _build.FLAGS + _build.FILE_FLAGS["mesh.hip"] + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", os.path.join(_build.CSRC, "mesh.hip"),
                                                                          "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    lines, name = ["--- hipcc -Rpass-analysis=kernel-resource-usage, csrc/mesh.hip (gfx950, -O3 -ffp-contract=off)"], None
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
            lines.append(f"{name:34s} VGPRs {row['VGPRs']:>3s}  SGPRs {row['TotalSGPRs']:>3s}  LDS {row['LDS']:>5s} B  scratch {row['ScratchSize']} B/lane  occupancy {row['Occupancy']} waves/SIMD")
            name = None
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_timing.txt"))
    ap.add_argument("--resource-usage", action="store_true", help="append the compiler's per-kernel report to --out and stop (needs no GPU)")
    a = ap.parse_args()
    if a.resource_usage:
        text = "\n".join(resource_usage()) + "\n"
        print(text, end="")
        with open(a.out, "a") as f:
            f.write(text)
        return
    import torch
    import _mesh_ref as R
    from fal_net_amd import _lib as L
    from fal_net_amd import confidence, dumps, synthetic
    from fal_net_amd.models import FAL_netB
    assert torch.cuda.is_available(), "needs an MI355X"
    lib = L.lib()
    dev = torch.device("cuda", 0)
    model = FAL_netB({"state_dict": synthetic.seeded_falnetb_state_dict(49)}, no_levels=49, compute_dtype=torch.float32).to(dev).eval()
    focal, baseline = dumps.camera_for_width(W)
    n, nq = H * W, (H - 1) * (W - 1)
    frames = []
    for seed in (7, 8):
        left, _, mn, mx = synthetic.structured_stereo(1, H, W, seed=seed)[:4]
        left = left.to(dev)
        st, disp = confidence.from_model(model, left, mn.to(dev), mx.to(dev), ("conf",))
        frames.append(dict(img=left[0].contiguous(), disp=disp[0, 0].float().contiguous(), conf=st["conf"][0, 0].contiguous()))
    st_ptr = L.stream_ptr()
    ws = torch.empty(int(lib.falnet_mesh_workspace_bytes(H, W)) // 8, dtype=torch.int64, device=dev)
    cws = torch.empty(int(lib.falnet_compact_workspace_bytes(n)) // 8, dtype=torch.int64, device=dev)
    for f in frames:
        f["vert"] = {nrm: torch.empty((n * rec + 3) // 4 * 4, dtype=torch.uint8, device=dev) for nrm, rec in ((0, 15), (1, 27))}
        f["face"] = torch.empty((2 * nq * 13 + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        f["counts"] = torch.empty(2, dtype=torch.int64, device=dev)
        f["cloud"], f["kept"] = (torch.empty((n * 15 + 3) // 4 * 4, dtype=torch.uint8, device=dev) for _ in range(2))
        f["ccount"] = torch.empty(1, dtype=torch.int64, device=dev)

    def mesh_call(f, nrm):
        L.check(lib.falnet_mesh_build(L.ptr(f["img"]), dumps.MEAN[0], dumps.MEAN[1], dumps.MEAN[2], 255.0, L.ptr(f["disp"]), focal, baseline, None, 0.0, 0.0, 80.0,
                                      MAX_JUMP, H, W, nrm, L.ptr(f["vert"][nrm]), L.ptr(f["face"]), L.ptr(f["counts"]), L.ptr(ws), st_ptr), "mesh_build")

    def cloud_call(f):
        L.check(lib.falnet_point_cloud(L.ptr(f["img"]), dumps.MEAN[0], dumps.MEAN[1], dumps.MEAN[2], 255.0, L.ptr(f["disp"]), focal, baseline, None, L.ptr(f["cloud"]),
                                       1, H, W, st_ptr), "point_cloud")
        L.check(lib.falnet_compact_records(L.ptr(f["cloud"]), 15, L.ptr(f["conf"]), MIN_CONF, n, L.ptr(f["kept"]), L.ptr(f["ccount"]), L.ptr(cws), st_ptr),
                "compact_records")

    # the check, before any timing: both forms of both frames against the definition
    kept = []
    for f in frames:
        img_h, disp_h = f["img"].cpu().numpy(), f["disp"].cpu().numpy()
        for nrm, rec in ((0, 15), (1, 27)):
            want_v, want_f, _ = R.build_ref(img_h, disp_h, focal, baseline, max_jump=MAX_JUMP, normals=bool(nrm))
            mesh_call(f, nrm)
            nv, nf = f["counts"].tolist()
            assert (nv, nf) == (len(want_v), len(want_f)) and f["vert"][nrm][:nv * rec].cpu().numpy().tobytes() == want_v.tobytes() \
                and f["face"][:nf * 13].cpu().numpy().tobytes() == want_f.tobytes(), "the device mesh differs from the definition: nothing timed"
        cloud_call(f)
        kept.append((nv, nf, int(f["ccount"].item())))
        f["host"] = (img_h, disp_h)
    cands = {"mesh": lambda f: mesh_call(f, 0), "mesh+normals": lambda f: mesh_call(f, 1), "cloud+compact": cloud_call}
    for r in range(WARM):
        for c in cands.values():
            c(frames[r % 2])
    torch.cuda.synchronize()
    ev = {k: [] for k in cands}
    for r in range(REPS):
        for k, c in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c(frames[r % 2])
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    nv, nf, nc = kept[0]
    lines = [f"{H} x {W}: the f32 disparity of FAL_netB (seeded weights, 49 planes) on structured stereo, seeds 7 and 8, KITTI camera of the width; max_jump {MAX_JUMP}, "
             f"depth in (0, 80]; milliseconds",
             f"device: {torch.cuda.get_device_name(0)}; HIP events around single calls, {REPS} rounds after {WARM} warm-up rounds, the three candidates alternating "
             f"inside a round and the two frames from round to round; host figures over {HOST_REPS} calls after one",
             "checked before timing: vertex bytes, face bytes and both counts == tests/_mesh_ref.py build_ref, with and without normals, both frames"]
    for (v, f_, c), seed in zip(kept, (7, 8)):
        lines.append(f"frame seed {seed}: {v} of {n} vertices used ({v / n:.4f}), {f_} of {2 * nq} faces kept ({f_ / (2 * nq):.4f}); cloud: {c} of {n} vertices with conf >= {MIN_CONF} ({c / n:.4f})")
    lines.append(f"{'falnet_mesh_build, 6 launches (code, count, scan, scan, vertices, faces)':76s} {stats(ms['mesh'])}")
    lines.append(f"{'falnet_mesh_build with normals, 6 launches':76s} {stats(ms['mesh+normals'])}")
    lines.append(f"{'falnet_point_cloud packed + falnet_compact_records, 4 launches':76s} {stats(ms['cloud+compact'])}")
    for tag, rec, key in (("mesh", 15, "mesh"), ("mesh with normals", 27, "mesh+normals")):
        # disparity: once by the code kernel, once by the vertex kernel (the neighbours' re-reads stay in cache); image: three planes at the used pixels;
        # codes: written once, read by the count, vertex and face kernels; index map: written once, read once; the records
        moved = 4 * n * 2 + 12 * nv + n * 4 + 4 * n * 2 + rec * nv + 13 * nf
        floor = 4 * n + 12 * nv + rec * nv + 13 * nf
        lines.append(f"{tag + ': bytes moved (disparity x 2, image, codes x 4, index map x 2, records)':76s} {moved / 1e6:9.3f} MB = {moved / (med[key] * 1e-3) / 1e9:7.1f} GB/s; "
                     f"{moved / HBM * 1e3:.5f} ms at 8 TB/s, the call takes {med[key] / (moved / HBM * 1e3):5.1f} x that")
        lines.append(f"{tag + ': HBM floor (disparity and image once, records once)':76s} {floor / 1e6:9.3f} MB; {floor / HBM * 1e3:.5f} ms at 8 TB/s, the call takes "
                     f"{med[key] / (floor / HBM * 1e3):5.1f} x that")
    moved = 4 * n + 12 * n + 15 * n * 2 + 4 * n * 2 + 15 * nc
    lines.append(f"{'cloud + compact: bytes moved (maps, cloud written and read, scores x 2, kept)':76s} {moved / 1e6:9.3f} MB = {moved / (med['cloud+compact'] * 1e-3) / 1e9:7.1f} GB/s")

    def wall(fn):
        fn()
        out = []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    img_h, disp_h = frames[0]["host"]
    lines.append(f"{'host: build_ref (array-wise numpy), no normals':76s} {stats(wall(lambda: R.build_ref(img_h, disp_h, focal, baseline, max_jump=MAX_JUMP)))}")
    lines.append(f"{'host: build_ref (array-wise numpy), normals':76s} {stats(wall(lambda: R.build_ref(img_h, disp_h, focal, baseline, max_jump=MAX_JUMP, normals=True)))}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
