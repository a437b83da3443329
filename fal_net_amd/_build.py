"""Build libfalnet_hip.so (gfx950 code objects + C-ABI host stubs) in-tree with hipcc.

`python -m fal_net_amd._build` or `__graft_entry__.build()`.  hipcc cross-compiles without a GPU;
the resulting .so travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "csrc", "_obj")
LIB = os.path.join(HERE, "libfalnet_hip.so")
SOURCES = ["api.cpp", "replay.cpp", "med_head.hip", "med_head2.hip", "med_sweep.hip", "med_pose.hip", "inpaint.hip", "med_stats.hip", "compact.hip", "losses.hip", "adam.hip", "elementwise.hip", "data.hip", "augment_batch.hip", "dump.hip", "metrics.hip", "ssim.hip", "velo.hip", "lidar.hip", "mesh.hip", "components.hip", "sort.hip", "sparsify.hip", "nearest.hip", "ground.hip", "wgrad_rows.hip", "wgrad_wave.hip", "wgrad.hip", "pack.hip", "conv_wave.hip", "conv_dma.hip", "conv.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]
# Per-file flags.  The MED head kernels are f32 VALU work per pixel and plane: the SLP vectoriser pairs independent scalar
# f32 operations into v_pk_* with extra moves to form the pairs, which is slower here (forward 88 -> 79 us, backward 157 -> 153 us
# at 8x192x640x49, same box: profiles/r05_ab_head_noslp.txt).
# dump.hip reproduces the host's f32 arithmetic operation by operation (its 8-bit outputs are compared with numpy byte for byte): a
# multiply and an add must not contract into one fused multiply-add there.  metrics.hip restates the host's float64 metric chain in the host's
# order for the same reason (its threshold counts are compared with numpy's as integers).  augment_batch.hip restates the host's float64
# resampling coefficients (data_transforms.resample_coeffs) for the same reason: its 22-bit integers must equal the host's.  velo.hip
# restates the host's float64 projection sums in a fixed order: the pixel a point lands on must be the host's; lidar.hip, its inverse, restates
# the host's float64 back-projection and bin search the same way: a record and its bin must be the host's bit for bit.  sparsify.hip runs
# the depth chain of metrics.hip per pixel (csrc/depth_pair.h, whose includers all need the flag): its errors order the pixels and its d1 counts
# are compared with numpy's as integers.  ssim.hip forms the metric's 0..255 operands in f32 as torch does (an add, a multiply, a rounding half to
# even): contracted into a fused multiply-add, pixels cross a rounding boundary.  mesh.hip runs the point cloud's f32 vertex chain (csrc/pc_vertex.h,
# whose includers all need the flag) and sums its normals in float64 in a fixed order: a vertex record and a kept triangle must be the host's bit for bit.
# nearest.hip forms a pair's squared distance in f32 in a stated order (three differences, three products, two sums): contracted, a nearest distance
# and the index that attains it would no longer be the host's bit for bit.  ground.hip forms a point's vertical residual to a plane in f32 and a
# hypothesis plane in f64 in stated orders: contracted, an inlier count, a stored plane and a height would no longer be the host's bit for bit.
FILE_FLAGS = {"med_head.hip": ["-fno-slp-vectorize"], "med_head2.hip": ["-fno-slp-vectorize"], "med_sweep.hip": ["-fno-slp-vectorize"],
              "med_stats.hip": ["-fno-slp-vectorize"], "med_pose.hip": ["-fno-slp-vectorize"],
              "dump.hip": ["-ffp-contract=off"],
              "metrics.hip": ["-ffp-contract=off"], "ssim.hip": ["-ffp-contract=off"], "augment_batch.hip": ["-ffp-contract=off"], "velo.hip": ["-ffp-contract=off"],
              "lidar.hip": ["-ffp-contract=off"], "sparsify.hip": ["-ffp-contract=off"], "mesh.hip": ["-ffp-contract=off"],
              "nearest.hip": ["-ffp-contract=off"], "ground.hip": ["-ffp-contract=off"]}


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def build_ab(tag="ab", defines=(), verbose=True, raw=()):
    """Experiment build: the same sources with -DFALNET_AB (the FALNET_* kernel switches of include/falnet_hip.h are honoured) plus
    extra -D flags -> fal_net_amd/libfalnet_hip_<tag>.so, selected at run time with FALNET_LIB=<path>.  Never the product library."""
    obj_dir = os.path.join(CSRC, "_obj_" + tag)
    os.makedirs(obj_dir, exist_ok=True)
    flags = FLAGS + ["-DFALNET_AB"] + ["-D" + d for d in defines]
    lib = os.path.join(HERE, f"libfalnet_hip_{tag}.so")

    def run(src):
        cmd = [HIPCC] + flags + FILE_FLAGS.get(src, []) + list(raw) + (["-x", "hip"] if src.endswith(".hip") else []) + ["-c", os.path.join(CSRC, src), "-o", os.path.join(obj_dir, src + ".o")]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, SOURCES))
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + [os.path.join(obj_dir, s + ".o") for s in SOURCES], check=True)
    return lib


def build(force=False, verbose=True):
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "conv_epilogue.h"), os.path.join(CSRC, "adam.h"), os.path.join(CSRC, "ordered.h"), os.path.join(CSRC, "depth_pair.h"), os.path.join(CSRC, "med_planes.h"), os.path.join(CSRC, "pc_vertex.h"), os.path.join(CSRC, "wgrad_dispatch.h"), os.path.join(HERE, "..", "include", "falnet_hip.h")]
    jobs = []
    for src in SOURCES:
        path = os.path.join(CSRC, src)
        obj = os.path.join(OBJ, src + ".o")
        if force or _stale(obj, [path] + headers):
            cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(src, []) + (["-x", "hip"] if src.endswith(".hip") else []) + ["-c", path, "-o", obj]
            jobs.append(cmd)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(OBJ, s + ".o") for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    if "--ab" in sys.argv:  # python -m fal_net_amd._build --ab [tag] [-DNAME[=V] ...] [-f<compiler flag> ...]
        rest = [a for a in sys.argv[sys.argv.index("--ab") + 1:]]
        tag = next((a for a in rest if not a.startswith("-")), "ab")
        print(build_ab(tag, [a[2:] for a in rest if a.startswith("-D")], raw=[a for a in rest if a.startswith("-") and not a.startswith("-D")]))
    else:
        build(force="--force" in sys.argv)
        print(LIB)
