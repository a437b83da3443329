// Velodyne ground truth of the original Eigen split: a raw KITTI scan projected into the camera on the device -- Monodepth's generate_depth_map
// (a numpy chain that ends in a Python loop over every pixel hit twice) as three launches.  The chain, with the matrix product written out:
//   1. keep a point when x >= 0 (f32 compare; a NaN x drops it);
//   2. f64, rows i = 0, 1, 2 of P: s_i = ((P[i][0] x + P[i][1] y) + P[i][2] z) + P[i][3]   (the scan's fourth value is taken as 1);
//   3. u = rint(s_0 / s_2) - 1, v = rint(s_1 / s_2) - 1   (rint: half to even, as np.round);
//   4. depth = (float)s_2, or x itself with vel_depth;
//   5. the point lands on (v, u) when u >= 0 && v >= 0 && u < W && v < H, compared as DOUBLES (NaN and infinity fail, as in numpy);
//   6. a pixel holds the minimum depth of the points on it; no point: 0; a negative minimum: 0 (Monodepth's depth[depth < 0] = 0 comes after its
//      closest-point rule, so a positive point on the same pixel does not survive).
// Two rules hold:
//   * every + and * of step 2 and both divisions are correctly rounded f64 operations in exactly this order: this file is compiled with
//     -ffp-contract=off (no fused multiply-add), so the pixel a point lands on -- a discontinuous function of s -- is the one the host chain finds;
//   * the z-buffer is an integer atomicMin on the monotone 32-bit image of the f32 depth (key_f32 of ordered.h, the key of dump.hip's
//     percentile).  An integer minimum does not depend on arrival order: the map is bit-identical for any order of the points and from run
//     to run.  No floating-point atomics.  Rounding to f32 is monotone, so the minimum of the rounded depths is the rounded minimum.
// The all-ones sentinel of the fill pass is the key of a positive NaN only; a landed point's depth is never NaN (a NaN s_2 fails step 5, and
// with vel_depth x >= 0 has passed step 1).
// Not on the training step's path, not replayable, and not part of the autotune key (ops.py: _TUNE_SOURCES).
#include <math.h>
#include "common.h"
#include "ordered.h"

#define VELO_THREADS 256
#define VELO_EMPTY 0xffffffffu

struct VeloP {
    double m[12];  // row-major 3 x 4, by value in the kernel arguments
};

__global__ __launch_bounds__(VELO_THREADS) void velo_fill_kernel(uint32_t* __restrict__ keys, uint32_t n) {
    const uint32_t i = blockIdx.x * VELO_THREADS + threadIdx.x;
    if (i < n) keys[i] = VELO_EMPTY;
}

__global__ __launch_bounds__(VELO_THREADS) void velo_scatter_kernel(const float* __restrict__ points, uint32_t n_points, VeloP P, int H, int W, int vel_depth,
                                                                    uint32_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * VELO_THREADS + threadIdx.x;
    if (i >= n_points) return;
    const float* pt = points + (size_t)i * 4;
    const float xf = pt[0];
    if (!(xf >= 0.f)) return;
    const double x = (double)xf, y = (double)pt[1], z = (double)pt[2];
    const double s0 = ((P.m[0] * x + P.m[1] * y) + P.m[2] * z) + P.m[3];
    const double s1 = ((P.m[4] * x + P.m[5] * y) + P.m[6] * z) + P.m[7];
    const double s2 = ((P.m[8] * x + P.m[9] * y) + P.m[10] * z) + P.m[11];
    const double u = rint(s0 / s2) - 1.0, v = rint(s1 / s2) - 1.0;
    if (!(u >= 0.0 && v >= 0.0 && u < (double)W && v < (double)H)) return;
    const float d = vel_depth ? xf : (float)s2;
    atomicMin(&keys[(size_t)(int)v * W + (int)u], key_f32(d));  // 0 <= v < H, 0 <= u < W hold as doubles: the index is inside the map
}

// keys -> depths in place: the sentinel and every value that is not positive become 0
__global__ __launch_bounds__(VELO_THREADS) void velo_finish_kernel(uint32_t* __restrict__ keys, uint32_t n) {
    const uint32_t i = blockIdx.x * VELO_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    const float d = unkey_f32(k);
    keys[i] = (k != VELO_EMPTY && d > 0.f) ? __float_as_uint(d) : 0u;
}

extern "C" int falnet_velo_project(const float* points, int n_points, const double* P, int H, int W, int vel_depth, float* depth_out, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "velo_project: map %d x %d must hold between 1 and 2^31 pixels", H, W);
    FALNET_CHECK_ARG(n_points >= 0, "velo_project: n_points %d is negative", n_points);
    FALNET_CHECK_ARG(P, "velo_project: null projection matrix");
    VeloP p;
    for (int i = 0; i < 12; ++i) {
        FALNET_CHECK_ARG(isfinite(P[i]), "velo_project: entry [%d][%d] of the projection matrix is not finite", i / 4, i % 4);
        p.m[i] = P[i];
    }
    FALNET_CHECK_ARG(depth_out, "velo_project: null output map");
    FALNET_CHECK_ARG(n_points == 0 || points, "velo_project: null points with n_points = %d", n_points);
    FALNET_CHECK_ARG((((uintptr_t)points | (uintptr_t)depth_out) & 3) == 0, "velo_project: points and output must be 4-byte aligned");
    const uint32_t n = (uint32_t)H * (uint32_t)W;
    uint32_t* keys = (uint32_t*)depth_out;
    const dim3 map_grid((n + VELO_THREADS - 1) / VELO_THREADS);
    hipLaunchKernelGGL(velo_fill_kernel, map_grid, dim3(VELO_THREADS), 0, (hipStream_t)stream, keys, n);
    if (n_points > 0)
        hipLaunchKernelGGL(velo_scatter_kernel, dim3(((uint32_t)n_points + VELO_THREADS - 1) / VELO_THREADS), dim3(VELO_THREADS), 0, (hipStream_t)stream,
                           points, (uint32_t)n_points, p, H, W, vel_depth, keys);
    hipLaunchKernelGGL(velo_finish_kernel, map_grid, dim3(VELO_THREADS), 0, (hipStream_t)stream, keys, n);
    FALNET_RETURN_LAUNCH();
}
