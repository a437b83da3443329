// Evaluation metrics computed on the device: the KITTI / Make3D depth errors with optional median scaling (myUtils.py:196-334), the end-point
// error (loss_functions.py:124-173) and the view errors RMSE / MAE / PSNR (myUtils.py:123-172).  Every kernel is one HBM-bound pass over planar
// f32 maps as the model returns them; a frame's finished metrics land in one row of a device-resident table of doubles, so an evaluation loop
// reads the table once after its last frame instead of copying two full-size maps to the host per frame.
//
// Three rules hold throughout:
//   * the depth chain (depth_pair.h, shared with sparsify.hip) is f64 per pixel in the HOST's order (the host chain is float64 because `1.0 -
//     mask` promotes it; the `< 1.25^n` counts are discontinuous, so f32 arithmetic would flip pixels near a threshold).  This file is compiled
//     with -ffp-contract=off: no fused multiply-add, correctly rounded f64 division and square root.  One thing the host does in f32 is done in
//     f32 here too: the Eigen / Make3D ground truth stays an f32 array on the host, so np.median of it takes the mean of the two middle values
//     in f32 (the scale factor is compared at 1e-14).  The host's np.log of that f32 array is an f32 logarithm as well; the kernel takes the f64
//     one, the correctly rounded value of which the host's is a rounding (measured closer to the host than the device's own logf, which rounds
//     differently);
//   * every reduction is deterministic by construction: a FIXED grid of MET_BLOCKS workgroups writes one line of partial sums each (wave
//     shuffles, then the four waves in order), and a finalising kernel adds the lines in index order.  No floating-point atomics; the
//     radix select counts with integer atomics, whose sums do not depend on arrival order;
//   * nothing is read by the host: the median scale factor goes from the select to the error kernel through device memory.
// None of this is on the training step's path and none of it is part of the autotune key (ops.py: _TUNE_SOURCES).
#include "common.h"
#include "depth_pair.h"
#include "ordered.h"

#define MET_BLOCKS 256
#define MET_THREADS 256
#define MET_NSUM 8  // partial sums per workgroup (doubles; counts are exact integers far below 2^53)
// workspace, in 64-bit words: the partial sums, then the state of the median select, then its histograms (32-bit counters, two per word)
#define MED_STATE 16  // [0..3] prefixes of the four slots, [4..7] ranks still to skip, [8] n, [9..12] the four order statistics (f64 bits)
#define MED_PASSES 8
#define MED_SLOTS 4  // 0, 1: ground truth, lower / upper middle; 2, 3: prediction
#define MED_HIST_WORDS32 (MED_PASSES * MED_SLOTS * 256)
#define MET_WS_WORDS64 (MET_BLOCKS * MET_NSUM + MED_STATE + MED_HIST_WORDS32 / 2)

extern "C" int64_t falnet_metrics_workspace_bytes(void) { return (int64_t)MET_WS_WORDS64 * 8; }

// ---- block reduction: NS doubles per thread -> one line of partial sums per workgroup ------------------------------------------------------
template <int NS> __device__ __forceinline__ void store_partials(double (&v)[NS], double* __restrict__ partials) {
    __shared__ double red[MET_THREADS / 64][NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = wave_sum_f64(v[k]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) red[w][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < MET_NSUM) {  // every line has MET_NSUM entries: the unused ones are written 0, the finaliser adds whole lines
        double s = 0.0;
        if (threadIdx.x < NS)
            for (int i = 0; i < MET_THREADS / 64; ++i) s += red[i][threadIdx.x];
        partials[(size_t)blockIdx.x * MET_NSUM + threadIdx.x] = s;
    }
}

// ---- np.median of gt[mask] and pred[mask] on the device -------------------------------------------------------------------------------------
// A radix select (the scheme of dump.hip's percentile) over the f64 DEPTHS themselves, with a predicate (mask and crop) and a 64-bit key
// (key_f64 of ordered.h): eight passes of 8 bits.  The alternative -- selecting on the f32 disparities and converting the two order statistics afterwards -- is exact only
// where the depth is monotone in the stored value, and the prediction's is not: a disparity <= 0 takes the denominator d + 1, an f64 that
// need not be an f32, and a negative denominator gives a negative depth that sorts below every positive one.  Selecting the values numpy sorts
// needs no such case analysis.  The number of selected pixels is the sum of the first pass's histogram; the ranks (n - 1) / 2 and n / 2 follow
// from it on the device.
__global__ __launch_bounds__(MET_THREADS) void median_hist_kernel(DepthArgs a, uint64_t* __restrict__ state, uint32_t* __restrict__ tables, int pass) {
    __shared__ uint32_t hist[MED_SLOTS][256];
    for (int s = 0; s < MED_SLOTS; ++s) hist[s][threadIdx.x] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const bool all = pass == 0;  // no prefix yet: every selected pixel counts (a shift by 64 is not defined, hence the flag)
    uint64_t pre[MED_SLOTS];
#pragma unroll
    for (int s = 0; s < MED_SLOTS; ++s) pre[s] = all ? 0 : state[s];
    const uint32_t n = (uint32_t)a.rh * (uint32_t)a.rw;
    for (uint32_t i = blockIdx.x * MET_THREADS + threadIdx.x; i < n; i += gridDim.x * MET_THREADS) {
        double g, p;
        if (!depth_pair(a, i, g, p)) continue;
        const uint64_t kg = key_f64(g), kp = key_f64(p);
        const uint64_t hg = all ? 0 : (kg >> (shift + 8)), hp = all ? 0 : (kp >> (shift + 8));
        const uint32_t bg = (uint32_t)(kg >> shift) & 255u, bp = (uint32_t)(kp >> shift) & 255u;
        if (hg == pre[0]) atomicAdd(&hist[0][bg], 1u);
        if (hg == pre[1]) atomicAdd(&hist[1][bg], 1u);
        if (hp == pre[2]) atomicAdd(&hist[2][bp], 1u);
        if (hp == pre[3]) atomicAdd(&hist[3][bp], 1u);
    }
    __syncthreads();
    uint32_t* table = tables + (size_t)pass * MED_SLOTS * 256;
    for (int s = 0; s < MED_SLOTS; ++s) {
        const uint32_t c = hist[s][threadIdx.x];
        if (c) atomicAdd(&table[s * 256 + threadIdx.x], c);
    }
}

// one workgroup of four waves: wave s resolves slot s (its lane 0 walks the 256 bins).  After the last pass: scale_out = {factor, median of the
// ground truth, median of the prediction, n}; n = 0 gives NaN like np.median of an empty array.
__global__ __launch_bounds__(256) void median_select_kernel(uint64_t* __restrict__ state, const uint32_t* __restrict__ tables, int pass, int gt_is_f32,
                                                            double* __restrict__ scale_out) {
    __shared__ uint32_t cnt[MED_SLOTS][256];
    __shared__ double stat[MED_SLOTS];
    const uint32_t* table = tables + (size_t)pass * MED_SLOTS * 256;
    for (int i = threadIdx.x; i < MED_SLOTS * 256; i += 256) cnt[i >> 8][i & 255] = table[i];
    __syncthreads();
    const int slot = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        uint64_t rank;
        if (pass == 0) {
            uint64_t n = 0;
            for (int b = 0; b < 256; ++b) n += cnt[slot][b];
            rank = n == 0 ? 0 : ((slot & 1) ? n / 2 : (n - 1) / 2);
            if (slot == 0) state[8] = n;
        } else {
            rank = state[4 + slot];
        }
        uint32_t bin = 0;
        // the counts of a slot sum to more than `rank` (rank < n in pass 0, rank < the count of the chosen bin from then on), unless n = 0
        for (; bin < 255 && rank >= cnt[slot][bin]; ++bin) rank -= cnt[slot][bin];
        const uint64_t prefix = ((pass == 0 ? 0ull : state[slot]) << 8) | bin;
        state[slot] = prefix;
        state[4 + slot] = rank;
        if (pass == MED_PASSES - 1) {
            stat[slot] = unkey_f64(prefix);
            state[9 + slot] = (uint64_t)__double_as_longlong(stat[slot]);
        }
    }
    if (pass != MED_PASSES - 1) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t n = state[8];
        // numpy: the mean of the two middle order statistics (the same element twice for an odd count), in the array's own type -- the
        // Eigen / Make3D ground truth is an f32 array on the host (a + b and the division by 2 round to f32), everything else is f64
        double mg = gt_is_f32 ? (double)(((float)stat[0] + (float)stat[1]) / 2.f) : (stat[0] + stat[1]) / 2.0;
        double mp = (stat[2] + stat[3]) / 2.0;
        if (n == 0) mg = mp = __longlong_as_double(0x7ff8000000000000ll);
        scale_out[0] = mg / mp;
        scale_out[1] = mg;
        scale_out[2] = mp;
        scale_out[3] = (double)n;
    }
}

// ---- the error sums (compute_kitti_errors / compute_make_errors) --------------------------------------------------------------------------------
__global__ __launch_bounds__(MET_THREADS) void depth_errors_kernel(DepthArgs a, const double* __restrict__ scale, double min_d, double max_d,
                                                                   double* __restrict__ partials) {
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // n, sum |d| / gt, sum d^2 / gt, sum d^2, sum of the log term, n(< 1.25), n(< 1.25^2), n(< 1.25^3)
    uint32_t cn = 0, c1 = 0, c2 = 0, c3 = 0;
    const bool scaled = scale != nullptr;
    const double factor = scaled ? scale[0] : 1.0;
    const uint32_t n = (uint32_t)a.rh * (uint32_t)a.rw;
    for (uint32_t i = blockIdx.x * MET_THREADS + threadIdx.x; i < n; i += gridDim.x * MET_THREADS) {
        double g, p;
        if (!depth_pair(a, i, g, p)) continue;
        const double t = depth_scale_clamp(g, p, scaled, factor, min_d, max_d);
        cn += 1;
        c1 += t < 1.25 ? 1u : 0u;
        c2 += t < 1.5625 ? 1u : 0u;    // 1.25 ** 2, exact
        c3 += t < 1.953125 ? 1u : 0u;  // 1.25 ** 3, exact
        const double d = g - p, d2 = d * d;
        v[1] += fabs(d) / g;
        v[2] += d2 / g;
        v[3] += d2;
        if (a.mode == FALNET_DEPTH_MAKE3D) {  // |log10 gt - log10 pred|
            v[4] += fabs(log10(g) - log10(p));
        } else {  // (ln gt - ln pred)^2
            const double l = log(g) - log(p);
            v[4] += l * l;
        }
    }
    v[0] = (double)cn, v[5] = (double)c1, v[6] = (double)c2, v[7] = (double)c3;
    store_partials<8>(v, partials);
}

// ---- end-point error: bilinear (align_corners=True) sample of the prediction at the target's size, |target - up| --------------------------------
// the sampling arithmetic is falnet_resize_planar's (f32; equal sizes give weights 0 and 1: the identity)
__global__ __launch_bounds__(MET_THREADS) void epe_kernel(const float* __restrict__ pred, int h, int w, const float* __restrict__ target, int H, int W,
                                                          int sparse, uint32_t total, double* __restrict__ partials) {
    const float ry = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, rx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    double v[2] = {0.0, 0.0};  // n, sum |target - up|
    uint32_t cn = 0;
    for (uint32_t i = blockIdx.x * MET_THREADS + threadIdx.x; i < total; i += gridDim.x * MET_THREADS) {
        const float t = target[i];
        if (sparse && t == 0.f) continue;
        const int ox = (int)(i % (uint32_t)W), oy = (int)((i / (uint32_t)W) % (uint32_t)H);
        const float* pl = pred + (size_t)(i / ((uint32_t)W * (uint32_t)H)) * ((size_t)h * w);
        const float fy = ry * oy, fx = rx * ox;
        const int y0 = min((int)fy, h - 1), x0 = min((int)fx, w - 1);
        const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
        const float wy = fy - y0, wx = fx - x0;
        const float up = (1.f - wy) * ((1.f - wx) * pl[(size_t)y0 * w + x0] + wx * pl[(size_t)y0 * w + x1]) +
                         wy * ((1.f - wx) * pl[(size_t)y1 * w + x0] + wx * pl[(size_t)y1 * w + x1]);
        cn += 1;
        v[1] += (double)fabsf(t - up);
    }
    v[0] = (double)cn;
    store_partials<2>(v, partials);
}

// ---- view errors: the three sums behind get_rmse, get_mea and get_psnr ---------------------------------------------------------------------
// out = clamp((x + mean) * 255, 0, 255), lab = (y + mean) * 255 in f32 as torch forms them; sums of d^2, |d| and (round(out) - lab)^2 in f64
__global__ __launch_bounds__(MET_THREADS) void view_errors_kernel(const float* __restrict__ x, const float* __restrict__ y, float m0, float m1, float m2,
                                                                  uint32_t hw, uint32_t total, double* __restrict__ partials) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};  // n, sum d^2, sum |d|, sum (round(out) - lab)^2
    for (uint32_t i = blockIdx.x * MET_THREADS + threadIdx.x; i < total; i += gridDim.x * MET_THREADS) {
        const uint32_t c = (i / hw) % 3u;
        const float m = c == 0 ? m0 : (c == 1 ? m1 : m2);
        const float o = fminf(fmaxf((x[i] + m) * 255.f, 0.f), 255.f), l = (y[i] + m) * 255.f;
        const double d = (double)(o - l), r = (double)(rintf(o) - l);  // torch.round: half to even
        v[1] += d * d;
        v[2] += fabs(d);
        v[3] += r * r;
    }
    // every thread takes the same number of elements up to one: the count is the total
    v[0] = threadIdx.x == 0 && blockIdx.x == 0 ? (double)total : 0.0;
    store_partials<4>(v, partials);
}

// ---- finaliser: the MET_BLOCKS lines in index order -> the finished metrics in the caller's row ----------------------------------------------
__global__ __launch_bounds__(64) void metrics_finalize_kernel(const double* __restrict__ partials, int kind, int mode, const double* __restrict__ scale,
                                                              double* __restrict__ row) {
    __shared__ double s[MET_NSUM];
    if (threadIdx.x < MET_NSUM) {
        double t = 0.0;
        for (int b = 0; b < MET_BLOCKS; ++b) t += partials[(size_t)b * MET_NSUM + threadIdx.x];
        s[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = s[0];  // n = 0: 0 / 0 = NaN, as numpy's mean of an empty array
    if (kind == 0) {  // depth errors
        row[FALNET_MET_ABS_REL] = s[1] / n;
        row[FALNET_MET_SQ_REL] = s[2] / n;
        row[FALNET_MET_RMS] = sqrt(s[3] / n);
        row[FALNET_MET_LOG] = mode == FALNET_DEPTH_MAKE3D ? s[4] / n : sqrt(s[4] / n);
        row[FALNET_MET_A1] = s[5] / n;
        row[FALNET_MET_A2] = s[6] / n;
        row[FALNET_MET_A3] = s[7] / n;
        row[FALNET_MET_N] = n;
        row[FALNET_MET_N_A1] = s[5];
        row[FALNET_MET_N_A2] = s[6];
        row[FALNET_MET_N_A3] = s[7];
        row[FALNET_MET_SCALE] = scale ? scale[0] : 1.0;
        row[FALNET_MET_MEDIAN_GT] = scale ? scale[1] : 0.0;
        row[FALNET_MET_MEDIAN_PRED] = scale ? scale[2] : 0.0;
    } else if (kind == 1) {  // end-point error
        row[FALNET_MET_EPE] = s[1] / n;
        row[FALNET_MET_EPE_N] = n;
    } else {  // view errors
        row[FALNET_MET_RMSE] = sqrt(s[1] / n);
        row[FALNET_MET_MEA] = s[2] / n;
        row[FALNET_MET_PSNR] = 20.0 * log10(255.0 / sqrt(s[3] / n));
        row[FALNET_MET_VIEW_SUM_SQ] = s[1];
        row[FALNET_MET_VIEW_SUM_ABS] = s[2];
        row[FALNET_MET_VIEW_SUM_RSQ] = s[3];
        row[FALNET_MET_VIEW_N] = n;
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------------------
static inline double* ws_partials(void* ws) { return (double*)ws; }
static inline uint64_t* ws_state(void* ws) { return (uint64_t*)ws + MET_BLOCKS * MET_NSUM; }
static inline uint32_t* ws_tables(void* ws) { return (uint32_t*)((uint64_t*)ws + MET_BLOCKS * MET_NSUM + MED_STATE); }

extern "C" int falnet_depth_median_scale(const float* pred_disp, const float* gt, int H, int W, int mode, double fb, double max_d, double* scale_out,
                                         void* workspace, void* stream) {
    FALNET_ENTER(stream);
    DepthArgs a;
    if (depth_args(a, pred_disp, gt, H, W, mode, fb, max_d, "depth_median_scale")) return -1;
    FALNET_CHECK_ARG(scale_out && workspace, "depth_median_scale: null output or workspace");
    FALNET_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)scale_out & 7) == 0, "depth_median_scale: workspace and output must be 8-byte aligned");
    hipError_t e = hipMemsetAsync(ws_state(workspace), 0, (size_t)MED_STATE * 8 + (size_t)MED_HIST_WORDS32 * 4, (hipStream_t)stream);
    if (e != hipSuccess) {
        falnet_set_error("depth_median_scale: clearing the workspace failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    for (int pass = 0; pass < MED_PASSES; ++pass) {
        hipLaunchKernelGGL(median_hist_kernel, dim3(MET_BLOCKS), dim3(MET_THREADS), 0, (hipStream_t)stream, a, ws_state(workspace), ws_tables(workspace), pass);
        hipLaunchKernelGGL(median_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws_state(workspace), ws_tables(workspace), pass,
                           (int)(mode != FALNET_DEPTH_KITTI2015), scale_out);
    }
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_depth_errors(const float* pred_disp, const float* gt, int H, int W, int mode, double fb, const double* scale, double min_d, double max_d,
                                   double* row, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    DepthArgs a;
    if (depth_args(a, pred_disp, gt, H, W, mode, fb, max_d, "depth_errors")) return -1;
    FALNET_CHECK_ARG(row && workspace, "depth_errors: null row or workspace");
    FALNET_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)row & 7) == 0 && ((uintptr_t)scale & 7) == 0,
                     "depth_errors: workspace, row and scale must be 8-byte aligned");
    FALNET_CHECK_ARG(min_d > 0.0 && max_d >= min_d, "depth_errors: need 0 < min_d <= max_d");
    FALNET_CHECK_ARG(mode != FALNET_DEPTH_MAKE3D || scale, "depth_errors: make3d is always median-scaled (scale from falnet_depth_median_scale)");
    hipLaunchKernelGGL(depth_errors_kernel, dim3(MET_BLOCKS), dim3(MET_THREADS), 0, (hipStream_t)stream, a, scale, min_d, max_d, ws_partials(workspace));
    hipLaunchKernelGGL(metrics_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws_partials(workspace), 0, mode, scale, row);
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_epe(const float* pred, int h, int w, const float* target, int B, int H, int W, int sparse, double* row, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(pred && target && row && workspace, "epe: null argument");
    FALNET_CHECK_ARG(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "epe: empty map");
    FALNET_CHECK_ARG((int64_t)B * H * W < ((int64_t)1 << 31) && (int64_t)B * h * w < ((int64_t)1 << 31), "epe: more than 2^31 pixels");
    FALNET_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)row & 7) == 0, "epe: workspace and row must be 8-byte aligned");
    hipLaunchKernelGGL(epe_kernel, dim3(MET_BLOCKS), dim3(MET_THREADS), 0, (hipStream_t)stream, pred, h, w, target, H, W, sparse, (uint32_t)B * H * W,
                       ws_partials(workspace));
    hipLaunchKernelGGL(metrics_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws_partials(workspace), 1, 0, (const double*)nullptr, row);
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_view_errors(const float* out, const float* label, float mean_r, float mean_g, float mean_b, int B, int H, int W, double* row,
                                  void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(out && label && row && workspace, "view_errors: null argument");
    FALNET_CHECK_ARG(B > 0 && H > 0 && W > 0 && (int64_t)B * 3 * H * W < ((int64_t)1 << 31), "view_errors: between 1 and 2^31 values");
    FALNET_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)row & 7) == 0, "view_errors: workspace and row must be 8-byte aligned");
    hipLaunchKernelGGL(view_errors_kernel, dim3(MET_BLOCKS), dim3(MET_THREADS), 0, (hipStream_t)stream, out, label, mean_r, mean_g, mean_b, (uint32_t)H * W,
                       (uint32_t)B * 3 * H * W, ws_partials(workspace));
    hipLaunchKernelGGL(metrics_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws_partials(workspace), 2, 0, (const double*)nullptr, row);
    FALNET_RETURN_LAUNCH();
}
