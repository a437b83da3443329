// Cloud metrics: the nearest neighbour between two point sets (falnet_nearest) and the sums behind the Chamfer distance and the F-score
// (falnet_cloud_errors).  include/falnet_hip.h; the numpy restatement is tests/_cloud_ref.py.
//
// A record is 4 consecutive f32 x, y, z, . -- the 16-byte point of falnet_velo_unproject and of a KITTI .bin file; the fourth value is ignored.
// For a query q and a reference r:
//   dx = qx - rx, dy = qy - ry, dz = qz - rz;   d2(q, r) = (dx dx + dy dy) + dz dz
// every operation rounded to f32 in this order, no fused multiply-add: the file is compiled with -ffp-contract=off.  A pair whose d2 is NaN (a
// non-finite coordinate, inf - inf) does not take part.  d2[q] is the minimum over the pairs that take part, idx[q] the smallest r that attains
// it; no pair taking part: d2 = +inf, idx = -1.
// Why the result is exact: a minimum does not depend on order; d2 is >= +0 or NaN (a product of equal factors is >= +0, and +0 + +0 = +0), so
// its bit pattern is monotone as an unsigned integer, every NaN above +inf; the 64-bit key (bits(d2) << 32) | r -- the idiom of lidar.hip --
// decides value and tie together.  Any decomposition of the reference set gives the same (d2, idx).
//
//   nn_kernel         workgroup (bx, s) owns the NN_BLOCK queries from bx NN_BLOCK on -- NN_QPT per thread, in registers -- and walks the
//                     reference range of split s through LDS tiles of NN_TILE records.  Every lane reads the same LDS address per reference
//                     (identical addresses broadcast: no bank conflict).  References are visited in increasing index and the running
//                     (bits(d2), r) of a query is replaced on strict <, as unsigned integers, starting from the smallest pattern above +inf:
//                     a NaN never enters, +inf does.  One split: the result is stored plainly.  S > 1: one integer atomicMin per query on
//                     a u64 key of the workspace.
//   nn_fill_kernel    S > 1: the workspace's keys set to all ones -- no pair's key: its upper half is a NaN's pattern
//   nn_finish_kernel  S > 1: key -> (d2, idx)
// No workgroup waits for another, every loop is bounded by nr, no floating-point atomics, nothing cooperative.
//
//   ce_partial_kernel workgroup (b, direction) of a FIXED grid sums its stride of one d2 array in f64: n, sum sqrt((double)d2), sum (double)d2
//                     and per threshold #{(double)d2 <= tau2[k]} over the finite entries -- a thread's stride in order, wave_sum_f64, the
//                     four waves in order
//   ce_final_kernel   one thread per column adds the CE_BLOCKS partials in block order and writes the row
// Two calls give the same bits.  Not on the training step's path, not replayable, and not part of the autotune key (ops.py: _TUNE_SOURCES).
#include <math.h>
#include "common.h"
#include "ordered.h"

#define NN_THREADS 256
#define NN_QPT 4
#define NN_BLOCK (NN_THREADS * NN_QPT)  // queries per workgroup (cloud_metrics.QUERY_BLOCK)
#define NN_TILE 1024                    // reference records per LDS tile (cloud_metrics.REF_TILE)
#define NN_TARGET_WGS 512               // the default split rule fills this many workgroups (cloud_metrics.TARGET_WORKGROUPS)
#define NN_MAX_SPLITS 1024
#define NN_EMPTY 0xffffffffffffffffull
#define NN_ABOVE_INF 0x7f800001u  // the smallest bit pattern above +inf: what a running minimum starts from

#define CE_THREADS 256
#define CE_BLOCKS 64
#define CE_MAX_K FALNET_CLOUD_MAX_THRESHOLDS
#define CE_COLS (3 + CE_MAX_K)  // per direction: n, sum sqrt, sum, K counts

static_assert(NN_TILE % NN_THREADS == 0, "a tile is staged in whole rounds of the workgroup");
static_assert(FALNET_CLOUD_ROW == 2 * CE_COLS, "the row holds both directions");

// ---- nearest neighbour ----------------------------------------------------------------------------------------------------------------------
// refs [r_begin, r_end) of split blockIdx.y; SPLIT: the result goes to keys[] by atomicMin, else to d2[] / idx[]
template <bool SPLIT>
__global__ __launch_bounds__(NN_THREADS) void nn_kernel(const float4* __restrict__ query, uint32_t nq, const float4* __restrict__ ref, uint32_t nr,
                                                        uint32_t tiles_per_split, float* __restrict__ d2, int32_t* __restrict__ idx,
                                                        unsigned long long* __restrict__ keys) {
    __shared__ float4 tile[NN_TILE];
    const uint32_t q0 = blockIdx.x * NN_BLOCK + threadIdx.x;
    const uint64_t r_first = (uint64_t)blockIdx.y * tiles_per_split * NN_TILE;
    const uint64_t r_last = r_first + (uint64_t)tiles_per_split * NN_TILE;
    const uint32_t r_begin = r_first < nr ? (uint32_t)r_first : nr, r_end = r_last < nr ? (uint32_t)r_last : nr;
    if (r_begin >= r_end && SPLIT) return;  // an empty split offers nothing (the whole workgroup leaves: no barrier is passed)
    float qx[NN_QPT], qy[NN_QPT], qz[NN_QPT];
    uint32_t best[NN_QPT], arg[NN_QPT];
#pragma unroll
    for (int k = 0; k < NN_QPT; ++k) {
        const uint32_t q = q0 + k * NN_THREADS;
        const float4 v = q < nq ? query[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        qx[k] = v.x, qy[k] = v.y, qz[k] = v.z;
        best[k] = NN_ABOVE_INF, arg[k] = 0xffffffffu;
    }
    for (uint32_t base = r_begin; base < r_end; base += NN_TILE) {  // base + NN_TILE <= 2^31 + NN_TILE: no wrap
        const uint32_t cnt = r_end - base < NN_TILE ? r_end - base : NN_TILE;
        __syncthreads();  // the previous tile has been read
#pragma unroll
        for (int k = 0; k < NN_TILE / NN_THREADS; ++k) {
            const uint32_t j = k * NN_THREADS + threadIdx.x;
            if (j < cnt) tile[j] = ref[base + j];  // base + j < r_end <= nr
        }
        __syncthreads();
#pragma unroll 4
        for (uint32_t j = 0; j < cnt; ++j) {
            const float4 r = tile[j];  // one address for the whole wave
            const uint32_t ri = base + j;
#pragma unroll
            for (int k = 0; k < NN_QPT; ++k) {
                const float dx = qx[k] - r.x, dy = qy[k] - r.y, dz = qz[k] - r.z;
                const uint32_t b = __float_as_uint((dx * dx + dy * dy) + dz * dz);
                const bool lt = b < best[k];
                best[k] = lt ? b : best[k];
                arg[k] = lt ? ri : arg[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NN_QPT; ++k) {
        const uint32_t q = q0 + k * NN_THREADS;
        if (q >= nq) continue;
        const bool any = arg[k] != 0xffffffffu;
        if (SPLIT) {
            if (any) atomicMin(&keys[q], ((unsigned long long)best[k] << 32) | (unsigned long long)arg[k]);  // q < nq: inside the workspace
        } else {
            d2[q] = any ? __uint_as_float(best[k]) : INFINITY;
            idx[q] = any ? (int32_t)arg[k] : -1;
        }
    }
}

__global__ __launch_bounds__(NN_THREADS) void nn_fill_kernel(unsigned long long* __restrict__ keys, uint32_t nq) {
    const uint32_t q = blockIdx.x * NN_THREADS + threadIdx.x;
    if (q < nq) keys[q] = NN_EMPTY;
}

__global__ __launch_bounds__(NN_THREADS) void nn_finish_kernel(const unsigned long long* __restrict__ keys, uint32_t nq, float* __restrict__ d2,
                                                               int32_t* __restrict__ idx) {
    const uint32_t q = blockIdx.x * NN_THREADS + threadIdx.x;
    if (q >= nq) return;
    const unsigned long long k = keys[q];
    d2[q] = k == NN_EMPTY ? INFINITY : __uint_as_float((uint32_t)(k >> 32));
    idx[q] = k == NN_EMPTY ? -1 : (int32_t)(uint32_t)k;
}

static inline int64_t nn_tiles(int64_t nr) { return (nr + NN_TILE - 1) / NN_TILE; }
static inline bool nn_shape_ok(int64_t nq, int64_t nr) { return nq >= 0 && nr >= 0 && nq < ((int64_t)1 << 31) && nr < ((int64_t)1 << 31); }

// the default split rule: enough splits of the reference range that ceil(nq / NN_BLOCK) * S reaches NN_TARGET_WGS workgroups, at most one split
// per tile
extern "C" int falnet_nearest_splits(int64_t nq, int64_t nr) {
    if (!nn_shape_ok(nq, nr) || nq == 0 || nr == 0) return nn_shape_ok(nq, nr) ? 1 : 0;
    const int64_t blocks = (nq + NN_BLOCK - 1) / NN_BLOCK, tiles = nn_tiles(nr);
    int64_t s = (NN_TARGET_WGS + blocks - 1) / blocks;
    if (s > tiles) s = tiles;
    if (s > NN_MAX_SPLITS) s = NN_MAX_SPLITS;
    return (int)(s < 1 ? 1 : s);
}

extern "C" int64_t falnet_nearest_workspace_bytes(int64_t nq, int64_t nr, int splits) {
    if (!nn_shape_ok(nq, nr) || splits < 0 || splits > NN_MAX_SPLITS) return 0;
    const int s = splits == 0 ? falnet_nearest_splits(nq, nr) : splits;
    return s > 1 ? nq * (int64_t)sizeof(unsigned long long) : 0;
}

extern "C" int falnet_nearest(const float* query, int64_t nq, const float* ref, int64_t nr, int splits, float* d2, int32_t* idx, void* workspace,
                              void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(nn_shape_ok(nq, nr), "nearest: nq = %lld and nr = %lld must lie in [0, 2^31)", (long long)nq, (long long)nr);
    FALNET_CHECK_ARG(splits >= 0 && splits <= NN_MAX_SPLITS, "nearest: splits %d outside [0, %d] (0: the library's choice)", splits, NN_MAX_SPLITS);
    if (nq == 0) return 0;  // nothing to write, nothing launched
    FALNET_CHECK_ARG(query && d2 && idx, "nearest: null query, d2 or idx");
    FALNET_CHECK_ARG(nr == 0 || ref, "nearest: null ref with nr = %lld", (long long)nr);
    FALNET_CHECK_ARG((((uintptr_t)query | (uintptr_t)ref) & 15) == 0, "nearest: query and ref must be 16-byte aligned (one record is one 16-byte load)");
    FALNET_CHECK_ARG((((uintptr_t)d2 | (uintptr_t)idx) & 3) == 0, "nearest: d2 and idx must be 4-byte aligned");
    const int s = splits == 0 ? falnet_nearest_splits(nq, nr) : splits;
    FALNET_CHECK_ARG(s == 1 || (workspace && ((uintptr_t)workspace & 7) == 0), "nearest: %d splits need an 8-byte aligned workspace", s);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = (uint32_t)nq, m = (uint32_t)nr;
    const dim3 threads(NN_THREADS);
    const unsigned qblocks = (unsigned)((nq + NN_BLOCK - 1) / NN_BLOCK), qgrid = (unsigned)((nq + NN_THREADS - 1) / NN_THREADS);
    const int64_t tiles = nn_tiles(nr);
    const uint32_t tps = (uint32_t)((tiles + s - 1) / s);  // whole tiles per split; 0 when nr = 0: every range is empty
    const float4* q4 = reinterpret_cast<const float4*>(query);
    const float4* r4 = reinterpret_cast<const float4*>(ref);
    if (s == 1) {
        hipLaunchKernelGGL(nn_kernel<false>, dim3(qblocks, 1), threads, 0, st, q4, n, r4, m, tps, d2, idx, (unsigned long long*)nullptr);
    } else {
        unsigned long long* keys = static_cast<unsigned long long*>(workspace);
        hipLaunchKernelGGL(nn_fill_kernel, dim3(qgrid), threads, 0, st, keys, n);
        hipLaunchKernelGGL(nn_kernel<true>, dim3(qblocks, (unsigned)s), threads, 0, st, q4, n, r4, m, tps, (float*)nullptr, (int32_t*)nullptr, keys);
        hipLaunchKernelGGL(nn_finish_kernel, dim3(qgrid), threads, 0, st, (const unsigned long long*)keys, n, d2, idx);
    }
    FALNET_RETURN_LAUNCH();
}

// ---- the sums of a frame ----------------------------------------------------------------------------------------------------------------------
struct CloudArgs {  // by value in the kernel arguments
    const float* d2[2];
    uint32_t n[2];
    double tau2[CE_MAX_K];
    int K;
};

// partial[(direction * CE_BLOCKS + block) * CE_COLS + column]
__global__ __launch_bounds__(CE_THREADS) void ce_partial_kernel(CloudArgs a, double* __restrict__ partial) {
    __shared__ double red[CE_THREADS / 64][CE_COLS];
    const int dir = blockIdx.y;
    const float* __restrict__ d2 = a.d2[dir];
    const uint32_t n = a.n[dir];
    double s_sqrt = 0.0, s_sq = 0.0;
    uint32_t c_n = 0, c_hit[CE_MAX_K];
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) c_hit[k] = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * CE_THREADS + threadIdx.x; i < n; i += (uint64_t)CE_BLOCKS * CE_THREADS) {
        const float f = d2[i];
        if (!isfinite(f)) continue;  // left out of everything
        const double v = (double)f;
        c_n += 1;
        s_sqrt += sqrt(v);
        s_sq += v;
#pragma unroll
        for (int k = 0; k < CE_MAX_K; ++k) c_hit[k] += (k < a.K && v <= a.tau2[k]) ? 1u : 0u;
    }
    double col[CE_COLS];
    col[0] = wave_sum_f64((double)c_n), col[1] = wave_sum_f64(s_sqrt), col[2] = wave_sum_f64(s_sq);  // a count is an exact double: < 2^31
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) col[3 + k] = wave_sum_f64((double)c_hit[k]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < CE_COLS; ++c) red[w][c] = col[c];
    }
    __syncthreads();
    if (threadIdx.x < CE_COLS) {
        double t = 0.0;
        for (int i = 0; i < CE_THREADS / 64; ++i) t += red[i][threadIdx.x];
        partial[((size_t)dir * CE_BLOCKS + blockIdx.x) * CE_COLS + threadIdx.x] = t;
    }
}

// thread (direction, column): the partials in block order -> the row (FALNET_CLOUD_* of the header)
__global__ __launch_bounds__(64) void ce_final_kernel(const double* __restrict__ partial, double* __restrict__ row) {
    const int t = threadIdx.x;
    if (t >= 2 * CE_COLS) return;
    const int dir = t / CE_COLS, c = t - dir * CE_COLS;
    double s = 0.0;
    for (int b = 0; b < CE_BLOCKS; ++b) s += partial[((size_t)dir * CE_BLOCKS + b) * CE_COLS + c];
    const int at = c < 3 ? (dir == 0 ? FALNET_CLOUD_N_PRED : FALNET_CLOUD_N_GT) + c : (dir == 0 ? FALNET_CLOUD_HIT_PRED : FALNET_CLOUD_HIT_GT) + (c - 3);
    row[at] = s;
}

extern "C" int64_t falnet_cloud_errors_workspace_bytes(void) { return (int64_t)2 * CE_BLOCKS * CE_COLS * (int64_t)sizeof(double); }

extern "C" int falnet_cloud_errors(const float* d2_pred, int64_t n_pred, const float* d2_gt, int64_t n_gt, const double* tau2, int K, double* row,
                                   void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(nn_shape_ok(n_pred, n_gt), "cloud_errors: n_pred = %lld and n_gt = %lld must lie in [0, 2^31)", (long long)n_pred, (long long)n_gt);
    FALNET_CHECK_ARG(K >= 0 && K <= CE_MAX_K, "cloud_errors: %d thresholds (0 to %d)", K, CE_MAX_K);
    FALNET_CHECK_ARG(K == 0 || tau2, "cloud_errors: null thresholds with K = %d", K);
    FALNET_CHECK_ARG((n_pred == 0 || d2_pred) && (n_gt == 0 || d2_gt), "cloud_errors: null d2 array");
    FALNET_CHECK_ARG(row && workspace, "cloud_errors: null row or workspace");
    FALNET_CHECK_ARG((((uintptr_t)row | (uintptr_t)workspace) & 7) == 0, "cloud_errors: row and workspace must be 8-byte aligned");
    FALNET_CHECK_ARG((((uintptr_t)d2_pred | (uintptr_t)d2_gt) & 3) == 0, "cloud_errors: the d2 arrays must be 4-byte aligned");
    CloudArgs a;
    for (int k = 0; k < CE_MAX_K; ++k) {
        FALNET_CHECK_ARG(k >= K || tau2[k] >= 0.0, "cloud_errors: tau2[%d] = %g must be >= 0 (a NaN is refused)", k, tau2[k]);
        a.tau2[k] = k < K ? tau2[k] : 0.0;
    }
    a.d2[0] = d2_pred, a.d2[1] = d2_gt, a.n[0] = (uint32_t)n_pred, a.n[1] = (uint32_t)n_gt, a.K = K;
    hipStream_t st = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(ce_partial_kernel, dim3(CE_BLOCKS, 2), dim3(CE_THREADS), 0, st, a, partial);
    hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(64), 0, st, (const double*)partial, row);
    FALNET_RETURN_LAUNCH();
}
