// Sparsification curves of one frame on the device: the pixels that count for the depth errors are removed in order of
// decreasing predicted uncertainty -- one ordering per score map -- and in order of their true error -- one oracle ordering per metric -- and
// abs_rel, rms and d1 = 1 - a1 of the pixels that are left are written for `steps` cuts into one row of doubles.
//
//   1  sp_count_kernel     workgroup g counts the pixels of its SP_TILE consecutive region positions that depth_pair accepts     -> counts[g]
//   2  falnet_offset_scan  the offset scan of compact.hip: exclusive offsets in place                                             -> counts[g], *n
//   3  sp_scatter_kernel   the ordered compaction of ordered.h: counted pixel number k (region row-major order) gets its errors e_abs[k],
//                          e_sq[k], the flag t < 1.25 and one sort key per ordering, keys[s * N + k]
//   4  falnet_sort_u32     all orderings in one call over N = the region's size: the positions n .. N - 1, which hold no pixel, keep the key
//                          0xFFFFFFFF of the pre-fill, above every key a value can have, so the first n ranks are the counted pixels
//   5  sp_interval_kernel  workgroup (j, s) sums the errors of ordering s over the ranks r_j .. r_(j+1) - 1 that cut j + 1 removes beyond cut j
//   6  sp_finalize_kernel  thread s adds the interval sums from the last cut to the first and writes the curves
// The depth chain is depth_pair.h's, the one of metrics.hip, f64 in the host's order: this file is compiled with -ffp-contract=off.  Every sum
// has a fixed partition and a fixed order (a thread's stride, the shuffles of a wave, the four waves in order, the intervals in order): two calls
// give the same bits.  No floating-point atomics, no atomics at all.  The number of counted pixels never leaves the device.
#include "common.h"
#include "depth_pair.h"
#include "ordered.h"

#define SP_THREADS ORD_THREADS
#define SP_ROUNDS ORD_ROUNDS
#define SP_TILE ORD_TILE
#define SP_MAX_STEPS 100
#define SP_MAX_SCORES 4
#define SP_MAX_PIXELS (1ll << 24)

// the monotone image of an f32 (-0 below +0) with every NaN above everything, complemented: an ascending sort removes the most uncertain pixel
// first
__device__ __forceinline__ uint32_t sort_key(float x) { return ~(x != x ? 0xFFFFFFFFu : key_f32(x)); }

// ---- the numbering of the counted pixels ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void sp_count_kernel(DepthArgs a, uint32_t N, int64_t* __restrict__ counts) {
    __shared__ int wsum[SP_THREADS / 64];
    const uint32_t base = blockIdx.x * SP_TILE;
    int c = 0;
#pragma unroll
    for (int r = 0; r < SP_ROUNDS; ++r) {
        const uint32_t i = base + r * SP_THREADS + threadIdx.x;
        double g, p;
        size_t idx;
        c += i < N && depth_pair(a, i, g, p, idx) ? 1 : 0;
    }
    const int total = block_count(c, wsum);
    if (threadIdx.x == 0) counts[blockIdx.x] = (int64_t)total;
}

struct SpBuffers {
    double* e_abs;   // [N] |g - p| / g of counted pixel k
    double* e_sq;    // [N] (g - p)^2
    uint8_t* lt;     // [N] t < 1.25
    uint32_t* keys;  // [(scores.n + 3) * N], pre-filled with 0xFFFFFFFF
};

__global__ __launch_bounds__(SP_THREADS) void sp_scatter_kernel(DepthArgs a, uint32_t N, const double* __restrict__ scale, double min_d, double max_d,
                                                                falnet_scores_t sc, const int64_t* __restrict__ counts, SpBuffers o) {
    __shared__ int wsum[SP_THREADS / 64];
    const uint32_t base = blockIdx.x * SP_TILE;
    const bool scaled = scale != nullptr;
    const double factor = scaled ? scale[0] : 1.0;
    uint32_t pos = (uint32_t)counts[blockIdx.x];
    for (int r = 0; r < SP_ROUNDS; ++r) {
        const uint32_t i = base + r * SP_THREADS + threadIdx.x;
        double g = 1.0, p = 1.0;
        size_t idx = 0;
        const bool keep = i < N && depth_pair(a, i, g, p, idx);
        int total;
        const int rank = block_rank(keep, wsum, total);
        if (keep) {
            const uint32_t k = pos + rank;  // < n <= N
            const double t = depth_scale_clamp(g, p, scaled, factor, min_d, max_d);
            const double d = g - p;
            const double e_abs = fabs(d) / g, e_sq = d * d;
            o.e_abs[k] = e_abs;
            o.e_sq[k] = e_sq;
            o.lt[k] = t < 1.25 ? 1 : 0;
#pragma unroll
            for (int s = 0; s < SP_MAX_SCORES; ++s) {
                if (s < sc.n) {
                    const float x = sc.map[s][idx];
                    o.keys[(size_t)s * N + k] = sort_key(sc.sign[s] > 0 ? x : -x);
                }
            }
            uint32_t* ok = o.keys + (size_t)sc.n * N;
            ok[k] = sort_key((float)e_abs);
            ok[(size_t)N + k] = sort_key((float)e_sq);
            ok[2 * (size_t)N + k] = sort_key((float)t);
        }
        pos += total;
    }
}

// ---- the sums -----------------------------------------------------------------------------------------------------------------------------------
// cut j removes the first r_j = (j n) / S ranks
__device__ __forceinline__ uint32_t cut_rank(uint32_t j, uint32_t n, uint32_t S) { return (uint32_t)(((uint64_t)j * n) / S); }

// workgroup (j, s): the sums of ordering s over the ranks [r_j, r_(j+1)) -- the last interval ends at n -> partial[(s * S + j) * 3 + {abs, sq, count}].
// An oracle ordering sums its own metric only (the two other entries are written 0 and never read).
__global__ __launch_bounds__(SP_THREADS) void sp_interval_kernel(const uint32_t* __restrict__ perm, uint32_t N, const int64_t* __restrict__ total, int n_scores,
                                                                 uint32_t S, SpBuffers o, double* __restrict__ partial) {
    __shared__ double red[SP_THREADS / 64][3];
    const uint32_t n = (uint32_t)*total, j = blockIdx.x, s = blockIdx.y;
    const uint32_t r0 = cut_rank(j, n, S), r1 = j + 1 == S ? n : cut_rank(j + 1, n, S);
    const int own = (int)s - n_scores;  // < 0: a score ordering, all three sums; 0, 1, 2: the oracle of abs_rel, rms, d1
    const uint32_t* pm = perm + (size_t)s * N;
    double v0 = 0.0, v1 = 0.0;
    uint32_t c = 0;
    for (uint32_t r = r0 + threadIdx.x; r < r1; r += SP_THREADS) {
        const uint32_t k = pm[r];  // < n: the first n ranks of an ordering are the counted pixels
        if (own < 0 || own == 0) v0 += o.e_abs[k];
        if (own < 0 || own == 1) v1 += o.e_sq[k];
        if (own < 0 || own == 2) c += o.lt[k];
    }
    double v2 = (double)c;
    v0 = wave_sum_f64(v0), v1 = wave_sum_f64(v1), v2 = wave_sum_f64(v2);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w][0] = v0, red[w][1] = v1, red[w][2] = v2;
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int i = 0; i < SP_THREADS / 64; ++i) t += red[i][threadIdx.x];
        partial[((size_t)s * S + j) * 3 + threadIdx.x] = t;
    }
}

// thread s: ordering s from the last cut to the first, kept sum of cut j = kept sum of cut j + 1 + interval j.  row: n, then per score its abs_rel,
// rms and d1 curves, then the three oracle curves.  n = 0: 0 / 0 = NaN everywhere.
__global__ __launch_bounds__(64) void sp_finalize_kernel(const double* __restrict__ partial, const int64_t* __restrict__ total, int n_scores, uint32_t S,
                                                         double* __restrict__ row) {
    const uint32_t n = (uint32_t)*total;
    const int s = threadIdx.x, own = s - n_scores;
    if (s == 0) row[0] = (double)n;
    if (s >= n_scores + 3) return;
    double* abs_rel = row + 1 + (size_t)(own < 0 ? 3 * s : 3 * n_scores) * S;
    double *rms = abs_rel + S, *d1 = rms + S;
    double k0 = 0.0, k1 = 0.0, k2 = 0.0;
    for (int j = (int)S - 1; j >= 0; --j) {
        const double* q = partial + ((size_t)s * S + j) * 3;
        k0 += q[0], k1 += q[1], k2 += q[2];
        const double nj = (double)(n - cut_rank((uint32_t)j, n, S));
        if (own < 0 || own == 0) abs_rel[j] = k0 / nj;
        if (own < 0 || own == 1) rms[j] = sqrt(k1 / nj);
        if (own < 0 || own == 2) d1[j] = (nj - k2) / nj;
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------------
static inline int64_t up8(int64_t b) { return (b + 7) & ~(int64_t)7; }
static inline int64_t sp_tiles(int64_t N) { return (N + SP_TILE - 1) / SP_TILE; }

struct SpLayout {  // byte offsets into the workspace, sized for cap = H * W pixels whatever the mode
    int64_t counts, total, e_abs, e_sq, lt, keys, perm, partial, sort, bytes;
};

static SpLayout sp_layout(int64_t cap, int n_scores) {
    SpLayout l;
    const int64_t seg = n_scores + 3;
    int64_t at = 0;
    l.counts = at, at += sp_tiles(cap) * 8;
    l.total = at, at += 8;
    l.e_abs = at, at += cap * 8;
    l.e_sq = at, at += cap * 8;
    l.lt = at, at += up8(cap);
    l.keys = at, at += up8(seg * cap * 4);
    l.perm = at, at += up8(seg * cap * 4);
    l.partial = at, at += seg * SP_MAX_STEPS * 3 * 8;
    l.sort = at, at += falnet_sort_u32_workspace_bytes(cap, (int)seg);
    l.bytes = at;
    return l;
}

extern "C" int64_t falnet_sparsify_workspace_bytes(int H, int W, int n_scores) {
    if (H < 1 || W < 1 || (int64_t)H * W > SP_MAX_PIXELS || n_scores < 0 || n_scores > SP_MAX_SCORES) return 0;
    return sp_layout((int64_t)H * W, n_scores).bytes;
}

extern "C" int falnet_sparsify(const float* pred_disp, const float* gt, int H, int W, int mode, double fb, const double* scale, double min_d, double max_d,
                               falnet_scores_t scores, int steps, double* row, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    // the sort's cap first: the shared checks speak of the 2^31 pixels of the metrics
    FALNET_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W <= SP_MAX_PIXELS, "sparsify: frame %d x %d must hold between 1 and 2^24 pixels", H, W);
    DepthArgs a;
    if (depth_args(a, pred_disp, gt, H, W, mode, fb, max_d, "sparsify")) return -1;
    FALNET_CHECK_ARG(steps >= 2 && steps <= SP_MAX_STEPS, "sparsify: steps=%d outside [2, %d]", steps, SP_MAX_STEPS);
    FALNET_CHECK_ARG(scores.n >= 0 && scores.n <= SP_MAX_SCORES, "sparsify: %d scores (0 to %d)", scores.n, SP_MAX_SCORES);
    for (int s = 0; s < scores.n; ++s) {
        FALNET_CHECK_ARG(scores.map[s], "sparsify: score %d is a null map", s);
        FALNET_CHECK_ARG(scores.sign[s] == 1 || scores.sign[s] == -1, "sparsify: sign of score %d is %d (+1: larger is more uncertain, -1: more confident)", s,
                         scores.sign[s]);
    }
    FALNET_CHECK_ARG(row && workspace, "sparsify: null row or workspace");
    FALNET_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)row & 7) == 0 && ((uintptr_t)scale & 7) == 0,
                     "sparsify: workspace, row and scale must be 8-byte aligned");
    FALNET_CHECK_ARG(min_d > 0.0 && max_d >= min_d, "sparsify: need 0 < min_d <= max_d");
    FALNET_CHECK_ARG(mode != FALNET_DEPTH_MAKE3D || scale, "sparsify: make3d is always median-scaled (scale from falnet_depth_median_scale)");
    const int64_t N = (int64_t)a.rh * a.rw;
    const int seg = scores.n + 3;
    const SpLayout l = sp_layout((int64_t)H * W, scores.n);
    char* ws = static_cast<char*>(workspace);
    int64_t* counts = reinterpret_cast<int64_t*>(ws + l.counts);
    int64_t* total = reinterpret_cast<int64_t*>(ws + l.total);
    SpBuffers o;
    o.e_abs = reinterpret_cast<double*>(ws + l.e_abs), o.e_sq = reinterpret_cast<double*>(ws + l.e_sq);
    o.lt = reinterpret_cast<uint8_t*>(ws + l.lt), o.keys = reinterpret_cast<uint32_t*>(ws + l.keys);
    uint32_t* perm = reinterpret_cast<uint32_t*>(ws + l.perm);
    double* partial = reinterpret_cast<double*>(ws + l.partial);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(o.keys, 0xFF, (size_t)seg * N * 4, st);
    if (e != hipSuccess) {
        falnet_set_error("sparsify: filling the keys failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    const unsigned tiles = (unsigned)sp_tiles(N);
    hipLaunchKernelGGL(sp_count_kernel, dim3(tiles), dim3(SP_THREADS), 0, st, a, (uint32_t)N, counts);
    falnet_offset_scan(counts, (int64_t)tiles, total, st);
    hipLaunchKernelGGL(sp_scatter_kernel, dim3(tiles), dim3(SP_THREADS), 0, st, a, (uint32_t)N, scale, min_d, max_d, scores, (const int64_t*)counts, o);
    const int rc = falnet_sort_u32(o.keys, N, seg, perm, ws + l.sort, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(sp_interval_kernel, dim3((unsigned)steps, (unsigned)seg), dim3(SP_THREADS), 0, st, (const uint32_t*)perm, (uint32_t)N,
                       (const int64_t*)total, scores.n, (uint32_t)steps, o, partial);
    hipLaunchKernelGGL(sp_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)partial, (const int64_t*)total, scores.n, (uint32_t)steps, row);
    FALNET_RETURN_LAUNCH();
}
