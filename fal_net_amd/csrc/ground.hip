// The ground plane of a scan: plane hypotheses from point triples (falnet_ground_hypotheses), their consensus over the scan
// (falnet_ground_consensus), the moments of a plane's inliers (falnet_ground_moments), heights above a plane (falnet_ground_heights) and the
// ordered split of a scan by height (falnet_ground_split).  include/falnet_hip.h; the numpy restatement is tests/_ground_ref.py.
//
// A record is 4 consecutive f32 x, y, z, . -- the 16-byte point of falnet_velo_unproject; the fourth value is ignored.  A plane is held in height
// form z = p x + q y + r, and every residual is the vertical one:
//   e = z - ((p x + q y) + r)
// every operation rounded to f32 in this order, no fused multiply-add: the file is compiled with -ffp-contract=off.  A point is an inlier of a plane
// iff |e| <= tol in f32; a NaN anywhere makes the comparison false.  No square root is taken anywhere a result decides an integer.
//
//   gr_hyp_kernel        thread h forms the plane through the points of triple h in f64 in the stated order:
//                          u = P1 - P0, v = P2 - P0;  nx = uy vz - uz vy, ny = uz vx - ux vz, nz = ux vy - uy vx
//                          p = -(nx / nz), q = -(ny / nz), r = z0 - (p x0 + q y0)
//                        valid iff p, q, r are finite and (p p + q q) <= tan2_max (and every index lies in [0, n)); stored (f32 p, f32 q, f32 r, 1.0f),
//                        or four +0.  f64 + - x / are IEEE: the host reproduces the planes bit for bit.
//   gr_consensus_kernel  workgroup (bx, s) owns the GR_BLOCK hypotheses from bx GR_BLOCK on -- GR_HPT per thread, in registers -- and walks the point
//                        range of split s through LDS tiles of GR_TILE records.  Every lane reads the same LDS address per point (identical addresses
//                        broadcast: no bank conflict) and adds to private integer counters.  One split: the counts are stored plainly.  S > 1: one
//                        integer atomicAdd per hypothesis and workgroup on the u32 counters of the workspace, which gr_fill_kernel has zeroed.
//   gr_select_kernel     one workgroup: counts -> the output (an invalid hypothesis: 0), the maximum of the 64-bit key (count << 32) | (0xffffffff - h)
//                        -- the largest count, ties to the smallest index: the key idiom of lidar.hip and nearest.hip -- and the winner's record
//   gr_moments_kernel    workgroup b of a FIXED grid sums over the inliers of one plane -- the winner's record in device memory, or the caller's --
//                        n, x, y, z, xx, xy, yy, xz, yz, zz in f64, products formed in f64 from the f32 coordinates: a thread's stride in order,
//                        wave_sum_f64, the four waves in order (the shape of ce_partial_kernel)
//   gr_moments_final_kernel  one thread per column adds the GM_BLOCKS partials in block order and writes the row (the shape of ce_final_kernel)
//   gr_heights_kernel    h[i] = (z - ((p x + q y) + r)) cz in the same f32 chain
//   gr_split_count_kernel / gr_split_scatter_kernel   the ordered compaction of ordered.h around falnet_offset_scan: keep (lo < h <= hi) == inside
// No workgroup waits for another, every loop is bounded by n or H, the only atomics are integer ones on vector memory, nothing is cooperative, no
// inline assembly.  Counts are integers: any decomposition of the point range gives the same result.  Two calls give the same bits.
// Not on the training step's path, not replayable, and not part of the autotune key (ops.py: _TUNE_SOURCES).
#include <math.h>
#include "common.h"
#include "ordered.h"

#define GR_THREADS 256
#define GR_HPT 2
#define GR_BLOCK (GR_THREADS * GR_HPT)  // hypotheses per workgroup (ground.HYP_BLOCK)
#define GR_TILE 1024                    // point records per LDS tile (ground.POINT_TILE)
#define GR_TARGET_WGS 512               // the default split rule fills this many workgroups (ground.TARGET_WORKGROUPS)
#define GR_MAX_SPLITS 1024
#define GR_MAX_H FALNET_GROUND_MAX_HYPOTHESES

#define GM_THREADS 256
#define GM_BLOCKS 64
#define GM_COLS 10  // n, x, y, z, xx, xy, yy, xz, yz, zz

static_assert(GR_TILE % GR_THREADS == 0, "a tile is staged in whole rounds of the workgroup");
static_assert(FALNET_GROUND_ROW == GM_COLS + 6, "the row holds the sums, then index, count, p, q, r, status");
static_assert(GM_THREADS >= FALNET_GROUND_ROW, "one thread per column of the row");

// the vertical residual of the header, in f32, in the stated order
__device__ __forceinline__ float gr_residual(float x, float y, float z, float p, float q, float r) { return z - ((p * x + q * y) + r); }

// ---- hypotheses -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GR_THREADS) void gr_hyp_kernel(const float4* __restrict__ pts, uint32_t n, const int32_t* __restrict__ triples, uint32_t H,
                                                            double tan2_max, float4* __restrict__ planes) {
    const uint32_t h = blockIdx.x * GR_THREADS + threadIdx.x;
    if (h >= H) return;
    const int32_t i0 = triples[3 * h], i1 = triples[3 * h + 1], i2 = triples[3 * h + 2];
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i0 >= 0 && i1 >= 0 && i2 >= 0 && (uint32_t)i0 < n && (uint32_t)i1 < n && (uint32_t)i2 < n) {  // an index outside the scan: invalid, nothing read
        const float4 a = pts[i0], b = pts[i1], c = pts[i2];
        const double x0 = (double)a.x, y0 = (double)a.y, z0 = (double)a.z;
        const double ux = (double)b.x - x0, uy = (double)b.y - y0, uz = (double)b.z - z0;
        const double vx = (double)c.x - x0, vy = (double)c.y - y0, vz = (double)c.z - z0;
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double p = -(nx / nz), q = -(ny / nz);
        const double r = z0 - (p * x0 + q * y0);
        if (isfinite(p) && isfinite(q) && isfinite(r) && (p * p + q * q) <= tan2_max) out = make_float4((float)p, (float)q, (float)r, 1.0f);
    }
    planes[h] = out;
}

// ---- consensus --------------------------------------------------------------------------------------------------------------------------------
// points [i_begin, i_end) of split blockIdx.y; SPLIT: the counts go to acc[] by atomicAdd, else to counts[]
template <bool SPLIT>
__global__ __launch_bounds__(GR_THREADS) void gr_consensus_kernel(const float4* __restrict__ pts, uint32_t n, const float4* __restrict__ planes, uint32_t H,
                                                                  float tol, uint32_t tiles_per_split, uint32_t* __restrict__ counts,
                                                                  uint32_t* __restrict__ acc) {
    __shared__ float4 tile[GR_TILE];
    const uint32_t h0 = blockIdx.x * GR_BLOCK + threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.y * tiles_per_split * GR_TILE;
    const uint64_t last = first + (uint64_t)tiles_per_split * GR_TILE;
    const uint32_t i_begin = first < n ? (uint32_t)first : n, i_end = last < n ? (uint32_t)last : n;
    if (i_begin >= i_end && SPLIT) return;  // an empty split adds nothing (the whole workgroup leaves: no barrier is passed)
    float p[GR_HPT], q[GR_HPT], r[GR_HPT];
    uint32_t c[GR_HPT];
    bool valid[GR_HPT];
#pragma unroll
    for (int k = 0; k < GR_HPT; ++k) {
        const uint32_t h = h0 + k * GR_THREADS;
        const float4 v = h < H ? planes[h] : make_float4(0.f, 0.f, 0.f, 0.f);
        p[k] = v.x, q[k] = v.y, r[k] = v.z, valid[k] = h < H && v.w != 0.f, c[k] = 0;
    }
    for (uint32_t base = i_begin; base < i_end; base += GR_TILE) {  // base + GR_TILE <= 2^31 + GR_TILE: no wrap
        const uint32_t cnt = i_end - base < GR_TILE ? i_end - base : GR_TILE;
        __syncthreads();  // the previous tile has been read
#pragma unroll
        for (int k = 0; k < GR_TILE / GR_THREADS; ++k) {
            const uint32_t j = k * GR_THREADS + threadIdx.x;
            if (j < cnt) tile[j] = pts[base + j];  // base + j < i_end <= n
        }
        __syncthreads();
#pragma unroll 4
        for (uint32_t j = 0; j < cnt; ++j) {
            const float4 v = tile[j];  // one address for the whole wave
#pragma unroll
            for (int k = 0; k < GR_HPT; ++k) c[k] += fabsf(gr_residual(v.x, v.y, v.z, p[k], q[k], r[k])) <= tol ? 1u : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < GR_HPT; ++k) {
        const uint32_t h = h0 + k * GR_THREADS;
        if (h >= H) continue;
        const uint32_t v = valid[k] ? c[k] : 0u;
        if (SPLIT) {
            if (v) atomicAdd(&acc[h], v);  // h < H: inside the workspace
        } else {
            counts[h] = v;
        }
    }
}

__global__ __launch_bounds__(GR_THREADS) void gr_fill_kernel(uint32_t* __restrict__ acc, uint32_t H) {
    const uint32_t h = blockIdx.x * GR_THREADS + threadIdx.x;
    if (h < H) acc[h] = 0u;
}

// best: FALNET_GROUND_BEST_WORDS 32-bit words: key low, key high, status, index, bits(p), bits(q), bits(r), count
__global__ __launch_bounds__(GR_THREADS) void gr_select_kernel(const uint32_t* src, const float4* __restrict__ planes, uint32_t H, uint32_t* counts,
                                                               uint32_t* __restrict__ best) {  // src may BE counts (one split)
    __shared__ unsigned long long keys[GR_THREADS];
    unsigned long long k = 0ull;  // below every key: index 0xffffffff is no hypothesis
    for (uint32_t h = threadIdx.x; h < H; h += GR_THREADS) {
        const uint32_t c = src[h];
        if (src != counts) counts[h] = c;
        const unsigned long long key = ((unsigned long long)c << 32) | (unsigned long long)(0xffffffffu - h);
        k = key > k ? key : k;
    }
    keys[threadIdx.x] = k;
    __syncthreads();
    for (int o = GR_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const unsigned long long a = keys[threadIdx.x], b = keys[threadIdx.x + o];
            keys[threadIdx.x] = a > b ? a : b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long key = keys[0];
        const uint32_t c = (uint32_t)(key >> 32), h = 0xffffffffu - (uint32_t)key;
        const bool found = c >= 3u && h < H;
        const float4 w = found ? planes[h] : make_float4(0.f, 0.f, 0.f, 0.f);
        best[0] = (uint32_t)key, best[1] = (uint32_t)(key >> 32);
        best[2] = found ? 1u : 0u, best[3] = found ? h : 0xffffffffu;
        best[4] = __float_as_uint(w.x), best[5] = __float_as_uint(w.y), best[6] = __float_as_uint(w.z), best[7] = c;
    }
}

static inline int64_t gr_tiles(int64_t n) { return (n + GR_TILE - 1) / GR_TILE; }
static inline bool gr_shape_ok(int64_t n, int64_t H) { return n >= 3 && n < ((int64_t)1 << 31) && H >= 1 && H <= GR_MAX_H; }

// the default split rule: enough splits of the point range that ceil(H / GR_BLOCK) * S reaches GR_TARGET_WGS workgroups, at most one split per tile
extern "C" int falnet_ground_splits(int64_t n, int64_t H) {
    if (!gr_shape_ok(n, H)) return 0;
    const int64_t blocks = (H + GR_BLOCK - 1) / GR_BLOCK, tiles = gr_tiles(n);
    int64_t s = (GR_TARGET_WGS + blocks - 1) / blocks;
    if (s > tiles) s = tiles;
    if (s > GR_MAX_SPLITS) s = GR_MAX_SPLITS;
    return (int)(s < 1 ? 1 : s);
}

extern "C" int64_t falnet_ground_consensus_workspace_bytes(int64_t n, int64_t H, int splits) {
    if (!gr_shape_ok(n, H) || splits < 0 || splits > GR_MAX_SPLITS) return 0;
    const int s = splits == 0 ? falnet_ground_splits(n, H) : splits;
    return s > 1 ? ((H * (int64_t)sizeof(uint32_t) + 7) / 8) * 8 : 0;
}

extern "C" int falnet_ground_hypotheses(const float* points, int64_t n, const int32_t* triples, int64_t H, double tan2_max, float* planes, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(gr_shape_ok(n, H), "ground_hypotheses: n = %lld must lie in [3, 2^31) and H = %lld in [1, %d]", (long long)n, (long long)H, GR_MAX_H);
    FALNET_CHECK_ARG(points && triples && planes, "ground_hypotheses: null points, triples or planes");
    FALNET_CHECK_ARG((((uintptr_t)points | (uintptr_t)planes) & 15) == 0, "ground_hypotheses: points and planes must be 16-byte aligned (one record is one 16-byte access)");
    FALNET_CHECK_ARG(((uintptr_t)triples & 3) == 0, "ground_hypotheses: triples must be 4-byte aligned");
    FALNET_CHECK_ARG(tan2_max >= 0.0 && isfinite(tan2_max), "ground_hypotheses: tan2_max = %g must be finite and >= 0", tan2_max);
    hipLaunchKernelGGL(gr_hyp_kernel, dim3((unsigned)((H + GR_THREADS - 1) / GR_THREADS)), dim3(GR_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(points), (uint32_t)n, triples, (uint32_t)H, tan2_max, reinterpret_cast<float4*>(planes));
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_ground_consensus(const float* points, int64_t n, const float* planes, int64_t H, float tol, int splits, uint32_t* counts,
                                       uint32_t* best, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(gr_shape_ok(n, H), "ground_consensus: n = %lld must lie in [3, 2^31) and H = %lld in [1, %d]", (long long)n, (long long)H, GR_MAX_H);
    FALNET_CHECK_ARG(splits >= 0 && splits <= GR_MAX_SPLITS, "ground_consensus: splits %d outside [0, %d] (0: the library's choice)", splits, GR_MAX_SPLITS);
    FALNET_CHECK_ARG(points && planes && counts && best, "ground_consensus: null points, planes, counts or best");
    FALNET_CHECK_ARG((((uintptr_t)points | (uintptr_t)planes) & 15) == 0, "ground_consensus: points and planes must be 16-byte aligned (one record is one 16-byte load)");
    FALNET_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)best & 7) == 0, "ground_consensus: counts must be 4-byte and best 8-byte aligned");
    FALNET_CHECK_ARG(tol >= 0.f && isfinite(tol), "ground_consensus: tol = %g must be finite and >= 0", (double)tol);
    const int s = splits == 0 ? falnet_ground_splits(n, H) : splits;
    FALNET_CHECK_ARG(s == 1 || (workspace && ((uintptr_t)workspace & 7) == 0), "ground_consensus: %d splits need an 8-byte aligned workspace", s);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t np = (uint32_t)n, nh = (uint32_t)H;
    const dim3 threads(GR_THREADS);
    const unsigned hblocks = (unsigned)((H + GR_BLOCK - 1) / GR_BLOCK), hgrid = (unsigned)((H + GR_THREADS - 1) / GR_THREADS);
    const uint32_t tps = (uint32_t)((gr_tiles(n) + s - 1) / s);  // whole tiles per split
    const float4* p4 = reinterpret_cast<const float4*>(points);
    const float4* h4 = reinterpret_cast<const float4*>(planes);
    if (s == 1) {
        hipLaunchKernelGGL(gr_consensus_kernel<false>, dim3(hblocks, 1), threads, 0, st, p4, np, h4, nh, tol, tps, counts, (uint32_t*)nullptr);
        hipLaunchKernelGGL(gr_select_kernel, dim3(1), threads, 0, st, (const uint32_t*)counts, h4, nh, counts, best);
    } else {
        uint32_t* acc = static_cast<uint32_t*>(workspace);
        hipLaunchKernelGGL(gr_fill_kernel, dim3(hgrid), threads, 0, st, acc, nh);
        hipLaunchKernelGGL(gr_consensus_kernel<true>, dim3(hblocks, (unsigned)s), threads, 0, st, p4, np, h4, nh, tol, tps, (uint32_t*)nullptr, acc);
        hipLaunchKernelGGL(gr_select_kernel, dim3(1), threads, 0, st, (const uint32_t*)acc, h4, nh, counts, best);
    }
    FALNET_RETURN_LAUNCH();
}

// ---- the moments of a plane's inliers ---------------------------------------------------------------------------------------------------------
struct GroundPlaneArg {  // by value in the kernel arguments: the caller's plane, read when `best` is null
    float p, q, r;
    int32_t index;
    uint32_t count;
};

struct GroundPlaneRead {
    float p, q, r;
    double index, count, status;
};

__device__ __forceinline__ GroundPlaneRead gr_plane(const uint32_t* __restrict__ best, const GroundPlaneArg& a) {
    GroundPlaneRead o;
    if (best) {
        o.status = (double)best[2], o.index = (double)(int32_t)best[3], o.count = (double)best[7];
        o.p = __uint_as_float(best[4]), o.q = __uint_as_float(best[5]), o.r = __uint_as_float(best[6]);
    } else {
        o.status = 1.0, o.index = (double)a.index, o.count = (double)a.count, o.p = a.p, o.q = a.q, o.r = a.r;
    }
    return o;
}

// partial[block * GM_COLS + column]
__global__ __launch_bounds__(GM_THREADS) void gr_moments_kernel(const float4* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ best,
                                                                GroundPlaneArg arg, float tol, double* __restrict__ partial) {
    __shared__ double red[GM_THREADS / 64][GM_COLS];
    const GroundPlaneRead pl = gr_plane(best, arg);
    const bool on = pl.status != 0.0;  // "no plane": nothing is an inlier
    double s[GM_COLS];
#pragma unroll
    for (int c = 0; c < GM_COLS; ++c) s[c] = 0.0;
    uint32_t cn = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * GM_THREADS + threadIdx.x; i < n && on; i += (uint64_t)GM_BLOCKS * GM_THREADS) {
        const float4 v = pts[i];
        if (!(fabsf(gr_residual(v.x, v.y, v.z, pl.p, pl.q, pl.r)) <= tol)) continue;
        const double x = (double)v.x, y = (double)v.y, z = (double)v.z;
        cn += 1;
        s[1] += x, s[2] += y, s[3] += z;
        s[4] += x * x, s[5] += x * y, s[6] += y * y, s[7] += x * z, s[8] += y * z, s[9] += z * z;
    }
    s[0] = (double)cn;  // a count is an exact double: < 2^31
#pragma unroll
    for (int c = 0; c < GM_COLS; ++c) s[c] = wave_sum_f64(s[c]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < GM_COLS; ++c) red[w][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < GM_COLS) {
        double t = 0.0;
        for (int i = 0; i < GM_THREADS / 64; ++i) t += red[i][threadIdx.x];
        partial[(size_t)blockIdx.x * GM_COLS + threadIdx.x] = t;
    }
}

// thread c: the partials of column c in block order -> the row; the six columns behind the sums carry the plane
__global__ __launch_bounds__(64) void gr_moments_final_kernel(const double* __restrict__ partial, const uint32_t* __restrict__ best, GroundPlaneArg arg,
                                                              double* __restrict__ row) {
    const int c = threadIdx.x;
    if (c >= FALNET_GROUND_ROW) return;
    if (c < GM_COLS) {
        double s = 0.0;
        for (int b = 0; b < GM_BLOCKS; ++b) s += partial[(size_t)b * GM_COLS + c];
        row[c] = s;
        return;
    }
    const GroundPlaneRead pl = gr_plane(best, arg);
    row[c] = c == FALNET_GROUND_INDEX ? pl.index : c == FALNET_GROUND_COUNT ? pl.count : c == FALNET_GROUND_P ? (double)pl.p
           : c == FALNET_GROUND_Q ? (double)pl.q : c == FALNET_GROUND_R ? (double)pl.r : pl.status;
}

extern "C" int64_t falnet_ground_moments_workspace_bytes(void) { return (int64_t)GM_BLOCKS * GM_COLS * (int64_t)sizeof(double); }

extern "C" int falnet_ground_moments(const float* points, int64_t n, const uint32_t* best, float p, float q, float r, int32_t index, uint32_t count,
                                     float tol, double* row, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(n >= 3 && n < ((int64_t)1 << 31), "ground_moments: n = %lld must lie in [3, 2^31)", (long long)n);
    FALNET_CHECK_ARG(points && row && workspace, "ground_moments: null points, row or workspace");
    FALNET_CHECK_ARG(((uintptr_t)points & 15) == 0, "ground_moments: points must be 16-byte aligned (one record is one 16-byte load)");
    FALNET_CHECK_ARG((((uintptr_t)row | (uintptr_t)workspace | (uintptr_t)best) & 7) == 0, "ground_moments: row, workspace and best must be 8-byte aligned");
    FALNET_CHECK_ARG(tol >= 0.f && isfinite(tol), "ground_moments: tol = %g must be finite and >= 0", (double)tol);
    FALNET_CHECK_ARG(best || (isfinite(p) && isfinite(q) && isfinite(r)), "ground_moments: the plane (%g, %g, %g) is not finite", (double)p, (double)q, (double)r);
    GroundPlaneArg a;
    a.p = p, a.q = q, a.r = r, a.index = index, a.count = count;
    hipStream_t st = (hipStream_t)stream;
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(gr_moments_kernel, dim3(GM_BLOCKS), dim3(GM_THREADS), 0, st, reinterpret_cast<const float4*>(points), (uint32_t)n, best, a, tol, partial);
    hipLaunchKernelGGL(gr_moments_final_kernel, dim3(1), dim3(64), 0, st, (const double*)partial, best, a, row);
    FALNET_RETURN_LAUNCH();
}

// ---- heights and the split --------------------------------------------------------------------------------------------------------------------
struct GroundHeightArgs {
    float p, q, r, cz;
};

__device__ __forceinline__ float gr_height(const float4 v, const GroundHeightArgs& a) { return gr_residual(v.x, v.y, v.z, a.p, a.q, a.r) * a.cz; }

__global__ __launch_bounds__(GR_THREADS) void gr_heights_kernel(const float4* __restrict__ pts, uint32_t n, GroundHeightArgs a, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * GR_THREADS + threadIdx.x;
    if (i < n) out[i] = gr_height(pts[i], a);
}

// record i is kept iff (lo < h <= hi) == inside; a NaN height is outside every range
__device__ __forceinline__ bool gr_keep(const float4* __restrict__ pts, uint32_t i, uint32_t n, const GroundHeightArgs& a, float lo, float hi, bool inside,
                                        float4& rec) {
    if (i >= n) return false;
    rec = pts[i];
    const float h = gr_height(rec, a);
    return (lo < h && h <= hi) == inside;
}

__global__ __launch_bounds__(ORD_THREADS) void gr_split_count_kernel(const float4* __restrict__ pts, uint32_t n, GroundHeightArgs a, float lo, float hi,
                                                                     bool inside, int64_t* __restrict__ counts) {
    __shared__ int wsum[ORD_THREADS / 64];
    const uint32_t base = blockIdx.x * ORD_TILE;  // blockIdx.x < ceil(n / ORD_TILE): base < 2^31, base + ORD_TILE < 2^32
    int c = 0;
    float4 rec;
#pragma unroll
    for (int r = 0; r < ORD_ROUNDS; ++r) c += gr_keep(pts, base + r * ORD_THREADS + threadIdx.x, n, a, lo, hi, inside, rec) ? 1 : 0;
    const int total = block_count(c, wsum);
    if (threadIdx.x == 0) counts[blockIdx.x] = (int64_t)total;
}

__global__ __launch_bounds__(ORD_THREADS) void gr_split_scatter_kernel(const float4* __restrict__ pts, uint32_t n, GroundHeightArgs a, float lo, float hi,
                                                                       bool inside, const int64_t* __restrict__ offsets, float4* __restrict__ out,
                                                                       int64_t capacity) {
    __shared__ int wsum[ORD_THREADS / 64];
    const uint32_t base = blockIdx.x * ORD_TILE;
    int64_t pos = offsets[blockIdx.x];
    for (int r = 0; r < ORD_ROUNDS; ++r) {
        float4 rec;
        const bool keep = gr_keep(pts, base + r * ORD_THREADS + threadIdx.x, n, a, lo, hi, inside, rec);
        int total;
        const int rank = block_rank(keep, wsum, total);
        if (keep) {
            const int64_t j = pos + rank;
            if (j < capacity) out[j] = rec;
        }
        pos += total;
    }
}

static inline bool gr_plane_ok(float p, float q, float r, float cz) { return isfinite(p) && isfinite(q) && isfinite(r) && isfinite(cz); }
static inline int64_t gr_split_blocks(int64_t n) { return (n + ORD_TILE - 1) / ORD_TILE; }

extern "C" int falnet_ground_heights(const float* points, int64_t n, float p, float q, float r, float cz, float* heights, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "ground_heights: n = %lld must lie in [0, 2^31)", (long long)n);
    FALNET_CHECK_ARG(gr_plane_ok(p, q, r, cz), "ground_heights: the plane (%g, %g, %g) or cz = %g is not finite", (double)p, (double)q, (double)r, (double)cz);
    if (n == 0) return 0;  // nothing to write, nothing launched
    FALNET_CHECK_ARG(points && heights, "ground_heights: null points or heights");
    FALNET_CHECK_ARG(((uintptr_t)points & 15) == 0 && ((uintptr_t)heights & 3) == 0, "ground_heights: points must be 16-byte and heights 4-byte aligned");
    GroundHeightArgs a;
    a.p = p, a.q = q, a.r = r, a.cz = cz;
    hipLaunchKernelGGL(gr_heights_kernel, dim3((unsigned)((n + GR_THREADS - 1) / GR_THREADS)), dim3(GR_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(points), (uint32_t)n, a, heights);
    FALNET_RETURN_LAUNCH();
}

extern "C" int64_t falnet_ground_split_workspace_bytes(int64_t n) {
    return n > 0 && n < ((int64_t)1 << 31) ? gr_split_blocks(n) * (int64_t)sizeof(int64_t) : 0;
}

extern "C" int falnet_ground_split(const float* points, int64_t n, float p, float q, float r, float cz, float lo, float hi, int inside, float* out_points,
                                   int64_t capacity, int64_t* count_dev, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "ground_split: n = %lld must lie in [0, 2^31)", (long long)n);
    FALNET_CHECK_ARG(gr_plane_ok(p, q, r, cz), "ground_split: the plane (%g, %g, %g) or cz = %g is not finite", (double)p, (double)q, (double)r, (double)cz);
    FALNET_CHECK_ARG(!isnan(lo) && !isnan(hi), "ground_split: lo or hi is NaN");
    FALNET_CHECK_ARG(capacity >= 0, "ground_split: capacity %lld is negative", (long long)capacity);
    if (n == 0) return 0;  // nothing to keep, nothing launched: the count is the caller's 0
    FALNET_CHECK_ARG(points && count_dev && workspace, "ground_split: null points, count or workspace");
    FALNET_CHECK_ARG(capacity == 0 || out_points, "ground_split: null output with capacity %lld", (long long)capacity);
    FALNET_CHECK_ARG((((uintptr_t)points | (uintptr_t)out_points) & 15) == 0, "ground_split: points and the output must be 16-byte aligned (one record is one 16-byte access)");
    FALNET_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)count_dev) & 7) == 0, "ground_split: workspace and count must be 8-byte aligned");
    GroundHeightArgs a;
    a.p = p, a.q = q, a.r = r, a.cz = cz;
    hipStream_t st = (hipStream_t)stream;
    int64_t* counts = static_cast<int64_t*>(workspace);
    const int64_t nb = gr_split_blocks(n);
    const float4* p4 = reinterpret_cast<const float4*>(points);
    hipLaunchKernelGGL(gr_split_count_kernel, dim3((unsigned)nb), dim3(ORD_THREADS), 0, st, p4, (uint32_t)n, a, lo, hi, inside != 0, counts);
    falnet_offset_scan(counts, nb, count_dev, st);
    hipLaunchKernelGGL(gr_split_scatter_kernel, dim3((unsigned)nb), dim3(ORD_THREADS), 0, st, p4, (uint32_t)n, a, lo, hi, inside != 0, (const int64_t*)counts,
                       reinterpret_cast<float4*>(out_points), capacity);
    FALNET_RETURN_LAUNCH();
}
