// Pseudo-LiDAR: a predicted depth (or disparity) map back-projected into a Velodyne-format scan on the device -- the inverse of velo.hip.
// Per pixel (v, u) of the (H, W) f32 map, index p = v W + u (include/falnet_hip.h; the numpy restatement is tests/_lidar_ref.py):
//   1. fb > 0: the map is a disparity, valid when disp > 0, d = (float)(fb / (double)disp); fb == 0: the map is the depth d;
//   2. keep when d > min_depth && d <= max_depth (f32 compares: NaN and infinity fail);
//   3. with a score map, keep when score >= threshold (a NaN score fails);
//   4. f64: r_i = (Q[i][0] (u + 1) + Q[i][1] (v + 1)) + Q[i][2], X_i = d r_i - Q[i][3]; (x, y, z) = (float)X_i; keep when x > 0 && z <= max_height;
//   5. the record is x, y, z, intensity (the intensity map's value at the pixel, or the constant) as four f32: one point of a KITTI .bin file.
// Dense mode writes the kept records in pixel order; beam mode keeps, per (elevation, azimuth) bin, the record of the smallest 64-bit key
// (bits(d) << 32) | p -- nearest first, lowest pixel index on a tie -- and writes the winners in bin order.
// Three rules hold:
//   * every + - * / and sqrt of steps 1, 4 and of the bin search is a correctly rounded operation in exactly this order: the file is compiled
//     with -ffp-contract=off, so a point's record and its bin are the host's, bit for bit;
//   * positions are decided by indices alone: a count pass, the offset scan of compact.hip and a scatter pass that evaluates the same
//     predicate again (the ordered compaction of ordered.h), so the output order is the pixel (or bin) order and no intermediate record
//     array exists;
//   * the only atomic is an integer atomicMin on a u64 key, whose result does not depend on arrival order: no floating-point atomics, and the
//     output is bit-identical from run to run.
// The all-ones sentinel of the key table is no pixel's key: its upper half is the pattern of a NaN, and a kept d has passed step 2.
// Not on the training step's path, not replayable, and not part of the autotune key (ops.py: _TUNE_SOURCES).
#include <math.h>
#include "common.h"
#include "ordered.h"

#define LD_THREADS ORD_THREADS
#define LD_ROUNDS ORD_ROUNDS
#define LD_TILE ORD_TILE
#define LD_EMPTY 0xffffffffffffffffull
#define LD_MAX_BEAMS 128
#define LD_MAX_AZ 4096

struct LidarArgs {  // by value in the kernel arguments
    const float* map;
    const float* score;
    const float* imap;
    double fb;
    double q[12];  // row-major 3 x 4
    float threshold, intensity, min_depth, max_depth, max_height;
    int W;
    uint32_t n;  // H W
};

// steps 1-5 of pixel p < a.n; d: the f32 depth of the record
__device__ __forceinline__ bool lidar_record(const LidarArgs& a, uint32_t p, float4& rec, float& d) {
    const float m = a.map[p];
    if (a.fb > 0.0) {
        if (!(m > 0.f)) return false;
        d = (float)(a.fb / (double)m);
    } else {
        d = m;
    }
    if (!(d > a.min_depth && d <= a.max_depth)) return false;
    if (a.score && !(a.score[p] >= a.threshold)) return false;
    const uint32_t v = p / (uint32_t)a.W, u = p - v * (uint32_t)a.W;
    const double u1 = (double)(u + 1u), v1 = (double)(v + 1u), dd = (double)d;
    const double r0 = (a.q[0] * u1 + a.q[1] * v1) + a.q[2];
    const double r1 = (a.q[4] * u1 + a.q[5] * v1) + a.q[6];
    const double r2 = (a.q[8] * u1 + a.q[9] * v1) + a.q[10];
    const float x = (float)(dd * r0 - a.q[3]), y = (float)(dd * r1 - a.q[7]), z = (float)(dd * r2 - a.q[11]);
    if (!(x > 0.f && z <= a.max_height)) return false;
    rec = make_float4(x, y, z, a.imap ? a.imap[p] : a.intensity);
    return true;
}

// #{k in [0, n) : t[k] <= val} of a non-decreasing table; a NaN val counts nothing
__device__ __forceinline__ int lidar_upper(const double* __restrict__ t, int n, double val) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (val >= t[mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(LD_THREADS) void lidar_fill_kernel(unsigned long long* __restrict__ table, uint32_t n) {
    const uint32_t i = blockIdx.x * LD_THREADS + threadIdx.x;
    if (i < n) table[i] = LD_EMPTY;
}

// beam mode, pass 1: every kept pixel offers its key to its bin
__global__ __launch_bounds__(LD_THREADS) void lidar_key_kernel(LidarArgs a, int beams, int az_bins, const double* __restrict__ te,
                                                               const double* __restrict__ ta, unsigned long long* __restrict__ table) {
    const uint32_t p = blockIdx.x * LD_THREADS + threadIdx.x;
    if (p >= a.n) return;
    float4 rec;
    float d;
    if (!lidar_record(a, p, rec, d)) return;
    const double x = (double)rec.x, y = (double)rec.y, z = (double)rec.z;
    const double rho = sqrt(x * x + y * y);
    const int beam = lidar_upper(te, beams + 1, z / rho) - 1, col = lidar_upper(ta, az_bins + 1, y / x) - 1;
    if (beam < 0 || beam >= beams || col < 0 || col >= az_bins) return;
    atomicMin(&table[(size_t)beam * az_bins + col], ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)p);  // inside the table
}

// item i of the output order: pixel i (dense) or the winner of bin i (beam mode)
template <bool BEAM>
__device__ __forceinline__ bool lidar_item(const LidarArgs& a, const unsigned long long* __restrict__ table, uint32_t i, uint32_t n, float4& rec) {
    if (i >= n) return false;
    float d;
    if (BEAM) {
        const unsigned long long k = table[i];
        if (k == LD_EMPTY) return false;
        const uint32_t p = (uint32_t)k;
        return p < a.n && lidar_record(a, p, rec, d);  // the pixel's record again: p is a kept pixel, the test cannot fail
    }
    return lidar_record(a, i, rec, d);
}

template <bool BEAM>
__global__ __launch_bounds__(LD_THREADS) void lidar_count_kernel(LidarArgs a, const unsigned long long* __restrict__ table, uint32_t n,
                                                                 int64_t* __restrict__ counts) {
    __shared__ int wsum[LD_THREADS / 64];
    const uint32_t base = blockIdx.x * LD_TILE;
    int c = 0;
    float4 rec;
#pragma unroll
    for (int r = 0; r < LD_ROUNDS; ++r) {
        const uint32_t i = base + r * LD_THREADS + threadIdx.x;
        if (BEAM) c += (i < n && table[i] != LD_EMPTY) ? 1 : 0;
        else c += lidar_item<false>(a, table, i, n, rec) ? 1 : 0;
    }
    const int total = block_count(c, wsum);
    if (threadIdx.x == 0) counts[blockIdx.x] = (int64_t)total;
}

// the predicate again, ranked (block_rank, and a running base over the rounds); record j of the output is one 16-byte store, and only below
// `capacity`
template <bool BEAM>
__global__ __launch_bounds__(LD_THREADS) void lidar_scatter_kernel(LidarArgs a, const unsigned long long* __restrict__ table, uint32_t n,
                                                                   const int64_t* __restrict__ offsets, float4* __restrict__ out, int64_t capacity) {
    __shared__ int wsum[LD_THREADS / 64];
    const uint32_t base = blockIdx.x * LD_TILE;
    int64_t pos = offsets[blockIdx.x];
    for (int r = 0; r < LD_ROUNDS; ++r) {
        float4 rec;
        const bool keep = lidar_item<BEAM>(a, table, base + r * LD_THREADS + threadIdx.x, n, rec);
        int total;
        const int rank = block_rank(keep, wsum, total);
        if (keep) {
            const int64_t j = pos + rank;
            if (j < capacity) out[j] = rec;
        }
        pos += total;
    }
}

static int64_t lidar_blocks(int64_t n) { return (n + LD_TILE - 1) / LD_TILE; }
static bool lidar_shape_ok(int H, int W, int beams, int az_bins) {
    return H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) && beams >= 0 && beams <= LD_MAX_BEAMS && az_bins >= 1 && az_bins <= LD_MAX_AZ;
}

extern "C" int64_t falnet_lidar_workspace_bytes(int H, int W, int beams, int az_bins) {
    if (!lidar_shape_ok(H, W, beams, az_bins)) return 0;
    if (beams == 0) return lidar_blocks((int64_t)H * W) * (int64_t)sizeof(int64_t);
    const int64_t bins = (int64_t)beams * az_bins;
    return (bins + lidar_blocks(bins)) * (int64_t)sizeof(int64_t);
}

extern "C" int falnet_velo_unproject(const float* map, double fb, const float* score, float threshold, const float* intensity_map, float intensity,
                                     const double* Q, float min_depth, float max_depth, float max_height, int H, int W, int beams, int az_bins,
                                     const double* elev_edges_dev, const double* az_edges_dev, float* out_points, int64_t capacity, int64_t* count_dev,
                                     void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "velo_unproject: map %d x %d must hold between 1 and 2^31 pixels", H, W);
    FALNET_CHECK_ARG(beams >= 0 && beams <= LD_MAX_BEAMS, "velo_unproject: beams %d outside [0, %d] (0: dense)", beams, LD_MAX_BEAMS);
    FALNET_CHECK_ARG(az_bins >= 1 && az_bins <= LD_MAX_AZ, "velo_unproject: az_bins %d outside [1, %d]", az_bins, LD_MAX_AZ);
    FALNET_CHECK_ARG(map, "velo_unproject: null map");
    FALNET_CHECK_ARG(Q, "velo_unproject: null back-projection matrix");
    FALNET_CHECK_ARG(count_dev && workspace, "velo_unproject: null count or workspace");
    FALNET_CHECK_ARG(beams == 0 || (elev_edges_dev && az_edges_dev), "velo_unproject: null edge table with beams = %d", beams);
    FALNET_CHECK_ARG(capacity >= 0, "velo_unproject: capacity %lld is negative", (long long)capacity);
    FALNET_CHECK_ARG(capacity == 0 || out_points, "velo_unproject: null output with capacity %lld", (long long)capacity);
    FALNET_CHECK_ARG(fb >= 0.0 && isfinite(fb), "velo_unproject: fb %g must be finite and >= 0 (0: the map is a depth)", fb);
    FALNET_CHECK_ARG(isfinite(max_depth), "velo_unproject: max_depth %g is not finite", (double)max_depth);
    FALNET_CHECK_ARG(!isnan(min_depth) && !isnan(max_height) && !isnan(threshold), "velo_unproject: min_depth, max_height or threshold is NaN");
    LidarArgs a;
    for (int i = 0; i < 12; ++i) {
        FALNET_CHECK_ARG(isfinite(Q[i]), "velo_unproject: entry [%d][%d] of the back-projection matrix is not finite", i / 4, i % 4);
        a.q[i] = Q[i];
    }
    FALNET_CHECK_ARG((((uintptr_t)map | (uintptr_t)score | (uintptr_t)intensity_map) & 3) == 0, "velo_unproject: maps must be 4-byte aligned");
    FALNET_CHECK_ARG(((uintptr_t)out_points & 15) == 0, "velo_unproject: the output must be 16-byte aligned (one record is one 16-byte store)");
    FALNET_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)count_dev | (uintptr_t)elev_edges_dev | (uintptr_t)az_edges_dev) & 7) == 0,
                     "velo_unproject: workspace, count and edge tables must be 8-byte aligned");
    a.map = map, a.score = score, a.imap = intensity_map, a.fb = fb;
    a.threshold = threshold, a.intensity = intensity, a.min_depth = min_depth, a.max_depth = max_depth, a.max_height = max_height;
    a.W = W, a.n = (uint32_t)H * (uint32_t)W;
    hipStream_t st = (hipStream_t)stream;
    const dim3 threads(LD_THREADS);
    float4* out = reinterpret_cast<float4*>(out_points);
    if (beams == 0) {
        int64_t* counts = static_cast<int64_t*>(workspace);
        const int nb = (int)lidar_blocks(a.n);
        hipLaunchKernelGGL(lidar_count_kernel<false>, dim3(nb), threads, 0, st, a, (const unsigned long long*)nullptr, a.n, counts);
        falnet_offset_scan(counts, nb, count_dev, st);
        hipLaunchKernelGGL(lidar_scatter_kernel<false>, dim3(nb), threads, 0, st, a, (const unsigned long long*)nullptr, a.n, counts, out, capacity);
    } else {
        const uint32_t bins = (uint32_t)beams * (uint32_t)az_bins;
        unsigned long long* table = static_cast<unsigned long long*>(workspace);
        int64_t* counts = static_cast<int64_t*>(workspace) + bins;
        const int nb = (int)lidar_blocks(bins);
        hipLaunchKernelGGL(lidar_fill_kernel, dim3((bins + LD_THREADS - 1) / LD_THREADS), threads, 0, st, table, bins);
        hipLaunchKernelGGL(lidar_key_kernel, dim3((a.n + LD_THREADS - 1) / LD_THREADS), threads, 0, st, a, beams, az_bins, elev_edges_dev, az_edges_dev, table);
        hipLaunchKernelGGL(lidar_count_kernel<true>, dim3(nb), threads, 0, st, a, table, bins, counts);
        falnet_offset_scan(counts, nb, count_dev, st);
        hipLaunchKernelGGL(lidar_scatter_kernel<true>, dim3(nb), threads, 0, st, a, table, bins, counts, out, capacity);
    }
    FALNET_RETURN_LAUNCH();
}
