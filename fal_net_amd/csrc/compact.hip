// Ordered stream compaction: keep record i of `src` when score[i] >= threshold (a NaN score compares false and is dropped), in index order.
//
// Three launches, no atomics, nothing decides a position but the index:
//   1  compact_count_kernel    workgroup g counts the kept records of its CP_TILE consecutive indices          -> ws[g]
//   2  offset_scan_kernel      ONE workgroup turns the counts into exclusive offsets in place, 256 at a time    -> ws[g], *count
//   3  compact_scatter_kernel  workgroup g evaluates its flags again, ranks them (block_rank: ballot + popcount inside a wave, the wave totals
//                              through LDS; a running base over the CP_ROUNDS rounds) and copies record i to dst[ws[g] + rank]
// Records are 4 bytes (one word) or 15 bytes (a packed PLY vertex, unaligned: copied byte by byte).  dst beyond the kept records is not written.
// The tile, block_count and block_rank are ordered.h's; the scan kernel is the only one of the library: lidar.hip and sparsify.hip reach it
// through falnet_offset_scan, defined here.
#include "common.h"
#include "ordered.h"

#define CP_THREADS ORD_THREADS
#define CP_ROUNDS ORD_ROUNDS
#define CP_TILE ORD_TILE

__device__ __forceinline__ bool compact_keep(const float* __restrict__ score, float threshold, int64_t i, int64_t n) {
    return i < n && score[i] >= threshold;
}

__global__ __launch_bounds__(CP_THREADS) void compact_count_kernel(const float* __restrict__ score, float threshold, int64_t n,
                                                                   int64_t* __restrict__ ws) {
    __shared__ int wsum[CP_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * CP_TILE;
    int c = 0;
#pragma unroll
    for (int r = 0; r < CP_ROUNDS; ++r) c += compact_keep(score, threshold, base + r * CP_THREADS + threadIdx.x, n) ? 1 : 0;
    const int total = block_count(c, wsum);
    if (threadIdx.x == 0) ws[blockIdx.x] = (int64_t)total;
}

// 256 counts at a time: an inclusive scan in LDS, and a carried base from one 256 to the next
__global__ __launch_bounds__(CP_THREADS) void offset_scan_kernel(int64_t* __restrict__ ws, int64_t nblocks, int64_t* __restrict__ count) {
    __shared__ int64_t sh[CP_THREADS];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t g0 = 0; g0 < nblocks; g0 += CP_THREADS) {
        const int64_t g = g0 + threadIdx.x;
        const int64_t v = g < nblocks ? ws[g] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < CP_THREADS; o <<= 1) {  // inclusive scan of the 256 counts
            const int64_t add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        const int64_t before = carry;
        if (g < nblocks) ws[g] = before + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == CP_THREADS - 1) carry = before + sh[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}

void falnet_offset_scan(int64_t* counts, int64_t nblocks, int64_t* total, hipStream_t st) {
    hipLaunchKernelGGL(offset_scan_kernel, dim3(1), dim3(CP_THREADS), 0, st, counts, nblocks, total);
}

template <int REC>
__global__ __launch_bounds__(CP_THREADS) void compact_scatter_kernel(const unsigned char* __restrict__ src, const float* __restrict__ score,
                                                                     float threshold, int64_t n, unsigned char* __restrict__ dst,
                                                                     const int64_t* __restrict__ ws) {
    __shared__ int wsum[CP_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * CP_TILE;
    int64_t pos = ws[blockIdx.x];
    for (int r = 0; r < CP_ROUNDS; ++r) {
        const int64_t i = base + r * CP_THREADS + threadIdx.x;
        const bool keep = compact_keep(score, threshold, i, n);
        int total;
        const int rank = block_rank(keep, wsum, total);
        if (keep) {
            const int64_t j = pos + rank;
            if (REC == 4) {
                reinterpret_cast<uint32_t*>(dst)[j] = reinterpret_cast<const uint32_t*>(src)[i];
            } else {
#pragma unroll
                for (int k = 0; k < REC; ++k) dst[j * REC + k] = src[i * REC + k];
            }
        }
        pos += total;
    }
}

static int64_t compact_blocks(int64_t n) { return (n + CP_TILE - 1) / CP_TILE; }

extern "C" int64_t falnet_compact_workspace_bytes(int64_t n) { return n > 0 ? compact_blocks(n) * (int64_t)sizeof(int64_t) : 0; }

extern "C" int falnet_compact_records(const void* src, int rec_bytes, const float* score, float threshold, int64_t n, void* dst, int64_t* count_dev,
                                      void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(rec_bytes == 4 || rec_bytes == 15, "compact_records: records of %d bytes (4 or 15 only)", rec_bytes);
    FALNET_CHECK_ARG(n > 0, "compact_records: n=%lld records", (long long)n);
    FALNET_CHECK_ARG(src && score && dst && count_dev && workspace, "compact_records: null pointer");
    FALNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(count_dev) & 7) == 0,
                     "compact_records: workspace and count_dev must be 8-byte aligned");
    FALNET_CHECK_ARG(rec_bytes != 4 || ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) == 0,
                     "compact_records: 4-byte records must be 4-byte aligned");
    const int64_t nb = compact_blocks(n);
    FALNET_CHECK_ARG(nb < (1ll << 31), "compact_records: n=%lld is too many records for one call", (long long)n);
    int64_t* ws = static_cast<int64_t*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nb), dim3(CP_THREADS), 0, st, score, threshold, n, ws);
    falnet_offset_scan(ws, nb, count_dev, st);
    if (rec_bytes == 4)
        hipLaunchKernelGGL(compact_scatter_kernel<4>, dim3((unsigned)nb), dim3(CP_THREADS), 0, st, static_cast<const unsigned char*>(src), score, threshold, n,
                           static_cast<unsigned char*>(dst), ws);
    else
        hipLaunchKernelGGL(compact_scatter_kernel<15>, dim3((unsigned)nb), dim3(CP_THREADS), 0, st, static_cast<const unsigned char*>(src), score, threshold,
                           n, static_cast<unsigned char*>(dst), ws);
    FALNET_RETURN_LAUNCH();
}
