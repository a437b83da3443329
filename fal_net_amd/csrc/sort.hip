// Stable segmented argsort of 32-bit keys: perm[s * n + r] is the index of the element of segment s with rank r in ascending key order, equal keys
// in ascending index order (np.argsort(kind="stable")).  Least-significant-digit radix, four passes of 8 bits over (key, index) pairs that
// ping-pong between two buffers of the workspace; the first pass reads the caller's keys (which are never written), the last one writes the
// indices alone into perm.
//
// A pass is the three launches of compact.hip with 256 bins in the place of one flag; every segment rides in the same
// launches as blockIdx.y:
//   1  sort_hist_kernel     workgroup g counts the digits of its ST_TILE consecutive positions               -> table[digit][g]
//   2  sort_scan_kernel     ONE workgroup per segment turns the 256 x tiles counts, digit-major and tile-minor, into exclusive offsets in
//                           place, SC_STEP entries at a time with a carried base (any number of tiles)
//   3  sort_scatter_kernel  workgroup g reads its digits again and ranks every element among the earlier elements of the tile with the same
//                           digit -- earlier rounds, then lower waves, then lower lanes -- and writes it to table[digit][g] + rank
// Inside a wave the lanes that share a digit come from eight ballots and the rank from a popcount of the lower lanes; across waves and rounds
// from the waves' digit counts in LDS, which the thread that owns a digit adds up in (round, wave) order.  The histogram counts with integer
// LDS atomics (a count has no order); no output position depends on the return value or the arrival order of an atomic, so two calls write the
// same bytes.  Integer arithmetic only, no scratch.
#include "common.h"

#define ST_THREADS 256
#define ST_ROUNDS 8
#define ST_TILE (ST_THREADS * ST_ROUNDS)
#define ST_WAVES (ST_THREADS / 64)
#define ST_SLOTS (ST_ROUNDS * ST_WAVES)  // the (round, wave) pairs of a tile, in the order that "earlier" means
#define SC_PER_THREAD 16
#define SC_STEP (ST_THREADS * SC_PER_THREAD)
#define ST_MAX_N (1ll << 24)
#define ST_MAX_SEGMENTS 8

// element i of the pass's source: the caller's keys with the position as the index (first pass), or a (key, index) pair
template <bool FIRST> __device__ __forceinline__ uint2 sort_load(const void* __restrict__ src, uint32_t seg_base, uint32_t i) {
    if (FIRST) return make_uint2(static_cast<const uint32_t*>(src)[seg_base + i], i);
    return static_cast<const uint2*>(src)[seg_base + i];
}

template <bool FIRST>
__global__ __launch_bounds__(ST_THREADS) void sort_hist_kernel(const void* __restrict__ src, uint32_t n, int shift, uint32_t* __restrict__ table,
                                                               uint32_t tiles) {
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t seg_base = blockIdx.y * n, base = blockIdx.x * ST_TILE;
#pragma unroll
    for (int r = 0; r < ST_ROUNDS; ++r) {
        const uint32_t i = base + r * ST_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&hist[(sort_load<FIRST>(src, seg_base, i).x >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[((size_t)blockIdx.y * 256 + threadIdx.x) * tiles + blockIdx.x] = hist[threadIdx.x];
}

// exclusive scan of a segment's `len` = 256 * tiles counts in place.  A step takes SC_STEP consecutive entries, SC_PER_THREAD per thread: the
// thread's own sum, an inclusive scan of the 64 sums of a wave by shuffles, the four wave totals through LDS, and the base carried from the
// steps before.
__global__ __launch_bounds__(ST_THREADS) void sort_scan_kernel(uint32_t* __restrict__ table, uint32_t len) {
    __shared__ uint32_t wtot[ST_WAVES];
    uint32_t* t = table + (size_t)blockIdx.y * len;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;  // every thread carries the same value
    for (uint32_t e0 = 0; e0 < len; e0 += SC_STEP) {
        const uint32_t first = e0 + threadIdx.x * SC_PER_THREAD;
        uint32_t v[SC_PER_THREAD], sum = 0;
#pragma unroll
        for (int k = 0; k < SC_PER_THREAD; ++k) {
            v[k] = first + k < len ? t[first + k] : 0u;
            sum += v[k];
        }
        uint32_t inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        __syncthreads();  // the previous step's totals are read
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        uint32_t before = carry, total = 0;
#pragma unroll
        for (int w = 0; w < ST_WAVES; ++w) {
            before += w < wave ? wtot[w] : 0u;
            total += wtot[w];
        }
        uint32_t run = before + inc - sum;
#pragma unroll
        for (int k = 0; k < SC_PER_THREAD; ++k) {
            if (first + k < len) t[first + k] = run;
            run += v[k];
        }
        carry += total;
    }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(ST_THREADS) void sort_scatter_kernel(const void* __restrict__ src, uint32_t n, int shift, const uint32_t* __restrict__ table,
                                                                  uint32_t tiles, void* __restrict__ dst) {
    __shared__ uint32_t cnt[ST_SLOTS][256];  // [round * ST_WAVES + wave][digit]: the wave's count, then the position of its first such element
#pragma unroll
    for (int k = 0; k < ST_SLOTS; ++k) cnt[k][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t seg_base = blockIdx.y * n, base = blockIdx.x * ST_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lower = (1ull << lane) - 1ull;
    uint2 e[ST_ROUNDS];
    uint32_t rank[ST_ROUNDS];
#pragma unroll
    for (int r = 0; r < ST_ROUNDS; ++r) {
        const uint32_t i = base + r * ST_THREADS + threadIdx.x;
        const bool in = i < n;
        e[r] = in ? sort_load<FIRST>(src, seg_base, i) : make_uint2(0u, 0u);
        const uint32_t d = (e[r].x >> shift) & 255u;
        unsigned long long same = __ballot(in);  // the lanes of this wave that hold an element with the digit d
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        rank[r] = (uint32_t)__popcll(same & lower);
        if (in && rank[r] == 0) cnt[r * ST_WAVES + wave][d] = (uint32_t)__popcll(same);  // one lane per digit and wave: no two write the same word
    }
    __syncthreads();
    {  // thread d owns digit d: the tile's base for the digit, then the counts of the earlier (round, wave) pairs in order
        uint32_t run = table[((size_t)blockIdx.y * 256 + threadIdx.x) * tiles + blockIdx.x];
#pragma unroll
        for (int k = 0; k < ST_SLOTS; ++k) {
            const uint32_t c = cnt[k][threadIdx.x];
            cnt[k][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ST_ROUNDS; ++r) {
        const uint32_t i = base + r * ST_THREADS + threadIdx.x;
        if (i >= n) continue;
        const uint32_t pos = cnt[r * ST_WAVES + wave][(e[r].x >> shift) & 255u] + rank[r];  // < n: the counts of a segment sum to n
        if (LAST) static_cast<uint32_t*>(dst)[seg_base + pos] = e[r].y;
        else static_cast<uint2*>(dst)[seg_base + pos] = e[r];
    }
}

static int64_t sort_tiles(int64_t n) { return (n + ST_TILE - 1) / ST_TILE; }
static int64_t sort_pair_bytes(int64_t n, int segments) { return (int64_t)segments * n * 8; }

extern "C" int64_t falnet_sort_u32_workspace_bytes(int64_t n, int segments) {
    if (n < 1 || n > ST_MAX_N || segments < 1 || segments > ST_MAX_SEGMENTS) return 0;
    return 2 * sort_pair_bytes(n, segments) + (((int64_t)segments * 256 * sort_tiles(n) * 4 + 7) & ~(int64_t)7);
}

extern "C" int falnet_sort_u32(const uint32_t* keys, int64_t n, int segments, uint32_t* perm, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(n >= 0 && n <= ST_MAX_N, "sort_u32: n=%lld keys per segment (at most 2^24)", (long long)n);
    FALNET_CHECK_ARG(segments >= 1 && segments <= ST_MAX_SEGMENTS, "sort_u32: %d segments (1 to %d)", segments, ST_MAX_SEGMENTS);
    FALNET_CHECK_ARG(keys && perm && workspace, "sort_u32: null pointer");
    FALNET_CHECK_ARG((reinterpret_cast<uintptr_t>(perm) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                     "sort_u32: perm and workspace must be 8-byte aligned");
    FALNET_CHECK_ARG((reinterpret_cast<uintptr_t>(keys) & 3) == 0, "sort_u32: keys must be 4-byte aligned");
    if (n == 0) return 0;
    const uint32_t tiles = (uint32_t)sort_tiles(n), un = (uint32_t)n;
    uint2* a = static_cast<uint2*>(workspace);
    uint2* b = a + (size_t)segments * n;
    uint32_t* table = reinterpret_cast<uint32_t*>(b + (size_t)segments * n);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(tiles, (unsigned)segments), scan_grid(1, (unsigned)segments), block(ST_THREADS);
    // pass 0: keys -> a
    hipLaunchKernelGGL(sort_hist_kernel<true>, grid, block, 0, st, (const void*)keys, un, 0, table, tiles);
    hipLaunchKernelGGL(sort_scan_kernel, scan_grid, block, 0, st, table, 256u * tiles);
    hipLaunchKernelGGL((sort_scatter_kernel<true, false>), grid, block, 0, st, (const void*)keys, un, 0, (const uint32_t*)table, tiles, (void*)a);
    // passes 1 and 2: a -> b -> a
    for (int pass = 1; pass < 3; ++pass) {
        const uint2* from = pass == 1 ? a : b;
        uint2* to = pass == 1 ? b : a;
        hipLaunchKernelGGL(sort_hist_kernel<false>, grid, block, 0, st, (const void*)from, un, 8 * pass, table, tiles);
        hipLaunchKernelGGL(sort_scan_kernel, scan_grid, block, 0, st, table, 256u * tiles);
        hipLaunchKernelGGL((sort_scatter_kernel<false, false>), grid, block, 0, st, (const void*)from, un, 8 * pass, (const uint32_t*)table, tiles, (void*)to);
    }
    // pass 3: a -> perm, the indices alone
    hipLaunchKernelGGL(sort_hist_kernel<false>, grid, block, 0, st, (const void*)a, un, 24, table, tiles);
    hipLaunchKernelGGL(sort_scan_kernel, scan_grid, block, 0, st, table, 256u * tiles);
    hipLaunchKernelGGL((sort_scatter_kernel<false, true>), grid, block, 0, st, (const void*)a, un, 24, (const uint32_t*)table, tiles, (void*)perm);
    FALNET_RETURN_LAUNCH();
}
