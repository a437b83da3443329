// Primitives whose result is decided by indices and integers alone, written ONCE for the evaluation-side kernels that the tests hold bit for
// bit: the monotone integer image of a float (dump.hip, velo.hip, metrics.hip, sparsify.hip), the f64 sum over a wave (metrics.hip,
// sparsify.hip) and the pieces of the ordered compaction -- count, ONE offset scan, scatter -- of compact.hip, lidar.hip, sparsify.hip and mesh.hip
// (DESIGN.md section 7d).  Device code is __forceinline__ and there is no __global__ in this file: the one scan kernel lives in compact.hip.
// Not part of common.h on purpose: that file is hashed into the autotune cache header (ops.py: _TUNE_SOURCES), this one is not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- monotone keys: x < y as floats <=> key(x) < key(y) as unsigned integers ---------------------------------------------------------------
// Negative floats: all bits flipped; others: sign bit set.  -0 sorts below +0; a NaN keeps its place by its bits (a positive NaN above
// +infinity; the all-ones key is a positive NaN only).  unkey is the inverse.
__device__ __forceinline__ uint32_t key_f32(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unkey_f32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ uint64_t key_f64(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double unkey_f64(uint64_t k) { return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k)); }

// ---- the sum of one double per lane over a wave, in the fixed order of the xor shuffles: every lane gets it -----------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- ordered compaction -----------------------------------------------------------------------------------------------------------------------
// Workgroup g of ORD_THREADS threads owns the ORD_TILE consecutive indices from g ORD_TILE on, ORD_ROUNDS rounds of one index per thread.  A
// count kernel writes how many of them its predicate keeps, falnet_offset_scan turns the counts into exclusive offsets, and a scatter kernel
// evaluates the same predicate again and ranks what it keeps.  The loop over the rounds, the predicate, the running position and what is
// emitted are the kernel's own; `wsum` is its LDS array of ORD_THREADS / 64 words.
#define ORD_THREADS 256
#define ORD_ROUNDS 8
#define ORD_TILE (ORD_THREADS * ORD_ROUNDS)

// the end of a count kernel: c kept indices in this thread -> their number in the workgroup, valid in thread 0.  One barrier.
__device__ __forceinline__ int block_count(int c, int* wsum) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one round of a scatter kernel: the number of kept indices of this round below this thread's (ballot + popcount inside the wave, the wave
// totals through LDS), valid where `keep`; total: the round's kept indices.  Two barriers: every thread of the workgroup calls it.
__device__ __forceinline__ int block_rank(bool keep, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(keep);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();  // the previous round's totals are read
    if (lane == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < ORD_THREADS / 64; ++w) {
        before += w < wave ? wsum[w] : 0;
        total += wsum[w];
    }
    return before + rank;
}

// counts[0 .. nblocks) -> their exclusive prefix sums in place, *total: their sum.  One launch of one workgroup on `st` (compact.hip); a launch
// error is the caller's to collect (FALNET_RETURN_LAUNCH).  Internal: not part of the C-ABI.
void falnet_offset_scan(int64_t* counts, int64_t nblocks, int64_t* total, hipStream_t st);
