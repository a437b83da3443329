// Weight-decayed form of the optimiser step fused with the weight re-pack (conv.hip: adam_pack_batched_kernel; torch.optim.Adam with
// weight_decay != 0, the `weight_parameters()` group of Train_Stage1_K.py:177-180).
//
// One block = one 32(cout) x 32(packed cin) tile of one layer, all taps: the f32 OIHW master tile is UPDATED while it is loaded into LDS
// (gr = g * grad_scale + decay * w, then the moments and the step of losses.hip: adam_dev_kernel) and leaves as the wf rows
// ([co][tap][32 cin]) and wd rows ([cin][tap][32 cout]) of the compute dtype -- the same tile geometry, descriptor (falnet_pack_t) and packed
// layout as conv.hip: pack_tile, so a layer packed here and one packed by falnet_pack_weights_batched from the same masters are bit-identical.
// ONE decay per launch is enough: every packed layer is a convolution WEIGHT (biases are never packed; they and the unpacked weights go
// through falnet_adam_ranges_wd with a decay per range).  Entries with no_update (derived weights: the composed logits conv) are only packed.
//
// A file of its own rather than a template flag on conv.hip's kernel: the autotune cache is keyed on a hash of the convolution sources
// (ops.py: _TUNE_SOURCES), and the decayed update is no reason to invalidate every tuned convolution choice.
// The price is a second copy of pack_tile's tile geometry, kept in step by hand (tests/test_gpu_adam_decay.py compares every operand packed here
// bit for bit with conv.hip's pack of the same masters).  When conv.hip is next changed for a reason of its own -- and the cache re-tuned
// anyway -- fold the decay into PackAdam / a template flag of its pack_tile and DELETE this file.
#include "common.h"

struct PackAdamWd {
    int64_t g_off, m_off, v_off;  // element offsets from a master weight to its gradient / first / second moment (the flat buffers share one layout)
    float b1, b2, eps, grad_scale, step_size, rsqrt_bc2;
    double decay;  // gr is formed in double and rounded once (losses.hip: decayed_grad -- where g and decay * w cancel, an f32 sum would not do)
};

template <typename T, int TAPS, bool UPDATE>
__device__ __forceinline__ void pack_tile_wd(const falnet_pack_t& d, int rel, float (&tile)[32][32 * 9 + 1], const PackAdamWd& ad) {
    const int ctiles = d.cin_pad / 32;
    const int co0 = (rel / ctiles) * 32, cp0 = (rel % ctiles) * 32;
    constexpr int rowlen = 32 * TAPS;
    // packed columns cp0..cp0+31 map to a contiguous run of real channels (group boundaries are multiples of 32)
    const int ci0 = cp0 < d.c0_pad ? cp0 : d.c0_real + (cp0 - d.c0_pad);
    const int ci_end = cp0 < d.c0_pad ? d.c0_real : d.cin;  // exclusive bound of valid real channels for this tile
    for (int e = threadIdx.x; e < 32 * rowlen; e += 256) {
        const int r = e / rowlen, k = e % rowlen;  // r: cout row of the tile, k = cil*TAPS + t
        const int co = co0 + r, ci = ci0 + k / TAPS;
        float val = 0.f;
        if (co < d.cout && ci < ci_end) {  // real elements only: the padded rows / columns of the packed copies are zeros, never read from w
            float* wp = const_cast<float*>(d.w) + ((int64_t)co * d.cin + ci0) * TAPS + k;
            val = *wp;
            if constexpr (UPDATE) {
                const float gr = (float)fma(ad.decay, (double)val, (double)wp[ad.g_off] * (double)ad.grad_scale);
                const float m = ad.b1 * wp[ad.m_off] + (1.f - ad.b1) * gr;
                const float v = ad.b2 * wp[ad.v_off] + (1.f - ad.b2) * gr * gr;
                val -= ad.step_size * m / (sqrtf(v) * ad.rsqrt_bc2 + ad.eps);
                *wp = val;
                wp[ad.m_off] = m;
                wp[ad.v_off] = v;
            }
        }
        tile[r][k] = val;
    }
    __syncthreads();
    T* wf = reinterpret_cast<T*>(d.wf);
    T* wd = reinterpret_cast<T*>(d.wd);
    // eight consecutive channels per thread and store (16 B in the 16-bit types)
    for (int e = threadIdx.x; e < 32 * TAPS * 4; e += 256) {
        const int g = e & 3, t = (e >> 2) % TAPS, r = e / (4 * TAPS);
        float vf[8], vd[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            vf[j] = tile[r][(8 * g + j) * TAPS + t];  // r = cout row, channels 8 g + j of the cin tile
            vd[j] = tile[8 * g + j][r * TAPS + t];    // r = cin row, channels 8 g + j of the cout tile
        }
        T* pf = wf ? wf + ((int64_t)(co0 + r) * TAPS + t) * d.cin_pad + cp0 + 8 * g : nullptr;
        T* pd = wd ? wd + ((int64_t)(cp0 + r) * TAPS + t) * d.cout_pad + co0 + 8 * g : nullptr;
        if constexpr (sizeof(T) == 2) {
            uint4 of, od;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                (&of.x)[k] = pack16x2<T>(vf[2 * k], vf[2 * k + 1]);
                (&od.x)[k] = pack16x2<T>(vd[2 * k], vd[2 * k + 1]);
            }
            if (pf) *reinterpret_cast<uint4*>(pf) = of;
            if (pd) *reinterpret_cast<uint4*>(pd) = od;
        } else {
            if (pf) {
                reinterpret_cast<float4*>(pf)[0] = make_float4(vf[0], vf[1], vf[2], vf[3]);
                reinterpret_cast<float4*>(pf)[1] = make_float4(vf[4], vf[5], vf[6], vf[7]);
            }
            if (pd) {
                reinterpret_cast<float4*>(pd)[0] = make_float4(vd[0], vd[1], vd[2], vd[3]);
                reinterpret_cast<float4*>(pd)[1] = make_float4(vd[4], vd[5], vd[6], vd[7]);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void adam_pack_batched_wd_kernel(const falnet_pack_t* __restrict__ descs, int n, int64_t g_off, int64_t m_off, int64_t v_off,
                                                                   const float* __restrict__ state, float b1, float b2, float eps, float grad_scale,
                                                                   double decay, const float* __restrict__ scaler) {
    __shared__ float tile[32][32 * 9 + 1];
    __shared__ int entry_begin[64];
    if (scaler != nullptr) {
        if (scaler[2] != 0.f) return;  // non-finite gradient somewhere: update AND decay are skipped, the packed copies stay valid (grid-uniform)
        grad_scale /= scaler[0];
    }
    const float t = state[1] + 1.0f;
    PackAdamWd ad;
    ad.g_off = g_off, ad.m_off = m_off, ad.v_off = v_off;
    ad.b1 = b1, ad.b2 = b2, ad.eps = eps, ad.grad_scale = grad_scale, ad.decay = decay;
    ad.step_size = state[0] / (1.0f - powf(b1, t));
    ad.rsqrt_bc2 = rsqrtf(1.0f - powf(b2, t));
    // entry of this block: the block_begin column in LDS, then a binary search (n <= 64, checked by the launcher)
    for (int i = threadIdx.x; i < n; i += blockDim.x) entry_begin[i] = descs[i].block_begin;
    __syncthreads();
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= entry_begin[mid]) lo = mid;
        else hi = mid - 1;
    }
    const falnet_pack_t d = descs[lo];
    const int rel = blockIdx.x - d.block_begin;
    if (d.no_update) {  // derived weights (their factors were updated by falnet_adam_ranges_wd and re-composed before this launch)
        if (d.taps == 9) pack_tile_wd<T, 9, false>(d, rel, tile, ad);
        else if (d.taps == 3) pack_tile_wd<T, 3, false>(d, rel, tile, ad);
        else pack_tile_wd<T, 1, false>(d, rel, tile, ad);
    } else if (d.taps == 9) pack_tile_wd<T, 9, true>(d, rel, tile, ad);
    else if (d.taps == 3) pack_tile_wd<T, 3, true>(d, rel, tile, ad);
    else pack_tile_wd<T, 1, true>(d, rel, tile, ad);
}

extern "C" int falnet_adam_pack_batched_wd(const falnet_pack_t* descs_dev, int n, int total_blocks, int dtype, int64_t g_off, int64_t m_off, int64_t v_off,
                                           const float* state, float b1, float b2, float eps, float grad_scale, double weight_decay, const float* scaler,
                                           void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(descs_dev && n > 0 && n <= 64 && total_blocks > 0 && state, "adam_pack_batched_wd: bad argument (n <= 64)");
    FALNET_CHECK_ARG(g_off != 0 && m_off != 0 && v_off != 0 && g_off != m_off && g_off != v_off && m_off != v_off,
                     "adam_pack_batched_wd: gradient / moment buffers must be distinct from the weights and from each other");
#define APACK_WD(T) hipLaunchKernelGGL(adam_pack_batched_wd_kernel<T>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n, g_off, m_off, \
                                       v_off, state, b1, b2, eps, grad_scale, weight_decay, scaler)
    FALNET_DISPATCH_DTYPE(dtype, APACK_WD);
#undef APACK_WD
    FALNET_RETURN_LAUNCH();
}
