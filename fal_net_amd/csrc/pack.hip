// Weight packing: the f32 OIHW masters -> the packed operands of the convolution kernels (include/falnet_hip.h: wf / wd rows, the sub-pixel
// weights of the deconv layers), and the optimiser step fused with the re-pack (torch.optim.Adam with or without weight decay).
// Not one of the autotuned sources (ops.py: _TUNE_SOURCES): a change here leaves every cached convolution choice valid.
#include <type_traits>
#include "adam.h"
#include "common.h"

// One block = one 32(cout) x 32(packed cin) tile of one layer, all taps, staged through LDS: the OIHW reads are
// runs of taps*32 contiguous floats, the wf rows ([co][tap][32 cin]) and wd rows ([cin][tap][32 cout]) are written as
// 32 contiguous elements.  (The element-per-thread version gathered with stride `taps` and scattered 2-byte writes.)
// ADAM: the tile's master weights are UPDATED while they are loaded (torch.optim.Adam, Train_Stage1_K.py:177-180: adam.h, the update the
// kernels of adam.hip apply) -- every real (co, ci, tap) element of a layer belongs to exactly one tile, so the optimiser step of all
// packed layers and their re-pack are ONE pass over the masters (the stand-alone re-pack read the 68 MB Adam had just written again).
// The update is a compile-time policy of the load loop: PackNone (plain pack, and the no_update entries of an Adam launch), PackAdam<AdamGrad>,
// PackAdam<AdamGradL2> (weight_decay != 0, the `weight_parameters()` group of Train_Stage1_K.py:177-180).  The two Adam forms differ in the
// gradient they feed the moments and keep their own arithmetic: the undecayed one is NOT the decayed one at decay = 0 (f32 product vs one
// rounding of a double fma), and it is the benchmarked step.
struct PackNone {};
template <typename Grad>
struct PackAdam {
    AdamCoef c;
    Grad grad;
    int64_t g_off, m_off, v_off;  // element offsets from a master weight to its gradient / first / second moment (the flat buffers share one layout)
};
template <typename T, int TAPS, typename Update = PackNone>
__device__ __forceinline__ void pack_tile(const falnet_pack_t& d, int rel, float (&tile)[32][32 * 9 + 1], const Update* ad = nullptr) {
    const int ctiles = d.cin_pad / 32;
    const int co0 = (rel / ctiles) * 32, cp0 = (rel % ctiles) * 32;
    constexpr int rowlen = 32 * TAPS;
    // packed columns cp0..cp0+31 map to a contiguous run of real channels (group boundaries are multiples of 32)
    const int ci0 = cp0 < d.c0_pad ? cp0 : d.c0_real + (cp0 - d.c0_pad);
    const int ci_end = cp0 < d.c0_pad ? d.c0_real : d.cin;   // exclusive bound of valid real channels for this tile
    for (int e = threadIdx.x; e < 32 * rowlen; e += 256) {
        const int r = e / rowlen, k = e % rowlen;            // r: cout row of the tile, k = cil*TAPS + t
        const int co = co0 + r, ci = ci0 + k / TAPS;
        float val = 0.f;
        if (co < d.cout && ci < ci_end) {  // real elements only: the padded rows / columns of the packed copies are zeros, never read from w
            float* wp = const_cast<float*>(d.w) + ((int64_t)co * d.cin + ci0) * TAPS + k;
            val = *wp;
            if constexpr (!std::is_same<Update, PackNone>::value) {
                const float g = wp[ad->g_off];
                // v before m on purpose: the order of these loads decides which of the two multiplies of the first moment the compiler fuses
                // into its add, i.e. the bits of m (tools/isa_identity.py against the parent commit shows a change)
                float v = wp[ad->v_off], m = wp[ad->m_off];
                adam_update(ad->c, ad->grad, val, g, m, v);
                *wp = val;
                wp[ad->m_off] = m;
                wp[ad->v_off] = v;
            }
        }
        tile[r][k] = val;
    }
    __syncthreads();
    T* wf = reinterpret_cast<T*>(d.wf);
    T* wd = reinterpret_cast<T*>(d.wd);
    // eight consecutive channels per thread and store (16 B in the 16-bit types): the first version stored one element per lane -- 2-B scalar
    // stores, 128 B per wave instruction -- and ran the 204 MB of the step's re-pack at 2 TB/s
    for (int e = threadIdx.x; e < 32 * TAPS * 4; e += 256) {
        const int g = e & 3, t = (e >> 2) % TAPS, r = e / (4 * TAPS);
        float vf[8], vd[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            vf[j] = tile[r][(8 * g + j) * TAPS + t];   // r = cout row, channels 8 g + j of the cin tile
            vd[j] = tile[8 * g + j][r * TAPS + t];     // r = cin row, channels 8 g + j of the cout tile
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

// One block = one 32(cout) x 32(packed cin) tile of one layer, all taps, staged through LDS: the OIHW reads are
// runs of taps*32 contiguous floats, the wf rows ([co][tap][32 cin]) and wd rows ([cin][tap][32 cout]) are written as
// 32 contiguous elements.  taps is 9, 3 or 1 (compile-time divisions).
template <typename T>
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const falnet_pack_t* __restrict__ descs, int n) {
    __shared__ float tile[32][32 * 9 + 1];
    __shared__ int entry_begin[64];
    const int li = find_entry(descs, n, entry_begin);
    const falnet_pack_t d = descs[li];
    const int rel = blockIdx.x - d.block_begin;
    if (d.taps == 9) pack_tile<T, 9>(d, rel, tile);
    else if (d.taps == 3) pack_tile<T, 3>(d, rel, tile);  // 3x1 / 1x3 (FAL_netA.py:73-76)
    else pack_tile<T, 1>(d, rel, tile);
}

// The optimiser step of every packed layer fused with its re-pack; ONE decay per launch is enough: every packed layer is a convolution
// WEIGHT (biases are never packed; they and the unpacked weights go through falnet_adam_ranges[_wd] with a decay per range).
template <typename T, typename Grad>
__device__ __forceinline__ void adam_pack_batched_body(Grad grad, const falnet_pack_t* __restrict__ descs, int n, int64_t g_off, int64_t m_off, int64_t v_off,
                                                       const float* __restrict__ state, float b1, float b2, float eps, float grad_scale,
                                                       const float* __restrict__ scaler) {
    __shared__ float tile[32][32 * 9 + 1];
    __shared__ int entry_begin[64];
    PackAdam<Grad> ad{{}, grad, g_off, m_off, v_off};
    if (!adam_begin(ad.c, state, b1, b2, eps, grad_scale, scaler)) return;  // a skipped step leaves the packed copies valid (grid-uniform)
    const int li = find_entry(descs, n, entry_begin);
    const falnet_pack_t d = descs[li];
    const int rel = blockIdx.x - d.block_begin;
    if (d.no_update) {  // derived weights (their factors were updated by falnet_adam_ranges[_wd] and re-composed before this launch)
        if (d.taps == 9) pack_tile<T, 9>(d, rel, tile);
        else if (d.taps == 3) pack_tile<T, 3>(d, rel, tile);
        else pack_tile<T, 1>(d, rel, tile);
    } else if (d.taps == 9) pack_tile<T, 9>(d, rel, tile, &ad);
    else if (d.taps == 3) pack_tile<T, 3>(d, rel, tile, &ad);
    else pack_tile<T, 1>(d, rel, tile, &ad);
}

template <typename T>
__global__ __launch_bounds__(256) void adam_pack_batched_kernel(const falnet_pack_t* __restrict__ descs, int n, int64_t g_off, int64_t m_off, int64_t v_off,
                                                                const float* __restrict__ state, float b1, float b2, float eps, float grad_scale,
                                                                const float* __restrict__ scaler) {
    adam_pack_batched_body<T>(AdamGrad(), descs, n, g_off, m_off, v_off, state, b1, b2, eps, grad_scale, scaler);
}

template <typename T>
__global__ __launch_bounds__(256) void adam_pack_batched_wd_kernel(const falnet_pack_t* __restrict__ descs, int n, int64_t g_off, int64_t m_off, int64_t v_off,
                                                                   const float* __restrict__ state, float b1, float b2, float eps, float grad_scale,
                                                                   double decay, const float* __restrict__ scaler) {
    adam_pack_batched_body<T>(AdamGradL2{decay}, descs, n, g_off, m_off, v_off, state, b1, b2, eps, grad_scale, scaler);
}

// Sub-pixel weights of the deconv layers (conv_dma.hip: conv3x3_up2_dma_kernel): wu[co][pair][ci], pair = 4 (2 py + px) + 2 a + b
template <typename T>
__global__ __launch_bounds__(256) void pack_up2_batched_kernel(const falnet_pack_up2_t* __restrict__ descs, int n) {
    __shared__ int entry_begin[64];
    const int li = find_entry(descs, n, entry_begin);
    const falnet_pack_up2_t d = descs[li];
    const int rel = blockIdx.x - d.block_begin;
    const int ncb = d.cin_pad / 32;
    const int co0 = (rel / ncb) * 32, ci0 = (rel % ncb) * 32;
    T* wu = reinterpret_cast<T*>(d.wu);
    // one (co, ci) weight per thread and pass: its nine taps are loaded once and feed all sixteen (class, tap) sums (the first version looped over
    // the 16384 outputs of the block with up to four dependent loads each: 40 us per step for three layers)
    for (int e = threadIdx.x; e < 32 * 32; e += blockDim.x) {
        const int ci = ci0 + (e & 31), co = co0 + (e >> 5);
        float w[9];
        const bool real = co < d.cout && ci < d.cin;
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = real ? d.w[((int64_t)co * d.cin + ci) * 9 + t] : 0.f;
#pragma unroll
        for (int pair = 0; pair < 16; ++pair) {
            const int cls = pair >> 2, a = (pair >> 1) & 1, b = pair & 1, py = cls >> 1, px = cls & 1;
            // 3x3 taps that coincide on low-resolution neighbour a (rows) / b (columns) for output parity py / px
            const int ky0 = py == 0 ? (a == 0 ? 0 : 1) : (a == 0 ? 0 : 2), ky1 = py == 0 ? (a == 0 ? 0 : 2) : (a == 0 ? 1 : 2);
            const int kx0 = px == 0 ? (b == 0 ? 0 : 1) : (b == 0 ? 0 : 2), kx1 = px == 0 ? (b == 0 ? 0 : 2) : (b == 0 ? 1 : 2);
            float v = 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    if (ky >= ky0 && ky <= ky1 && kx >= kx0 && kx <= kx1) v += w[ky * 3 + kx];
            wu[((int64_t)co * 16 + pair) * d.cin_pad + ci] = from_f32<T>(v);
        }
        if (d.wdd) {
            // data-gradient form on the low-resolution grid (conv_dma.hip: conv2x2_up2d_dma16_kernel): wdd[ci][2 du + dv][e 2 Cp + f Cp + co], the
            // coefficient of upstream pixel (2 (i + du) - 1 + e, 2 (j + dv) - 1 + f) in input position (i, j): per axis t = 2 d + parity selects the
            // 3x3 taps {2}, {1, 2}, {0, 1}, {0}
            T* wdd = reinterpret_cast<T*>(d.wdd);
#pragma unroll
            for (int tap = 0; tap < 4; ++tap)
#pragma unroll
                for (int ef = 0; ef < 4; ++ef) {
                    const int ty = 2 * (tap >> 1) + (ef >> 1), tx = 2 * (tap & 1) + (ef & 1);
                    const int ky0 = ty == 0 ? 2 : (ty == 1 ? 1 : 0), ky1 = ty == 0 ? 2 : (ty == 1 ? 2 : (ty == 2 ? 1 : 0));
                    const int kx0 = tx == 0 ? 2 : (tx == 1 ? 1 : 0), kx1 = tx == 0 ? 2 : (tx == 1 ? 2 : (tx == 2 ? 1 : 0));
                    float v = 0.f;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx)
                            if (ky >= ky0 && ky <= ky1 && kx >= kx0 && kx <= kx1) v += w[ky * 3 + kx];
                    wdd[((int64_t)ci * 4 + tap) * (4 * d.cout_pad) + ef * d.cout_pad + co] = from_f32<T>(v);
                }
        }
    }
}

// OIHW f32 -> packed operands (see falnet_hip.h)
template <typename T>
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w, int cout, int cin, int taps,
                                                           int c0_real, int c0_pad, int cin_pad, int cout_pad,
                                                           T* __restrict__ wf, T* __restrict__ wd) {
    const int64_t total = (int64_t)cout_pad * taps * cin_pad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cp = (int)(i % cin_pad), t = (int)((i / cin_pad) % taps), co = (int)(i / ((int64_t)cin_pad * taps));
        int ci = -1;
        if (cp < c0_pad) {
            if (cp < c0_real) ci = cp;
        } else if (c0_real + (cp - c0_pad) < cin) {
            ci = c0_real + (cp - c0_pad);
        }
        const float v = (co < cout && ci >= 0) ? w[((int64_t)co * cin + ci) * taps + t] : 0.f;
        if (wf) wf[i] = from_f32<T>(v);
        if (wd) wd[((int64_t)cp * taps + t) * cout_pad + co] = from_f32<T>(v);
    }
}

extern "C" int falnet_pack_up2_batched(const falnet_pack_up2_t* descs_dev, int n, int total_blocks, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(descs_dev && n > 0 && n <= 64 && total_blocks > 0, "pack_up2_batched: bad argument");
    FALNET_CHECK_ARG(dtype == FALNET_BF16 || dtype == FALNET_F16, "pack_up2_batched: 16-bit operand types only");
#define PACKU_L(T) hipLaunchKernelGGL(pack_up2_batched_kernel<T>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n)
    FALNET_DISPATCH_16(dtype, PACKU_L);
#undef PACKU_L
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_pack_weights_batched(const falnet_pack_t* descs_dev, int n, int total_blocks, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(descs_dev && n > 0 && n <= 64 && total_blocks > 0, "pack_weights_batched: bad argument (taps must be 9, 3 or 1, n <= 64)");
#define PACK_B(T) hipLaunchKernelGGL(pack_weights_batched_kernel<T>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n)
    FALNET_DISPATCH_DTYPE(dtype, PACK_B);
#undef PACK_B
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_adam_pack_batched(const falnet_pack_t* descs_dev, int n, int total_blocks, int dtype, int64_t g_off, int64_t m_off, int64_t v_off,
                                        const float* state, float b1, float b2, float eps, float grad_scale, const float* scaler, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(descs_dev && n > 0 && n <= 64 && total_blocks > 0 && state, "adam_pack_batched: bad argument (n <= 64)");
    FALNET_CHECK_ARG(g_off != 0 && m_off != 0 && v_off != 0 && g_off != m_off && g_off != v_off && m_off != v_off,
                     "adam_pack_batched: gradient / moment buffers must be distinct from the weights and from each other");
#define APACK_B(T) hipLaunchKernelGGL(adam_pack_batched_kernel<T>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n, g_off, m_off, v_off, \
                                      state, b1, b2, eps, grad_scale, scaler)
    FALNET_DISPATCH_DTYPE(dtype, APACK_B);
#undef APACK_B
    FALNET_RETURN_LAUNCH();
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

extern "C" int falnet_pack_weights(const float* w_oihw, int cout, int cin, int taps, int c0_real, int c0_pad,
                                   int cin_pad_total, int cout_pad, void* wf, void* wd, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(w_oihw && (wf || wd) && cout > 0 && cin > 0 && taps >= 1, "pack_weights: bad argument");
    FALNET_CHECK_ARG(cout_pad >= cout && cout_pad % 32 == 0 && cin_pad_total % 32 == 0, "pack_weights: pads must be multiples of 32");
    FALNET_CHECK_ARG(c0_real <= cin && c0_real <= c0_pad && c0_pad + (cin - c0_real) <= cin_pad_total, "pack_weights: channel groups do not fit");
    const int64_t total = (int64_t)cout_pad * taps * cin_pad_total;
    const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
#define PACK_L(T) hipLaunchKernelGGL(pack_weights_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w_oihw, cout, cin, taps, \
                                   c0_real, c0_pad, cin_pad_total, cout_pad, (T*)wf, (T*)wd)
    FALNET_DISPATCH_DTYPE(dtype, PACK_L);
#undef PACK_L
    FALNET_RETURN_LAUNCH();
}
