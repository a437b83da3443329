// Layout / resampling kernels around the NHWC conv stacks (gfx950, HBM-bound streaming).
//   nchw_to_nhwc / nhwc_to_nchw : boundary between the reference's planar f32 API and the pixel-major
//                                 compute layout (FAL_netB.py:200 input; loss_functions.py:36 VGG input)
//   upsample_bwd                : adjoint of F.interpolate(mode='nearest') (FAL_netB.py:58)
//   maxpool2 fwd/bwd            : torchvision VGG19 features[4,9,18] (loss_functions.py:21-29)
#include <stdlib.h>
#include "common.h"

#define EW_THREADS 256
static inline int ew_grid(int64_t n) {
    int64_t g = (n + EW_THREADS - 1) / EW_THREADS;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

__device__ __forceinline__ void store8_as(float* p, const float (&v)[8]) {
    reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
template <typename T>  // 16-bit operand types
__device__ __forceinline__ void store8_as(T* p, const float (&v)[8]) {
    uint4 q;
#pragma unroll
    for (int i = 0; i < 4; ++i) (&q.x)[i] = pack16x2<T>(v[2 * i], v[2 * i + 1]);
    *reinterpret_cast<uint4*>(p) = q;
}
__device__ __forceinline__ void load8_as(const float* p, float (&v)[8]) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <typename T>  // 16-bit operand types
__device__ __forceinline__ void load8_as(const T* p, float (&v)[8]) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned w = (&q.x)[i];
        v[2 * i] = H16<T>::lo(w);
        v[2 * i + 1] = H16<T>::hi(w);
    }
}

// planar f32 -> NHWC T.  A 64-pixel x Cpad tile goes through LDS so that both the planar reads
// (64 consecutive pixels per channel) and the NHWC writes (Cpad contiguous per pixel) are coalesced.
template <typename T>
__global__ __launch_bounds__(EW_THREADS) void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst,
                                                                  int C, int64_t HW, int Cpad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tile = reinterpret_cast<float*>(smem);  // [64][Cpad+1]
    const int b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int ld = Cpad + 1;
    for (int i = threadIdx.x; i < 64 * Cpad; i += blockDim.x) {
        const int c = i >> 6, px = i & 63;
        const int64_t p = p0 + px;
        tile[px * ld + c] = (c < C && p < HW) ? src[((int64_t)b * C + c) * HW + p] : 0.f;
    }
    __syncthreads();
    if (Cpad % 8 == 0) {  // 8 channels (16 B bf16 / 32 B f32) per thread
        const int cg = Cpad / 8;
        for (int i = threadIdx.x; i < 64 * cg; i += blockDim.x) {
            const int px = i / cg, c0 = (i % cg) * 8;
            const int64_t p = p0 + px;
            if (p < HW) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = tile[px * ld + c0 + j];
                store8_as(dst + ((int64_t)b * HW + p) * Cpad + c0, v);
            }
        }
        return;
    }
    for (int i = threadIdx.x; i < 64 * Cpad; i += blockDim.x) {
        const int px = i / Cpad, c = i % Cpad;
        const int64_t p = p0 + px;
        if (p < HW) dst[((int64_t)b * HW + p) * Cpad + c] = from_f32<T>(tile[px * ld + c]);
    }
}

template <typename T>
__global__ __launch_bounds__(EW_THREADS) void nhwc_to_nchw_kernel(const T* __restrict__ src, float* __restrict__ dst,
                                                                  int C, int64_t HW, int Cpad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tile = reinterpret_cast<float*>(smem);  // [64][Cpad+1]
    const int b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int ld = Cpad + 1;
    for (int i = threadIdx.x; i < 64 * Cpad; i += blockDim.x) {
        const int px = i / Cpad, c = i % Cpad;
        const int64_t p = p0 + px;
        tile[px * ld + c] = p < HW ? to_f32(src[((int64_t)b * HW + p) * Cpad + c]) : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * C; i += blockDim.x) {
        const int c = i >> 6, px = i & 63;
        const int64_t p = p0 + px;
        if (p < HW) dst[((int64_t)b * C + c) * HW + p] = tile[px * ld + c];
    }
}

__device__ __forceinline__ float elu_grad_from_out(float y) { return y > 0.f ? 1.f : y + 1.f; }  // alpha = 1

// nearest-upsample adjoint: source pixel (sy,sx) owns virtual rows [ceil(sy*IH/H), ceil((sy+1)*IH/H)) (the
// set {vy : floor(vy*H/IH) == sy}); gather form, no atomics.  8 channels (one 16-B bf16 / two f32 vec) per thread.
template <typename T>
__global__ __launch_bounds__(EW_THREADS) void upsample_bwd_kernel(const T* __restrict__ gup, T* __restrict__ gsrc,
                                                                  const T* __restrict__ actout, int B, int IH, int IW,
                                                                  int H, int W, int C) {
    const int cg = C / 8;
    const int64_t total = (int64_t)B * H * W * cg;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cg) * 8;
        const int sx = (int)((i / cg) % W), sy = (int)((i / ((int64_t)cg * W)) % H), b = (int)(i / ((int64_t)cg * W * H));
        const int vy0 = (sy * IH + H - 1) / H, vy1 = ((sy + 1) * IH + H - 1) / H;
        const int vx0 = (sx * IW + W - 1) / W, vx1 = ((sx + 1) * IW + W - 1) / W;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int vy = vy0; vy < vy1; ++vy)
            for (int vx = vx0; vx < vx1; ++vx) {
                const T* g = gup + (((int64_t)b * IH + vy) * IW + vx) * C + c0;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += to_f32(g[j]);
            }
        const int64_t o = (((int64_t)b * H + sy) * W + sx) * C + c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = acc[j];
            if (actout) v *= elu_grad_from_out(to_f32(actout[o + j]));
            gsrc[o + j] = from_f32<T>(v);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(EW_THREADS) void maxpool2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H,
                                                                  int W, int C) {
    const int OH = H / 2, OW = W / 2;
    const int64_t total = (int64_t)B * OH * OW * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C), ox = (int)((i / C) % OW), oy = (int)((i / ((int64_t)C * OW)) % OH);
        const int b = (int)(i / ((int64_t)C * OW * OH));
        const T* p = x + (((int64_t)b * H + 2 * oy) * W + 2 * ox) * C + c;
        const float v = fmaxf(fmaxf(to_f32(p[0]), to_f32(p[C])), fmaxf(to_f32(p[(int64_t)W * C]), to_f32(p[(int64_t)W * C + C])));
        y[i] = from_f32<T>(v);
    }
}

// gx = gy routed to the FIRST max of the window in row-major order (aten max_pool2d_with_indices
// tie rule), times relu'(x) (x is the ReLU output feeding the pool; x == 0 gets no gradient).
template <typename T>
__global__ __launch_bounds__(EW_THREADS) void maxpool2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ gy,
                                                                  T* __restrict__ gx, int B, int H, int W, int C) {
    const int OH = H / 2, OW = W / 2;
    const int64_t total = (int64_t)B * OH * OW * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C), ox = (int)((i / C) % OW), oy = (int)((i / ((int64_t)C * OW)) % OH);
        const int b = (int)(i / ((int64_t)C * OW * OH));
        const int64_t base = (((int64_t)b * H + 2 * oy) * W + 2 * ox) * C + c;
        const int64_t off[4] = {0, C, (int64_t)W * C, (int64_t)W * C + C};
        float best = to_f32(x[base]);
        int arg = 0;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const float v = to_f32(x[base + off[j]]);
            if (v > best) {
                best = v;
                arg = j;
            }
        }
        const float g = best > 0.f ? to_f32(gy[i]) : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) gx[base + off[j]] = from_f32<T>(j == arg ? g : 0.f);
    }
}

// 8 channels per thread (C % 8 == 0): 16-B loads / stores
template <typename T>
__global__ __launch_bounds__(EW_THREADS) void maxpool2_bwd_vec_kernel(const T* __restrict__ x, const T* __restrict__ gy,
                                                                      T* __restrict__ gx, int B, int H, int W, int C) {
    const int OH = H / 2, OW = W / 2, cg = C / 8;
    const int64_t total = (int64_t)B * OH * OW * cg;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cg) * 8, ox = (int)((i / cg) % OW), oy = (int)((i / ((int64_t)cg * OW)) % OH);
        const int b = (int)(i / ((int64_t)cg * OW * OH));
        const int64_t base = (((int64_t)b * H + 2 * oy) * W + 2 * ox) * C + c0;
        const int64_t off[4] = {0, C, (int64_t)W * C, (int64_t)W * C + C};
        float xv[4][8], g[8], o[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j) load8_as(x + base + off[j], xv[j]);
        load8_as(gy + (((int64_t)b * OH + oy) * OW + ox) * C + c0, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float best = xv[0][e];
            int arg = 0;
#pragma unroll
            for (int j = 1; j < 4; ++j)
                if (xv[j][e] > best) {
                    best = xv[j][e];
                    arg = j;
                }
            const float ge = best > 0.f ? g[e] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j][e] = j == arg ? ge : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) store8_as(gx + base + off[j], o[j]);
    }
}

// The same routing from the 4-bit argmax codes the fused pool wrote (falnet_conv_t::pool_code: one-hot nibble, bit 2 * row + column of the winner,
// 0 = no gradient; channel c of a pooled pixel in byte c / 2, low nibble for even c): the full-resolution map is neither kept nor re-read.
// One thread = 8 channels of one window: 4 B of codes, 16 B of gy (two for f32), four 16-B stores -- every element of gx is written.
template <typename T>
__global__ __launch_bounds__(EW_THREADS) void maxpool2_bwd_codes_kernel(const unsigned char* __restrict__ codes, const T* __restrict__ gy,
                                                                        T* __restrict__ gx, int B, int H, int W, int C) {
    const int OH = H / 2, OW = W / 2, cg = C / 8;
    const int64_t total = (int64_t)B * OH * OW * cg;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cg) * 8, ox = (int)((i / cg) % OW), oy = (int)((i / ((int64_t)cg * OW)) % OH);
        const int b = (int)(i / ((int64_t)cg * OW * OH));
        const int64_t base = (((int64_t)b * H + 2 * oy) * W + 2 * ox) * C + c0;
        const int64_t off[4] = {0, C, (int64_t)W * C, (int64_t)W * C + C};
        const unsigned code = *reinterpret_cast<const unsigned*>(codes + i * 4);  // (i enumerates (pooled pixel, 8-channel group) in memory order)
        float g[8], o[4][8];
        load8_as(gy + (((int64_t)b * OH + oy) * OW + ox) * C + c0, g);
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j][e] = ((code >> (4 * e + j)) & 1u) ? g[e] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) store8_as(gx + base + off[j], o[j]);
    }
}

template <typename T>
__global__ __launch_bounds__(EW_THREADS) void act_bwd_kernel(const T* __restrict__ g, const T* __restrict__ y,
                                                             T* __restrict__ gx, int64_t n, int kind) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float yy = to_f32(y[i]);
        const float d = kind == FALNET_ACT_RELU ? (yy > 0.f ? 1.f : 0.f) : elu_grad_from_out(yy);
        gx[i] = from_f32<T>(to_f32(g[i]) * d);
    }
}


extern "C" int falnet_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int Cpad, int dtype,
                                   void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && Cpad >= C && Cpad <= 512, "nchw_to_nhwc: bad argument");
    const int64_t HW = (int64_t)H * W;
    const dim3 grid((unsigned)((HW + 63) / 64), B);
    const size_t lds = (size_t)64 * (Cpad + 1) * sizeof(float);
#define EW_L(T) hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, grid, dim3(EW_THREADS), lds, (hipStream_t)stream, src, (T*)dst, C, HW, Cpad)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int Cpad, int dtype,
                                   void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(src && dst && B > 0 && C > 0 && H > 0 && W > 0 && Cpad >= C && Cpad <= 512, "nhwc_to_nchw: bad argument");
    const int64_t HW = (int64_t)H * W;
    const dim3 grid((unsigned)((HW + 63) / 64), B);
    const size_t lds = (size_t)64 * (Cpad + 1) * sizeof(float);
#define EW_L(T) hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, grid, dim3(EW_THREADS), lds, (hipStream_t)stream, (const T*)src, dst, C, HW, Cpad)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_upsample_bwd(const void* gup, void* gsrc, const void* actout, int B, int IH, int IW, int H, int W,
                                   int C, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(gup && gsrc && B > 0 && IH >= H && IW >= W && H > 0 && W > 0 && C % 8 == 0, "upsample_bwd: bad argument");
    // the kernel's row / column ranges ((s + 1) * I + S - 1) / S are 32-bit products
    FALNET_CHECK_ARG((int64_t)H * IH + H <= INT32_MAX && (int64_t)W * IW + W <= INT32_MAX, "upsample_bwd: %dx%d -> %dx%d too large for 32-bit index ranges", H, W, IH, IW);
    const int64_t total = (int64_t)B * H * W * (C / 8);
#define EW_L(T) hipLaunchKernelGGL(upsample_bwd_kernel<T>, dim3(ew_grid(total)), dim3(EW_THREADS), 0, (hipStream_t)stream, (const T*)gup, (T*)gsrc, (const T*)actout, B, IH, IW, H, W, C)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

// ---- weight gradient of a 3x3 conv (pad 1, stride 1 or 2) with respect to a PER-SAMPLE CONSTANT input plane ---------------------------
// The `flow` input of conv1 (FAL_netB.py:208-209,101: max_disp / 100 broadcast over the image) is one value f_b per sample, so
//   dW[co][ky][kx] = sum_b f_b * sum_{(i,j): tap (ky,kx) in bounds} g[b][i][j][co]
// and the inner sum is the whole-image sum S minus the first / last row and column sums the tap's zero padding cuts off (inclusion-
// exclusion with the four corners).  Nine sums per (sample, channel) replace a 32-channel padded K tile of the stride-2 weight-gradient
// kernel (half of conv1's launch: 31 zero channels beside the one real one).
//   stats kernel:   ws[b][k][c] += partial sums, k = S, top row, bottom row, left col, right col, tl, tr, bl, br
//   combine kernel: one block; adds into the f32 OIHW gradient and leaves ws ZERO again (it is zero on entry by contract).
template <typename T>
__global__ __launch_bounds__(256) void const_plane_stats_kernel(const T* __restrict__ g, float* __restrict__ ws, int TH, int TW, int gC, int rows_per_block) {
    __shared__ float red[256 * 8];
    const int b = blockIdx.y, segs = gC >> 3, npl = 256 / segs;
    const int seg = threadIdx.x % segs, pl = threadIdx.x / segs;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, TH);
    float st[9][8];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) st[k][i] = 0.f;
    const bool has_top = r0 == 0, has_bot = r1 == TH;
    if (pl < npl) {
        for (int y = r0; y < r1; ++y) {
            const bool top = y == 0, bot = y == TH - 1;
            const T* row = g + (((int64_t)b * TH + y) * TW) * gC + seg * 8;
            float rs[8];  // this thread's share of the row
#pragma unroll
            for (int i = 0; i < 8; ++i) rs[i] = 0.f;
            for (int x = pl; x < TW; x += npl) {
                float v[8];
                load8_as(row + (int64_t)x * gC, v);
#pragma unroll
                for (int i = 0; i < 8; ++i) rs[i] += v[i];
                if (x == 0) {  // two pixels per row: the column sums and the corners (compile-time indices: no scratch)
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        st[3][i] += v[i];
                        if (top) st[5][i] += v[i];
                        if (bot) st[7][i] += v[i];
                    }
                }
                if (x == TW - 1) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        st[4][i] += v[i];
                        if (top) st[6][i] += v[i];
                        if (bot) st[8][i] += v[i];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                st[0][i] += rs[i];
                if (top) st[1][i] += rs[i];
                if (bot) st[2][i] += rs[i];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        if ((k == 1 || k == 5 || k == 6) && !has_top) continue;  // (block-uniform) sums this block cannot have
        if ((k == 2 || k == 7 || k == 8) && !has_bot) continue;
#pragma unroll
        for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = st[k][i];
        __syncthreads();
        if ((int)threadIdx.x < gC) {
            const int c = threadIdx.x, sg = c >> 3, i = c & 7;
            float t = 0.f;
            for (int q = 0; q < npl; ++q) t += red[(q * segs + sg) * 8 + i];
            if (t != 0.f) atomicAdd(ws + ((int64_t)b * 9 + k) * gC + c, t);
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(1024) void const_plane_combine_kernel(float* __restrict__ ws, const T* __restrict__ plane, int64_t plane_stride, float* __restrict__ grad,
                                                                   int64_t co_stride, int B, int gC, int cout, int ex_bot, int ex_rt) {
    for (int e = threadIdx.x; e < cout * 9; e += blockDim.x) {
        const int co = e / 9, tap = e - co * 9, ky = tap / 3, kx = tap - ky * 3;
        const float et = ky == 0 ? 1.f : 0.f, eb = ((ex_bot >> ky) & 1) ? 1.f : 0.f, el = kx == 0 ? 1.f : 0.f, er = ((ex_rt >> kx) & 1) ? 1.f : 0.f;
        float acc = 0.f;
        for (int b = 0; b < B; ++b) {
            const float* w = ws + (int64_t)b * 9 * gC + co;
            const float s = w[0] - et * w[gC] - eb * w[2 * gC] - el * w[3 * gC] - er * w[4 * gC] + et * el * w[5 * gC] + et * er * w[6 * gC] +
                            eb * el * w[7 * gC] + eb * er * w[8 * gC];
            acc += to_f32(plane[b * plane_stride]) * s;
        }
        atomicAdd(grad + co * co_stride + tap, acc);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < B * 9 * gC; e += blockDim.x) ws[e] = 0.f;
}

extern "C" int falnet_wgrad_const_plane(const void* gout, const void* plane, int64_t plane_stride, float* grad, int64_t grad_co_stride, float* ws, int B,
                                        int TH, int TW, int gC, int cout, int IH, int IW, int stride, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(gout && plane && grad && ws && B > 0 && TH >= 2 && TW >= 2 && gC % 8 == 0 && gC <= 256 && cout > 0 && cout <= gC,
                     "wgrad_const_plane: bad argument (B=%d TH=%d TW=%d gC=%d cout=%d)", B, TH, TW, gC, cout);
    FALNET_CHECK_ARG((stride == 1 || stride == 2) && TH == (IH + stride - 1) / stride && TW == (IW + stride - 1) / stride,
                     "wgrad_const_plane: a 3x3 pad-1 conv of stride %d maps %dx%d to %dx%d, not %dx%d", stride, IH, IW, (IH + stride - 1) / stride,
                     (IW + stride - 1) / stride, TH, TW);
    FALNET_CHECK_ARG(!falnet_deterministic(), "wgrad_const_plane adds with f32 atomics: not available in deterministic mode");
    int ex_bot = 0, ex_rt = 0;  // bit k: tap row / column k reads beyond the last input row / column from the last output row / column
    for (int k = 0; k < 3; ++k) {
        if ((TH - 1) * stride + k - 1 >= IH) ex_bot |= 1 << k;
        if ((TW - 1) * stride + k - 1 >= IW) ex_rt |= 1 << k;
    }
    const int rows_per_block = TH >= 64 ? 4 : 1;
    const dim3 grid((unsigned)((TH + rows_per_block - 1) / rows_per_block), (unsigned)B);
#define EW_L(T)                                                                                                                                         \
    hipLaunchKernelGGL(const_plane_stats_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)gout, ws, TH, TW, gC, rows_per_block);           \
    hipLaunchKernelGGL(const_plane_combine_kernel<T>, dim3(1), dim3(1024), 0, (hipStream_t)stream, ws, (const T*)plane, plane_stride, grad, grad_co_stride, \
                       B, gC, cout, ex_bot, ex_rt)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_maxpool2_fwd(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(x && y && B > 0 && H >= 2 && W >= 2 && C > 0, "maxpool2_fwd: bad argument");
    const int64_t total = (int64_t)B * (H / 2) * (W / 2) * C;
#define EW_L(T) hipLaunchKernelGGL(maxpool2_fwd_kernel<T>, dim3(ew_grid(total)), dim3(EW_THREADS), 0, (hipStream_t)stream, (const T*)x, (T*)y, B, H, W, C)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_maxpool2_bwd(const void* x, const void* y, const void* gy, void* gx, int B, int H, int W, int C,
                                   int dtype, void* stream) {
    FALNET_ENTER(stream);
    (void)y;
    FALNET_CHECK_ARG(x && gy && gx && B > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C > 0,
                     "maxpool2_bwd: bad argument (even H, W required)");
    if (C % 8 == 0 && (((uintptr_t)x | (uintptr_t)gy | (uintptr_t)gx) & 15) == 0) {
        const int64_t tv = (int64_t)B * (H / 2) * (W / 2) * (C / 8);
#define EW_L(T) hipLaunchKernelGGL(maxpool2_bwd_vec_kernel<T>, dim3(ew_grid(tv)), dim3(EW_THREADS), 0, (hipStream_t)stream, (const T*)x, (const T*)gy, (T*)gx, B, H, W, C)
        FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
        FALNET_RETURN_LAUNCH();
    }
    const int64_t total = (int64_t)B * (H / 2) * (W / 2) * C;
#define EW_L(T) hipLaunchKernelGGL(maxpool2_bwd_kernel<T>, dim3(ew_grid(total)), dim3(EW_THREADS), 0, (hipStream_t)stream, (const T*)x, (const T*)gy, (T*)gx, B, H, W, C)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_maxpool2_bwd_codes(const void* codes, const void* gy, void* gx, int B, int H, int W, int C, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(codes && gy && gx && B > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && C > 0,
                     "maxpool2_bwd_codes: bad argument (even H, W required)");
    FALNET_CHECK_ARG(dtype == FALNET_F32 || dtype == FALNET_BF16 || dtype == FALNET_F16, "maxpool2_bwd_codes: bad dtype %d", dtype);
    FALNET_CHECK_ARG(C % 8 == 0 && (((uintptr_t)gy | (uintptr_t)gx) & 15) == 0 && ((uintptr_t)codes & 3) == 0,
                     "maxpool2_bwd_codes: C must be a multiple of 8, gy / gx 16-B and codes 4-B aligned");
    const int64_t tv = (int64_t)B * (H / 2) * (W / 2) * (C / 8);
#define EW_L(T) hipLaunchKernelGGL(maxpool2_bwd_codes_kernel<T>, dim3(ew_grid(tv)), dim3(EW_THREADS), 0, (hipStream_t)stream, (const unsigned char*)codes, (const T*)gy, (T*)gx, B, H, W, C)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_act_bwd(const void* g, const void* y, void* gx, int64_t n, int kind, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(g && y && gx && n > 0, "act_bwd: bad argument");
#define EW_L(T) hipLaunchKernelGGL(act_bwd_kernel<T>, dim3(ew_grid(n)), dim3(EW_THREADS), 0, (hipStream_t)stream, (const T*)g, (const T*)y, (T*)gx, n, kind)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

// ---- small f32 matrix products (composed logits conv, FAL_netB.py:127,190: Wc = W1x1 . W3x3 per update, and the split of
// dWc back into dW3x3 = W1x1^T dWc, dW1x1 = dWc W3x3^T): N x N by N x 864 with N = 49..96 -- a few MFLOP, one thread per
// output element (the dtype of the parameters, exact f32 like the rest of the optimiser path)
__global__ __launch_bounds__(EW_THREADS) void gemm_f32_small_kernel(const float* __restrict__ A, int64_t sam, int64_t sak,
                                                                    const float* __restrict__ Bm, int64_t sbk, int64_t sbn,
                                                                    float* __restrict__ C, int M, int N, int K, int accumulate) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)M * N; i += (int64_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / N), n = (int)(i % N);
        const float* a = A + m * sam;
        const float* b = Bm + n * sbn;
        float acc = 0.f;
        int k = 0;
        for (; k + 8 <= K; k += 8) {  // eight steps' operands in flight (the runtime-bound loop alone issued one dependent pair of loads per step: 16 us for K = 49)
            float av[8], bv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                av[u] = a[(k + u) * sak];
                bv[u] = b[(k + u) * sbk];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(av[u], bv[u], acc);  // (same order of accumulation as the plain loop)
        }
        for (; k < K; ++k) acc = fmaf(a[k * sak], b[k * sbk], acc);
        C[i] = accumulate ? C[i] + acc : acc;
    }
}

// Long-K, few-outputs products (dW1x1 = dWc W3x3^T: 49 x 49 outputs, K = 864): one WAVE per output element, lanes stride over K
// (coalesced when both operands are contiguous along K) and a wave reduction -- the thread-per-output form walked K serially with
// two uncoalesced loads per step on 10 workgroups: 140 us on the weight-gradient stream of every training step, now ~5 us.
__global__ __launch_bounds__(EW_THREADS) void gemm_f32_small_wave_kernel(const float* __restrict__ A, int64_t sam, int64_t sak,
                                                                         const float* __restrict__ Bm, int64_t sbk, int64_t sbn,
                                                                         float* __restrict__ C, int M, int N, int K, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < (int64_t)M * N; i += nwaves) {
        const int m = (int)(i / N), n = (int)(i % N);
        const float* a = A + m * sam;
        const float* b = Bm + n * sbn;
        float acc = 0.f;
        for (int k = lane; k < K; k += 64) acc = fmaf(a[k * sak], b[k * sbk], acc);
        acc = wave_sum(acc);
        if (lane == 0) C[i] = accumulate ? C[i] + acc : acc;
    }
}

extern "C" int falnet_gemm_f32_small(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C,
                                     int M, int N, int K, int accumulate, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(A && B && C && M > 0 && N > 0 && K > 0 && (int64_t)M * N * K <= (1ll << 32), "gemm_f32_small: bad argument (small products only)");
    static const bool wave_form = [] { const char* e = falnet_ab_env("FALNET_GEMM_WAVE"); return !(e && e[0] == '0'); }();
    if (wave_form && K >= 256 && (int64_t)M * N <= 65536) {
        const int64_t waves = (int64_t)M * N;
        hipLaunchKernelGGL(gemm_f32_small_wave_kernel, dim3((unsigned)((waves + 3) / 4 > 4096 ? 4096 : (waves + 3) / 4)), dim3(EW_THREADS), 0,
                           (hipStream_t)stream, A, sam, sak, B, sbk, sbn, C, M, N, K, accumulate);
        FALNET_RETURN_LAUNCH();
    }
    hipLaunchKernelGGL(gemm_f32_small_kernel, dim3(ew_grid((int64_t)M * N)), dim3(EW_THREADS), 0, (hipStream_t)stream, A, sam, sak, B, sbk, sbn, C,
                       M, N, K, accumulate);
    FALNET_RETURN_LAUNCH();
}

// ---- planar f32 resampling of Test_KITTI.py:287-300 (ms_pp): bilinear with align_corners=True (F.interpolate semantics:
// src = dst * (in - 1) / (out - 1)) and nearest (src = floor(dst * in / out)), one thread per output element
__global__ __launch_bounds__(EW_THREADS) void resize_planar_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int W,
                                                                   int OH, int OW, int bilinear, float scale, int64_t total) {
    const float ry = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f, rx = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
    const float ny = (float)H / (float)OH, nx = (float)W / (float)OW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
        const float* pl = src + (i / ((int64_t)OW * OH)) * ((int64_t)H * W);
        float v;
        if (bilinear) {
            const float fy = ry * oy, fx = rx * ox;
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
            const float wy = fy - y0, wx = fx - x0;
            v = (1.f - wy) * ((1.f - wx) * pl[(int64_t)y0 * W + x0] + wx * pl[(int64_t)y0 * W + x1]) +
                wy * ((1.f - wx) * pl[(int64_t)y1 * W + x0] + wx * pl[(int64_t)y1 * W + x1]);
        } else {
            const int sy = min((int)floorf(oy * ny), H - 1), sx = min((int)floorf(ox * nx), W - 1);
            v = pl[(int64_t)sy * W + sx];
        }
        dst[i] = v * scale;
    }
}

extern "C" int falnet_resize_planar(const float* src, float* dst, int64_t planes, int H, int W, int OH, int OW, int bilinear, float scale,
                                    void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(src && dst && planes > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "resize_planar: bad argument");
    const int64_t total = planes * OH * OW;
    hipLaunchKernelGGL(resize_planar_kernel, dim3(ew_grid(total)), dim3(EW_THREADS), 0, (hipStream_t)stream, src, dst, H, W, OH, OW, bilinear, scale, total);
    FALNET_RETURN_LAUNCH();
}

// ---------------------------------------------------------------------------------------- disparity-range prologue
// Per-sample scalars of one step in ONE launch (Train_Stage1_K.py:237, FAL_netB.py:208-209): min_disp = max_disp * mul / div,
// the plan's copies of both, and the constant `flow` input plane max_disp / 100 in the compute dtype.
template <typename T>
__global__ void disp_prologue_kernel(const float* __restrict__ max_disp, const float* __restrict__ min_disp, float mul, float div,
                                     float* __restrict__ min_out, float* __restrict__ max_out, T* __restrict__ flow, int flow_stride, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float mx = max_disp[b];
    min_out[b] = min_disp ? min_disp[b] : mx * mul / div;
    max_out[b] = mx;
    flow[(int64_t)b * flow_stride] = from_f32<T>(mx / 100.0f);
}

extern "C" int falnet_disp_prologue(const float* max_disp, const float* min_disp, float mul, float div, float* min_out, float* max_out,
                                    void* flow, int flow_stride, int B, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(max_disp && min_out && max_out && flow && B > 0 && flow_stride > 0 && (min_disp || div != 0.0f), "disp_prologue: bad argument");
#define EW_L(T) hipLaunchKernelGGL(disp_prologue_kernel<T>, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, max_disp, min_disp, mul, div, min_out, max_out, (T*)flow, flow_stride, B)
    FALNET_DISPATCH_DTYPE(dtype, EW_L);
#undef EW_L
    FALNET_RETURN_LAUNCH();
}

// ---- stream self-test probe (include/falnet_hip.h: falnet_spin) -----------------------------------------------------------------------
__global__ void spin_kernel(long long ticks) {
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    while ((long long)__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
extern "C" int falnet_spin(int microseconds, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(microseconds >= 0 && microseconds <= 100000, "spin: 0..100000 us");
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long)microseconds * 100);
    FALNET_RETURN_LAUNCH();
}

// ---- what the board sustains on the matrix pipe (include/falnet_hip.h: falnet_mfma_probe) -------------------------------------------------
// A register-resident v_mfma_f32_16x16x32 loop: every wave keeps four A and four B fragments (16 x 32 values of `ab` each, the caller's data:
// random for the ceiling under real switching activity, zeros for the clock-bound one) and sixteen independent accumulators, and issues
// `iters` x 16 MFMAs back to back -- no LDS, no memory traffic inside the loop.  bench.py times it after ~0.2 s of back-to-back launches (the
// power controller's settling time) and reports the rate beside the dense peak: the dominant convolution's 128 / 256-channel launches run at the
// board's 1 400 W cap (profiles/r05_power_probe.txt), where no kernel reaches the 2.5 PFLOP/s of the data sheet.
template <typename T>
__global__ __launch_bounds__(256, 2) void mfma_probe_kernel(const T* __restrict__ ab, float* __restrict__ out, int iters) {
    const int lane = threadIdx.x & 63, wave = (blockIdx.x * 4 + (threadIdx.x >> 6)) & 63;
    s16x8_t a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[k] = *reinterpret_cast<const s16x8_t*>(ab + ((size_t)(wave * 8 + k) * 64 + lane) * 8);
        b[k] = *reinterpret_cast<const s16x8_t*>(ab + ((size_t)(wave * 8 + 4 + k) * 64 + lane) * 8);
    }
    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = H16<T>::mma16(a[i], b[j], acc[i][j]);
    }
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
    if (sum == 123.456f) out[0] = sum;  // (keeps the loop alive; never true on finite data)
}
extern "C" int falnet_mfma_probe(const void* ab, float* out, int iters, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(ab && out && iters > 0 && (dtype == FALNET_BF16 || dtype == FALNET_F16), "mfma_probe: 16-bit operands (64 x 8 x 64 x 8 values), iters > 0");
    // 2 048 workgroups of four waves: eight per CU over the launch, two waves per SIMD resident (launch bounds), as the convolution kernels run
    if (dtype == FALNET_BF16) hipLaunchKernelGGL(mfma_probe_kernel<bf16_t>, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)ab, out, iters);
    else hipLaunchKernelGGL(mfma_probe_kernel<f16_t>, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const f16_t*)ab, out, iters);
    FALNET_RETURN_LAUNCH();
}

