// Test-time outputs computed on the device (reference Test_KITTI.py:211-253,303-317, myUtils.py:339-394): an exact per-sample percentile,
// the plasma-coloured disparity image, 8-bit images / feature maps, the local normalisation and the point cloud.
//
// Every kernel is a single HBM-bound pass over planar f32 maps as the model returns them.  Two rules hold throughout:
//   * the arithmetic the host would do in f32 is done here in f32 in the SAME order, with correctly rounded division and square root and
//     NO fused multiply-add (this file is compiled with -ffp-contract=off; the explicit __f*_rn spell the order out where it matters), so an
//     8-bit output equals numpy's byte for byte;
//   * byte outputs are assembled in registers and leave as whole dwords: a thread owns dword d of the flat output, i.e. bytes 4 d .. 4 d + 3,
//     whatever pixels / channels they belong to.  The caller rounds the allocation up to a multiple of 4 bytes; the pad bytes are written 0.
// None of this is on the training step's path and none of it is part of the autotune key (ops.py: _TUNE_SOURCES).
#include "common.h"
#include "ordered.h"
#include "pc_vertex.h"

// ---- exact percentile: radix select over the monotone integer image of the floats -----------------------------------------------------
// key_f32(x) (ordered.h) is monotone in x (negative floats: all bits flipped; others: sign bit set), so the k-th smallest float is the k-th
// smallest key.
// Four passes of 8 bits, most significant first.  A pass histograms the next byte of every element whose higher bytes equal the prefix found
// so far (LDS histogram per workgroup, then integer atomics into the sample's 256-bin table: integer sums, so the result does not depend on
// arrival order), and a one-workgroup kernel per sample walks the table to the bin that holds the wanted rank.  TWO ranks are tracked at once
// (the order statistics floor(pos) and ceil(pos) of numpy's linear definition): slot 0 and slot 1 of every table.
//
// Workspace, per sample, in 32-bit words: [0] prefix of slot 0, [1] prefix of slot 1, [2] [3] ranks still to skip inside those prefixes,
// [4] [5] the two order statistics as f32 (valid after the call), [6] [7] unused, then 4 passes x 2 slots x 256 bins.
#define PCT_STATE 8
#define PCT_WORDS (PCT_STATE + 4 * 2 * 256)

__global__ __launch_bounds__(256) void percentile_hist_kernel(const float* __restrict__ x, uint32_t n, uint32_t* ws, int pass) {
    __shared__ uint32_t hist[2][256];
    uint32_t* w = ws + (size_t)blockIdx.y * PCT_WORDS;
    hist[0][threadIdx.x] = 0;
    hist[1][threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    // pass 0 has no prefix yet: every element counts (a shift by 32 is not defined, hence the flag)
    const bool all = pass == 0;
    const uint32_t p0 = all ? 0 : w[0], p1 = all ? 0 : w[1];
    const float* xs = x + (size_t)blockIdx.y * n;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t k = key_f32(xs[i]);
        const uint32_t hi = all ? 0 : (k >> (shift + 8)), bin = (k >> shift) & 255u;
        if (hi == p0) atomicAdd(&hist[0][bin], 1u);
        if (hi == p1) atomicAdd(&hist[1][bin], 1u);
    }
    __syncthreads();
    uint32_t* table = w + PCT_STATE + pass * 512;
    const uint32_t c0 = hist[0][threadIdx.x], c1 = hist[1][threadIdx.x];
    if (c0) atomicAdd(&table[threadIdx.x], c0);
    if (c1) atomicAdd(&table[256 + threadIdx.x], c1);
}

// one workgroup of 128 threads per sample: wave 0 resolves slot 0, wave 1 slot 1 (lane 0 of each walks the 256 bins)
__global__ __launch_bounds__(128) void percentile_select_kernel(uint32_t* ws, int pass, uint32_t rank_lo, uint32_t rank_hi, double frac, float* __restrict__ out) {
    __shared__ uint32_t cnt[2][256];
    __shared__ float stat[2];
    uint32_t* w = ws + (size_t)blockIdx.x * PCT_WORDS;
    const uint32_t* table = w + PCT_STATE + pass * 512;
    for (int i = threadIdx.x; i < 512; i += 128) cnt[i >> 8][i & 255] = table[i];
    __syncthreads();
    const int slot = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        uint32_t rank = pass == 0 ? (slot ? rank_hi : rank_lo) : w[2 + slot];
        uint32_t bin = 0;
        // the counts of a slot sum to more than `rank` (rank < n in pass 0, rank < the count of the chosen bin from then on)
        for (; bin < 255 && rank >= cnt[slot][bin]; ++bin) rank -= cnt[slot][bin];
        const uint32_t prefix = ((pass == 0 ? 0u : w[slot]) << 8) | bin;
        w[slot] = prefix;
        w[2 + slot] = rank;
        if (pass == 3) {
            stat[slot] = unkey_f32(prefix);
            w[4 + slot] = __float_as_uint(stat[slot]);
        }
    }
    if (pass != 3) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double a = (double)stat[0], b = (double)stat[1];
        out[blockIdx.x] = (float)(a + (b - a) * frac);  // one interpolation, in double, rounded once
    }
}

extern "C" int64_t falnet_percentile_workspace_bytes(int B) { return B > 0 ? (int64_t)B * PCT_WORDS * 4 : 0; }

extern "C" int falnet_percentile_f32(const float* x, int64_t n_per_sample, int B, double q, float* out, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(x && out && workspace && B > 0 && B <= 65535, "percentile_f32: bad argument (1 <= B <= 65535)");
    FALNET_CHECK_ARG(n_per_sample > 0 && n_per_sample < ((int64_t)1 << 31), "percentile_f32: n_per_sample must be in [1, 2^31)");
    FALNET_CHECK_ARG(q >= 0.0 && q <= 100.0, "percentile_f32: q must be in [0, 100]");
    // numpy's default ('linear') definition: position q/100 (n - 1), interpolate between the order statistics on either side of it
    const double pos = q / 100.0 * (double)(n_per_sample - 1);
    int64_t lo = (int64_t)pos;
    if (lo > n_per_sample - 1) lo = n_per_sample - 1;
    const double frac = pos - (double)lo;
    const int64_t hi = (frac > 0.0 && lo + 1 < n_per_sample) ? lo + 1 : lo;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)falnet_percentile_workspace_bytes(B), (hipStream_t)stream);
    if (e != hipSuccess) {
        falnet_set_error("percentile_f32: clearing the workspace failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    int64_t blocks = (n_per_sample + 256 * 8 - 1) / (256 * 8);  // >= 8 elements per thread, at most 256 workgroups per sample
    if (blocks > 256) blocks = 256;
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(percentile_hist_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, x, (uint32_t)n_per_sample,
                           (uint32_t*)workspace, pass);
        hipLaunchKernelGGL(percentile_select_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, (uint32_t*)workspace, pass, (uint32_t)lo, (uint32_t)hi,
                           frac, out);
    }
    FALNET_RETURN_LAUNCH();
}

// ---- 8-bit outputs ---------------------------------------------------------------------------------------------------------------------
// rint of a value already clipped to [0, 255] -> byte (round half to even, like np.rint)
__device__ __forceinline__ uint32_t sat_rint_u8(float v) {
    v = rintf(v);
    return v >= 255.f ? 255u : (v > 0.f ? (uint32_t)v : 0u);  // NaN -> 0
}

// Test_KITTI.py:213-216: v = 256 clip(d / (p95 + 1e-6), 0, 1); k = min(rint(v), 255); out = lut[k] (one RGBA dword per pixel)
__global__ __launch_bounds__(256) void disp_to_plasma_kernel(const float* __restrict__ disp, const float* __restrict__ p95, const uint32_t* __restrict__ lut,
                                                             uint32_t* __restrict__ out, uint32_t n, uint32_t total) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const float den = __fadd_rn(p95[i / n], 1e-6f);
        float r = __fdiv_rn(disp[i], den);  // correctly rounded: the table index must be numpy's
        r = fminf(fmaxf(r, 0.f), 1.f);      // np.clip (NaN -> 0)
        const float k = fminf(rintf(256.f * r), 255.f);
        out[i] = tab[(uint32_t)k];
    }
}

extern "C" int falnet_disp_to_plasma_u8(const float* disp, const float* p95, const void* lut_rgba, void* out_rgba, int B, int H, int W, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(disp && p95 && lut_rgba && out_rgba && B > 0 && H > 0 && W > 0, "disp_to_plasma_u8: bad argument");
    FALNET_CHECK_ARG((int64_t)B * H * W < ((int64_t)1 << 31), "disp_to_plasma_u8: more than 2^31 pixels");
    FALNET_CHECK_ARG(((uintptr_t)lut_rgba & 3) == 0 && ((uintptr_t)out_rgba & 3) == 0, "disp_to_plasma_u8: table and output must be 4-byte aligned");
    const uint32_t n = (uint32_t)H * W, total = n * B;
    const uint32_t blocks = (total + 1023) / 1024 < 2048 ? (total + 1023) / 1024 : 2048;
    hipLaunchKernelGGL(disp_to_plasma_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, disp, p95, (const uint32_t*)lut_rgba, (uint32_t*)out_rgba, n,
                       total);
    FALNET_RETURN_LAUNCH();
}

// Test_KITTI.py:229-241: rint(255 (x + mean)) -> u8 (saturated, where the reference's astype(uint8) wraps), planar (B,3,H,W) -> (B,H,W,3).
// Thread = one output dword = flat bytes 4 d .. 4 d + 3; byte j is channel j % 3 of pixel j / 3 (pixels counted across the batch).
__global__ __launch_bounds__(256) void image_to_u8_kernel(const float* __restrict__ x, float m0, float m1, float m2, uint32_t* __restrict__ out, uint32_t hw,
                                                          uint32_t total_bytes) {
    const uint32_t ndw = (total_bytes + 3) / 4;
    for (uint32_t d = blockIdx.x * 256u + threadIdx.x; d < ndw; d += gridDim.x * 256u) {
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t j = 4 * d + k;
            if (j < total_bytes) {
                const uint32_t g = j / 3, c = j - 3 * g, b = g / hw, pix = g - b * hw;
                const float v = x[((size_t)b * 3 + c) * hw + pix];
                const float s = __fmul_rn(255.f, __fadd_rn(v, c == 0 ? m0 : (c == 1 ? m1 : m2)));
                word |= sat_rint_u8(fminf(fmaxf(s, 0.f), 255.f)) << (8 * k);
            }
        }
        out[d] = word;
    }
}

extern "C" int falnet_image_to_u8(const float* x, float mean_r, float mean_g, float mean_b, void* out, int B, int H, int W, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0, "image_to_u8: bad argument");
    FALNET_CHECK_ARG((int64_t)B * H * W * 3 < ((int64_t)1 << 31), "image_to_u8: more than 2^31 output bytes");
    FALNET_CHECK_ARG(((uintptr_t)out & 3) == 0, "image_to_u8: output must be 4-byte aligned (and allocated to a multiple of 4 bytes)");
    const uint32_t hw = (uint32_t)H * W, bytes = hw * 3u * B, ndw = (bytes + 3) / 4;
    const uint32_t blocks = (ndw + 255) / 256 < 2048 ? (ndw + 255) / 256 : 2048;
    hipLaunchKernelGGL(image_to_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, mean_r, mean_g, mean_b, (uint32_t*)out, hw, bytes);
    FALNET_RETURN_LAUNCH();
}

// Test_KITTI.py:248-253: rint(clip(255 |x|, 0, 255)) -> u8, same layout as the input; four consecutive values per thread and dword
__global__ __launch_bounds__(256) void feature_to_u8_kernel(const float* __restrict__ x, uint32_t* __restrict__ out, uint32_t n, int vec4) {
    const uint32_t ndw = (n + 3) / 4;
    for (uint32_t d = blockIdx.x * 256u + threadIdx.x; d < ndw; d += gridDim.x * 256u) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec4 && 4 * d + 3 < n) {
            const float4 q = reinterpret_cast<const float4*>(x)[d];
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * d + k < n) v[k] = x[4 * d + k];
        }
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) word |= sat_rint_u8(fminf(fmaxf(__fmul_rn(255.f, fabsf(v[k])), 0.f), 255.f)) << (8 * k);
        out[d] = word;
    }
}

extern "C" int falnet_feature_to_u8(const float* x, void* out, int64_t n, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(x && out && n > 0 && n < ((int64_t)1 << 31), "feature_to_u8: bad argument (0 < n < 2^31)");
    FALNET_CHECK_ARG(((uintptr_t)out & 3) == 0, "feature_to_u8: output must be 4-byte aligned (and allocated to a multiple of 4 bytes)");
    const uint32_t ndw = (uint32_t)((n + 3) / 4);
    const uint32_t blocks = (ndw + 255) / 256 < 2048 ? (ndw + 255) / 256 : 2048;
    hipLaunchKernelGGL(feature_to_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, (uint32_t*)out, (uint32_t)n, (int)(((uintptr_t)x & 15) == 0));
    FALNET_RETURN_LAUNCH();
}

// ---- local normalisation (Test_KITTI.py:303-317) -----------------------------------------------------------------------------------------
// img = x + mean;  mu = avg_pool3x3(img);  sigma = sqrt(avg_pool3x3((img - mu)^2));  out = (img - mu) / (sigma + 1e-7)
// avg_pool2d pads with zeros and divides by 9 everywhere (count_include_pad).  The second pool pads the SQUARED DEVIATION with zeros: a
// neighbour outside the image adds nothing, and a neighbour inside it brings the mean of its OWN window -- hence two pixels of halo.
#define LN_TW 64
#define LN_TH 16
__global__ __launch_bounds__(256) void local_norm_kernel(const float* __restrict__ x, float m0, float m1, float m2, float* __restrict__ out,
                                                         float* __restrict__ mu_out, float* __restrict__ sigma_out, int H, int W) {
    __shared__ float img[LN_TH + 4][LN_TW + 4];
    __shared__ float dev2[LN_TH + 2][LN_TW + 2];  // (img - mu)^2, zero outside the image
    const int plane = blockIdx.z, c = plane % 3;
    const float m = c == 0 ? m0 : (c == 1 ? m1 : m2);
    const int x0 = blockIdx.x * LN_TW, y0 = blockIdx.y * LN_TH;
    const float* xp = x + (size_t)plane * H * W;
    for (int e = threadIdx.x; e < (LN_TH + 4) * (LN_TW + 4); e += 256) {
        const int r = e / (LN_TW + 4), q = e - r * (LN_TW + 4);
        const int yy = y0 + r - 2, xx = x0 + q - 2;
        img[r][q] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? __fadd_rn(xp[(size_t)yy * W + xx], m) : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < (LN_TH + 2) * (LN_TW + 2); e += 256) {
        const int r = e / (LN_TW + 2), q = e - r * (LN_TW + 2);
        const int yy = y0 + r - 1, xx = x0 + q - 1;
        float d2 = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            float s = 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) s += img[r + dy][q + dx];
            const float d = img[r + 1][q + 1] - __fdiv_rn(s, 9.f);
            d2 = d * d;
        }
        dev2[r][q] = d2;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < LN_TH * LN_TW; e += 256) {
        const int r = e / LN_TW, q = e - r * LN_TW;
        const int yy = y0 + r, xx = x0 + q;
        if (yy >= H || xx >= W) continue;
        float s = 0.f, s2 = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                s += img[r + 1 + dy][q + 1 + dx];
                s2 += dev2[r + dy][q + dx];
            }
        const float mu = __fdiv_rn(s, 9.f), sigma = __fsqrt_rn(__fdiv_rn(s2, 9.f));
        const size_t o = (size_t)plane * H * W + (size_t)yy * W + xx;
        out[o] = __fdiv_rn(img[r + 2][q + 2] - mu, __fadd_rn(sigma, 1e-7f));
        if (mu_out) mu_out[o] = mu;
        if (sigma_out) sigma_out[o] = sigma;
    }
}

extern "C" int falnet_local_norm(const float* x, float mean_r, float mean_g, float mean_b, float* out, float* mu_out, float* sigma_out, int win, int B, int H,
                                 int W, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0, "local_norm: bad argument");
    FALNET_CHECK_ARG(win == 3, "local_norm: only the reference's 3x3 window is built");
    FALNET_CHECK_ARG((int64_t)B * 3 <= 65535 && (H + LN_TH - 1) / LN_TH <= 65535, "local_norm: B * 3 planes or H / 16 row tiles exceed the grid");
    hipLaunchKernelGGL(local_norm_kernel, dim3((W + LN_TW - 1) / LN_TW, (H + LN_TH - 1) / LN_TH, B * 3), dim3(256), 0, (hipStream_t)stream, x, mean_r, mean_g,
                       mean_b, out, mu_out, sigma_out, H, W);
    FALNET_RETURN_LAUNCH();
}

// ---- point cloud (myUtils.py:339-373) ----------------------------------------------------------------------------------------------------
// PcParams, PcVertex, pc_vertex and trunc_u8: csrc/pc_vertex.h, shared with mesh.hip

// rows x, z, -y, r, g, b of (B, 6, H W): one vertex per thread, every store coalesced
__global__ __launch_bounds__(256) void point_cloud_planar_kernel(const float* __restrict__ img, const float* __restrict__ disp, PcParams p, float* __restrict__ out,
                                                                 uint32_t total) {
    const uint32_t hw = (uint32_t)p.H * p.W;
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < total; g += gridDim.x * 256u) {
        const PcVertex v = pc_vertex(img, disp, p, g);
        const uint32_t b = g / hw, pix = g - b * hw;
        float* o = out + (size_t)b * 6 * hw + pix;
        o[0] = v.x, o[hw] = v.z, o[2 * (size_t)hw] = v.ny, o[3 * (size_t)hw] = v.r, o[4 * (size_t)hw] = v.g, o[5 * (size_t)hw] = v.b;
    }
}

// `val` at byte offset `off` of the little-endian dword array w (off is a compile-time constant after unrolling: all of this folds to registers)
__device__ __forceinline__ void put_bits(uint32_t (&w)[15], int off, uint32_t val, int nbytes) {
    const int i = off >> 2, sh = (off & 3) * 8;
    w[i] |= val << sh;
    if (sh && (off & 3) + nbytes > 4) w[i + 1] |= val >> (32 - sh);
}

// binary-PLY vertex records (3 little-endian f32 + 3 u8 = 15 bytes): four vertices = 60 bytes = 15 whole dwords per thread
__global__ __launch_bounds__(256) void point_cloud_packed_kernel(const float* __restrict__ img, const float* __restrict__ disp, PcParams p,
                                                                 uint32_t* __restrict__ out, uint32_t total) {
    const uint32_t groups = (total + 3) / 4;
    const uint64_t ndw = ((uint64_t)total * 15 + 3) / 4;  // dwords that hold a byte of a real vertex
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < groups; q += gridDim.x * 256u) {
        uint32_t w[15];
#pragma unroll
        for (int k = 0; k < 15; ++k) w[k] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t g = 4 * q + k;
            if (g < total) {
                const PcVertex v = pc_vertex(img, disp, p, g);
                put_bits(w, 15 * k, __float_as_uint(v.x), 4);
                put_bits(w, 15 * k + 4, __float_as_uint(v.z), 4);
                put_bits(w, 15 * k + 8, __float_as_uint(v.ny), 4);
                put_bits(w, 15 * k + 12, trunc_u8(v.r) | (trunc_u8(v.g) << 8) | (trunc_u8(v.b) << 16), 3);
            }
        }
#pragma unroll
        for (int k = 0; k < 15; ++k)
            if ((uint64_t)q * 15 + k < ndw) out[(size_t)q * 15 + k] = w[k];
    }
}

extern "C" int falnet_point_cloud(const float* img, float mean_r, float mean_g, float mean_b, float rgb_scale, const float* disp, double focal, double baseline,
                                  float* out_planar, void* out_packed, int B, int H, int W, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(img && disp && B > 0 && H > 0 && W > 0 && (out_planar || out_packed), "point_cloud: bad argument (at least one output)");
    FALNET_CHECK_ARG((int64_t)B * H * W < ((int64_t)1 << 28), "point_cloud: more than 2^28 vertices");
    FALNET_CHECK_ARG(((uintptr_t)out_packed & 3) == 0, "point_cloud: packed output must be 4-byte aligned (and allocated to a multiple of 4 bytes)");
    FALNET_CHECK_ARG(focal > 0.0, "point_cloud: focal length must be positive");
    PcParams p;
    p.m0 = mean_r, p.m1 = mean_g, p.m2 = mean_b, p.rgb_scale = rgb_scale;
    p.focal = (float)focal, p.fb = (float)(focal * baseline);
    p.cx = (float)(W / 2.0), p.cy = (float)(H / 2.0);
    p.H = H, p.W = W;
    const uint32_t total = (uint32_t)B * H * W;
    if (out_planar) {
        const uint32_t blocks = (total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048;
        hipLaunchKernelGGL(point_cloud_planar_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, disp, p, out_planar, total);
    }
    if (out_packed) {
        const uint32_t groups = (total + 3) / 4;
        const uint32_t blocks = (groups + 255) / 256 < 2048 ? (groups + 255) / 256 : 2048;
        hipLaunchKernelGGL(point_cloud_packed_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, img, disp, p, (uint32_t*)out_packed, total);
    }
    FALNET_RETURN_LAUNCH();
}
