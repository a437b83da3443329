// Batched training-data augmentation: both views of all B samples of a batch from ONE launch (falnet_augment_batch).
//
// The per-sample path (data.hip behind data_transforms.StereoAugment) resizes the WHOLE frame in two launches, crops in a third, and needs
// host-made coefficient tables per axis and size.  Here a workgroup owns one AUG_TY x AUG_TX tile of the CROP of one (sample, view):
//   1. it computes Pillow's bicubic coefficients (src/libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc) for the AUG_TX
//      columns and AUG_TY rows of its tile only, in f64, operation by operation as data_transforms.resample_coeffs does on the host
//      (this file is compiled with -ffp-contract=off: with correctly rounded f64 + - * / and no fused multiply-add the 22-bit integers
//      equal the host's by construction);
//   2. horizontal pass: the source rows its vertical taps need, resampled at its columns, rounded (+2^21, >> 22, clip8) into a uint8
//      tile in LDS -- Pillow's two-pass order, and that intermediate rounding is what keeps the result bit-exact;
//   3. vertical pass from LDS, then augment_normalize_kernel's colour chain unchanged (data.hip), the mirrored store and (v / 255) - mean.
// Byte / integer work, HBM bound; source reads run along x, stores along x per channel plane.
#include <stdint.h>
#include "common.h"

#define AUG_THREADS 256
#define AUG_TX 64
#define AUG_TY 16
#define AUG_KMAX 9    // ksize = 2 * ceil(2 * max(in / out, 1)) + 1 at in / out <= FALNET_AUG_MAX_SCALE
// source rows under one tile: (AUG_TY - 1) * scale + 2 * support + 1 = 30 + 8 + 1 at scale 2, + 1 for the two truncations
#define AUG_ROWS 40
#define AUG_PRECISION_BITS 22

static_assert(FALNET_AUG_MAX_SCALE == 2, "AUG_KMAX / AUG_ROWS are sized for in / out <= 2");
static_assert(sizeof(falnet_aug_t) == 112, "falnet_aug_t layout (mirrored by fal_net_amd._lib.Aug)");

__device__ __forceinline__ double aug_bicubic(double x) {  // bicubic_filter of Resample.c, a = -0.5; x >= 0
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// data_transforms.resample_coeffs for output index xx of an in_size -> out_size axis: first source index, tap count, fixed-point weights
__device__ void aug_coeffs(int* first, int* n, int* kk, int xx, int in_size, int out_size) {
    if (in_size == out_size) {  // the host path skips the pass (resize_bicubic_u8); Pillow's own coefficients are the identity too
        *first = xx;
        *n = 1;
        kk[0] = 1 << AUG_PRECISION_BITS;
        return;
    }
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale > 1.0 ? scale : 1.0;
    const double support = 2.0 * filterscale;
    const double inv = 1.0 / filterscale;
    const double center = ((double)xx + 0.5) * scale;
    const double lo = center - support + 0.5;
    const int xmin = lo < 0 ? 0 : (int)lo;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > AUG_KMAX) xmax = AUG_KMAX;  // (cannot happen inside the refused range; keeps the LDS row in bounds)
    double ww = 0.0;  // the weight sum, tap by tap
    for (int x = 0; x < xmax; ++x) {
        double arg = ((double)x + (double)xmin - center + 0.5) * inv;
        ww = ww + aug_bicubic(arg < 0 ? -arg : arg);
    }
    for (int x = 0; x < xmax; ++x) {  // the weights again (no per-thread array), normalised, to 22-bit fixed point
        double arg = ((double)x + (double)xmin - center + 0.5) * inv;
        double w = aug_bicubic(arg < 0 ? -arg : arg);
        if (ww != 0.0) w = w / ww;
        const double fx = w * (double)(1 << AUG_PRECISION_BITS);
        kk[x] = w < 0 ? (int)(-0.5 + fx) : (int)(0.5 + fx);
    }
    *first = xmin;
    *n = xmax;
}

__device__ __forceinline__ int aug_clip8(int ss) {
    ss >>= AUG_PRECISION_BITS;  // arithmetic shift, as clip8() in Resample.c
    return ss < 0 ? 0 : (ss > 255 ? 255 : ss);
}

__global__ __launch_bounds__(AUG_THREADS) void augment_batch_kernel(const falnet_aug_t* __restrict__ table, int th, int tw, float mean0, float mean1,
                                                                    float mean2, float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ int hfirst[AUG_TX], hn[AUG_TX], hkk[AUG_TX][AUG_KMAX];  // coefficients of the tile's columns
    __shared__ int vfirst[AUG_TY], vn[AUG_TY], vkk[AUG_TY][AUG_KMAX];  // ... and rows
    __shared__ uint8_t hbuf[AUG_ROWS][AUG_TX * 3];                     // horizontally resampled source rows
    const int b = blockIdx.z >> 1, view = blockIdx.z & 1;
    const falnet_aug_t* __restrict__ r = table + b;
    const uint8_t* __restrict__ src = (const uint8_t*)(uintptr_t)r->src[view];
    float* __restrict__ dst = (view ? out1 : out0) + (int64_t)b * 3 * th * tw;
    const int W = r->W, flip = r->flip;
    const double gamma = r->gamma, bright = r->bright, cb0 = r->cb[view][0], cb1 = r->cb[view][1], cb2 = r->cb[view][2];
    const int cx0 = blockIdx.x * AUG_TX, cy0 = blockIdx.y * AUG_TY;  // tile origin in the crop, before the mirror
    const int ncx = min(AUG_TX, tw - cx0), ncy = min(AUG_TY, th - cy0);
    const int t = threadIdx.x;

    if (t < ncx) {
        aug_coeffs(&hfirst[t], &hn[t], hkk[t], r->x1 + cx0 + t, W, r->rw);
    } else if (t >= AUG_TX && t < AUG_TX + ncy) {
        const int s = t - AUG_TX;
        aug_coeffs(&vfirst[s], &vn[s], vkk[s], r->y1 + cy0 + s, r->H, r->rh);
    }
    __syncthreads();

    // horizontal pass: source rows [row0, row0 + nrows) at the tile's columns -> hbuf
    const int row0 = vfirst[0];
    int nrows = vfirst[ncy - 1] + vn[ncy - 1] - row0;
    if (nrows > AUG_ROWS) nrows = AUG_ROWS;  // (cannot happen inside the refused range)
    const int rowlen = ncx * 3;
    for (int i = t; i < nrows * rowlen; i += AUG_THREADS) {
        const int row = i / rowlen, e = i - row * rowlen, col = e / 3, c = e - col * 3;
        const uint8_t* p = src + ((int64_t)(row0 + row) * W + hfirst[col]) * 3 + c;
        const int n = hn[col];
        int ss = 1 << (AUG_PRECISION_BITS - 1);
        for (int k = 0; k < n; ++k) ss += (int)p[k * 3] * hkk[col][k];
        hbuf[row][e] = (uint8_t)aug_clip8(ss);
    }
    __syncthreads();

    // vertical pass, colour chain (augment_normalize_kernel of data.hip, unchanged), mirrored planar store
    const bool is_float = gamma > 0.0 || bright > 0.0;  // the reference's array left uint8 only if neither fired
    const bool has_cb = cb0 > 0.0;
    for (int i = t; i < 3 * AUG_TY * AUG_TX; i += AUG_THREADS) {
        const int cx = i % AUG_TX, cy = (i / AUG_TX) % AUG_TY, c = i / (AUG_TX * AUG_TY);
        if (cx >= ncx || cy >= ncy) continue;
        const int n = vn[cy];
        int rr = vfirst[cy] - row0;
        int ss = 1 << (AUG_PRECISION_BITS - 1);
        for (int k = 0; k < n; ++k) ss += (int)hbuf[min(rr + k, AUG_ROWS - 1)][cx * 3 + c] * vkk[cy][k];
        const uint8_t u = (uint8_t)aug_clip8(ss);
        double v = (double)u;
        const double cb = c == 0 ? cb0 : (c == 1 ? cb1 : cb2);
        if (gamma > 0.0) v = 255.0 * pow(v / 255.0, gamma);
        if (bright > 0.0) {
            v = v * bright;
            if (v > 255.0) v = 255.0;
        }
        if (has_cb) {
            if (is_float) {
                v = v * cb;
                if (v > 255.0) v = 255.0;
            } else {
                // assignment of a float64 product into the uint8 array (data_transforms.py:155): C conversion, low 8 bits
                v = (double)(uint8_t)(int)(v * cb);
            }
        }
        float f = (float)v;
        f = (f - 0.0f) / 255.0f;
        f = (f - (c == 0 ? mean0 : (c == 1 ? mean1 : mean2))) / 1.0f;
        const int ox = flip ? tw - 1 - (cx0 + cx) : cx0 + cx;  // np.fliplr of the crop
        dst[((int64_t)c * th + cy0 + cy) * tw + ox] = f;
    }
}

extern "C" int falnet_augment_batch(const falnet_aug_t* table_dev, const falnet_aug_t* table_host, int B, int th, int tw, float mean0, float mean1,
                                    float mean2, float* out0, float* out1, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(table_dev && table_host && out0 && out1, "augment_batch: null operand");
    FALNET_CHECK_ARG(B > 0 && B <= 32767 && th > 0 && tw > 0, "augment_batch: bad batch %d or crop %d x %d", B, th, tw);
    for (int i = 0; i < B; ++i) {
        const falnet_aug_t& r = table_host[i];
        FALNET_CHECK_ARG(r.src[0] && r.src[1], "augment_batch: sample %d: null source", i);
        FALNET_CHECK_ARG(r.H > 0 && r.W > 0 && r.rh > 0 && r.rw > 0 && r.H <= 32768 && r.W <= 32768, "augment_batch: sample %d: bad size %d x %d -> %d x %d", i,
                         r.H, r.W, r.rh, r.rw);
        FALNET_CHECK_ARG(r.H <= FALNET_AUG_MAX_SCALE * r.rh && r.rh <= FALNET_AUG_MAX_SCALE * r.H && r.W <= FALNET_AUG_MAX_SCALE * r.rw &&
                             r.rw <= FALNET_AUG_MAX_SCALE * r.W,
                         "augment_batch: sample %d: resize %d x %d -> %d x %d is outside the supported scale factors [1/%d, %d]", i, r.H, r.W, r.rh, r.rw,
                         FALNET_AUG_MAX_SCALE, FALNET_AUG_MAX_SCALE);
        FALNET_CHECK_ARG(r.x1 >= 0 && r.y1 >= 0 && (int64_t)r.x1 + tw <= r.rw && (int64_t)r.y1 + th <= r.rh,
                         "augment_batch: sample %d: crop %d x %d at (%d, %d) is outside the resized image %d x %d", i, th, tw, r.y1, r.x1, r.rh, r.rw);
        for (int v = 0; v < 2; ++v) {  // raw addresses: they must name device memory (a host tensor's address would fault the kernel)
            hipPointerAttribute_t at;
            const hipError_t e = hipPointerGetAttributes(&at, (const void*)(uintptr_t)r.src[v]);
            if (e != hipSuccess) (void)hipGetLastError();
            FALNET_CHECK_ARG(e == hipSuccess && at.type == hipMemoryTypeDevice, "augment_batch: sample %d: source %d is not device memory (no CPU fallback)", i, v);
        }
    }
    const dim3 grid((tw + AUG_TX - 1) / AUG_TX, (th + AUG_TY - 1) / AUG_TY, 2 * B);
    FALNET_CHECK_ARG(grid.y <= 65535, "augment_batch: crop height %d too large", th);
    hipLaunchKernelGGL(augment_batch_kernel, grid, dim3(AUG_THREADS), 0, (hipStream_t)stream, table_dev, th, tw, mean0, mean1, mean2, out0, out1);
    FALNET_RETURN_LAUNCH();
}
