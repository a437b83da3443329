// Free-viewpoint rendering of the MED head's logits: a homography plane sweep (inference only; no backward, not replayable).
//
// The logits of one forward are a multiplane image: plane n is the fronto-parallel plane Z = fx b / s_n of the left camera, s_n = d_n (W-1)/W
// (the head's table, med_planes.h).  A target camera travels as 12 doubles (include/falnet_hip.h):
//   A = K R^T K_t^-1   (3 x 3, row-major: target pixel -> ray direction in source pixel coordinates)      E = K c / (fx b)
// For target pixel (x, y):  q = A (x, y, 1),  u0 = q_x / q_z,  v0 = q_y / q_z;  for plane n
//   w_n = 1 - s_n E_z      u_n = s_n E_x + w_n u0      v_n = s_n E_y + w_n v0          sampled iff q_z > 0 and w_n > 0
//   L'_n   = bilinear(dlog0_n, u_n, v_n)        four taps, zero outside the image; a plane that is not sampled has L'_n = 0 (0, not -inf)
//   P_n    = softmax_n L'_n
//   view_c = sum_n P_n bilinear(left_c, u_n, v_n)     disp = sum_n d_n P_n     cover = sum_n P_n omega_n
// omega_n = the sum of the bilinear weights of the taps inside the image (0 for a plane not sampled).  A = I, E = (t, 0, 0) is
// falnet_med_sweep_fwd's view t: u_n = x + t s_n, v_n = y.
//
// Split: gather form.  The source positions of a pixel over the planes lie on one epipolar line through the image, so
// there is no row window to stage; a workgroup of 256 threads owns a tile of 8 rows x 32 columns of ONE (sample, view), one pixel per thread,
// and reads its taps straight from global memory (a wave's taps of one plane are two row segments of about 33 floats for small rotations).
// One pass over the planes, PO_CH at a time, with an online softmax; seven accumulators per pixel (running max, sum, three colours,
// disparity, cover).  q, u0, v0 and the per-plane coordinate are formed in f64 from the f64 record; the coordinate is clamped AS A FLOATING
// VALUE into [-2, W + 1] x [-2, H + 1] before it is split into floor and fraction (max_disp comes from device memory unbounded and a pose can
// send a tap anywhere; a NaN coordinate clamps to -2), a tap is read only where its index lies inside the image and its weight is not zero,
// weights and blends are f32.
// No atomics: two launches give the same bits.
#include <limits.h>
#include "med_planes.h"

#define PO_TX 32
#define PO_TY 8
#define PO_THREADS (PO_TX * PO_TY)
#define PO_MAXV 8
#define PO_CH 4      // planes per online-softmax chunk

struct PoseT {  // the pose records, by value in the kernel arguments: A (row-major) then E
    double r[PO_MAXV][12];
};

// the four taps of one plane of one pixel: in-plane offset of the first, fractions, and which of them lie inside the image
struct PoseTaps {
    int off;
    float ax, ay;
    bool m00, m01, m10, m11;
};

__device__ __forceinline__ float pose_blend(const PoseTaps& t, float t00, float t01, float t10, float t11) {
    return (1.f - t.ay) * ((1.f - t.ax) * t00 + t.ax * t01) + t.ay * ((1.f - t.ax) * t10 + t.ax * t11);
}

// one float at `bytes` behind a wave-uniform base
__device__ __forceinline__ float pose_ld(const float* base, unsigned bytes) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + bytes);
}

template <bool VIEWS>
__global__ __launch_bounds__(PO_THREADS) void med_pose_kernel(
    const float* __restrict__ dlog0, const float* __restrict__ left, const float* __restrict__ min_disp,
    const float* __restrict__ max_disp, const PoseT poses, int V, float* __restrict__ views, float* __restrict__ disps,
    float* __restrict__ cover, int N, int H, int W, int tiles_x, int tiles) {
    __shared__ double tsx[MED_MAXN], tsy[MED_MAXN], tw[MED_MAXN];  // s_n E_x, s_n E_y, 1 - s_n E_z of this workgroup's view
    __shared__ float td[MED_MAXN];
    const int tile = blockIdx.x % tiles, bv = blockIdx.x / tiles;
    const int v = bv % V, b = bv / V;
    const double* rec = poses.r[v];
    {
        const float mn = min_disp[b], mx = max_disp[b];
        const double ex = rec[9], ey = rec[10], ez = rec[11];
        for (int n = threadIdx.x; n < N; n += PO_THREADS) {
            // the head's d and s (med_planes.h): at pure-baseline poses the shifts are the sweep's
            const float d = med_plane_disp(mn, mx, n, N);
            const float s = med_plane_shift(d, W);
            td[n] = d;
            tsx[n] = (double)s * ex;
            tsy[n] = (double)s * ey;
            tw[n] = 1.0 - (double)s * ez;
        }
    }
    __syncthreads();
    const int x = (tile % tiles_x) * PO_TX + (threadIdx.x % PO_TX);
    const int y = (tile / tiles_x) * PO_TY + (threadIdx.x / PO_TX);
    if (x >= W || y >= H) return;  // no barrier below
    const int64_t HW = (int64_t)H * W;  // < 2^30 (entry point): in-plane byte offsets fit 32 bits
    const bool want_disps = disps != nullptr, want_cover = cover != nullptr;

    const double qx = rec[0] * x + rec[1] * y + rec[2];
    const double qy = rec[3] * x + rec[4] * y + rec[5];
    const double qz = rec[6] * x + rec[7] * y + rec[8];
    const bool front = qz > 0.0;
    const double u0 = front ? qx / qz : 0.0, v0 = front ? qy / qz : 0.0;
    const double umax = (double)(W + 1), vmax = (double)(H + 1);

    const float* Lb = dlog0 + (int64_t)b * N * HW;
    const float* I0 = VIEWS ? left + (int64_t)b * 3 * HW : nullptr;
    const float *I1 = VIEWS ? I0 + HW : nullptr, *I2 = VIEWS ? I0 + 2 * HW : nullptr;

    float m = -INFINITY, z = 0.f, p0 = 0.f, p1 = 0.f, p2 = 0.f, dd = 0.f, cv = 0.f;
    for (int n0 = 0; n0 < N; n0 += PO_CH) {
        float lw[PO_CH], c0[PO_CH], c1[PO_CH], c2[PO_CH], om[PO_CH];
        float cm = -INFINITY;
#pragma unroll
        for (int j = 0; j < PO_CH; ++j) {
            const int n = n0 + j;
            lw[j] = -INFINITY;
            c0[j] = c1[j] = c2[j] = om[j] = 0.f;
            if (n < N) {
                const double w = tw[n];
                const bool samp = front && w > 0.0;
                // clamped as f64 values before they become integers; fmax(NaN, -2) = -2
                const double u = fmin(fmax(fma(w, u0, tsx[n]), -2.0), umax);
                const double vv = fmin(fmax(fma(w, v0, tsy[n]), -2.0), vmax);
                const double fu = floor(u), fv = floor(vv);
                const int ix = (int)fu, iy = (int)fv;  // in [-2, W + 1], [-2, H + 1]
                PoseTaps t;
                t.ax = (float)(u - fu);
                t.ay = (float)(vv - fv);
                t.off = iy * W + ix;
                // a tap is read where it lies inside the image and carries weight (a zero fraction leaves the second tap of its axis unread)
                const bool x0 = samp && ix >= 0 && ix < W, x1 = samp && ix >= -1 && ix < W - 1 && t.ax > 0.f;
                const bool y0 = iy >= 0 && iy < H, y1 = iy >= -1 && iy < H - 1 && t.ay > 0.f;
                t.m00 = x0 && y0;
                t.m01 = x1 && y0;
                t.m10 = x0 && y1;
                t.m11 = x1 && y1;
                om[j] = ((x0 ? 1.f - t.ax : 0.f) + (x1 ? t.ax : 0.f)) * ((y0 ? 1.f - t.ay : 0.f) + (y1 ? t.ay : 0.f));
                const float* Ln = Lb + (int64_t)n * HW;
                float l00 = 0.f, l01 = 0.f, l10 = 0.f, l11 = 0.f;
                float r00 = 0.f, r01 = 0.f, r10 = 0.f, r11 = 0.f, g00 = 0.f, g01 = 0.f, g10 = 0.f, g11 = 0.f, b00 = 0.f, b01 = 0.f, b10 = 0.f, b11 = 0.f;
                // byte offsets of the taps, unsigned and below 2^32 (entry point): with the plane's base in scalar registers a tap is one load
                // whose address needs no vector arithmetic.  Formed only where the tap lies inside the image.
                if (t.m00) {
                    const unsigned o = 4u * (unsigned)t.off;
                    l00 = pose_ld(Ln, o);
                    if (VIEWS) r00 = pose_ld(I0, o), g00 = pose_ld(I1, o), b00 = pose_ld(I2, o);
                }
                if (t.m01) {
                    const unsigned o = 4u * (unsigned)(t.off + 1);
                    l01 = pose_ld(Ln, o);
                    if (VIEWS) r01 = pose_ld(I0, o), g01 = pose_ld(I1, o), b01 = pose_ld(I2, o);
                }
                if (t.m10) {
                    const unsigned o = 4u * (unsigned)(t.off + W);
                    l10 = pose_ld(Ln, o);
                    if (VIEWS) r10 = pose_ld(I0, o), g10 = pose_ld(I1, o), b10 = pose_ld(I2, o);
                }
                if (t.m11) {
                    const unsigned o = 4u * (unsigned)(t.off + W + 1);
                    l11 = pose_ld(Ln, o);
                    if (VIEWS) r11 = pose_ld(I0, o), g11 = pose_ld(I1, o), b11 = pose_ld(I2, o);
                }
                lw[j] = pose_blend(t, l00, l01, l10, l11);  // every tap outside, or the plane not sampled: 0, not -inf
                if (VIEWS) {
                    c0[j] = pose_blend(t, r00, r01, r10, r11);
                    c1[j] = pose_blend(t, g00, g01, g10, g11);
                    c2[j] = pose_blend(t, b00, b01, b10, b11);
                }
            }
            cm = fmaxf(cm, lw[j]);
        }
        if (cm > m) {
            const float s = __expf(m - cm);
            z *= s;
            p0 *= s;
            p1 *= s;
            p2 *= s;
            dd *= s;
            cv *= s;
            m = cm;
        }
#pragma unroll
        for (int j = 0; j < PO_CH; ++j) {
            const int n = n0 + j;
            if (n < N) {
                const float e = __expf(lw[j] - m);
                z += e;
                if (want_disps) dd += td[n] * e;
                if (want_cover) cv += om[j] * e;
                if (VIEWS) {
                    p0 += e * c0[j];
                    p1 += e * c1[j];
                    p2 += e * c2[j];
                }
            }
        }
    }
    const int64_t pix = (int64_t)y * W + x;
    const int64_t img = (int64_t)b * V + v;
    if (VIEWS) {
        const float r = 1.f / z;
        float* o = views + img * 3 * HW + pix;
        o[0] = p0 * r;
        o[HW] = p1 * r;
        o[2 * HW] = p2 * r;
    }
    if (want_disps) disps[img * HW + pix] = dd / z;
    if (want_cover) cover[img * HW + pix] = cv / z;
}

// ---------------------------------------------------------------------------------------- C-ABI
extern "C" int falnet_med_pose_fwd(const float* dlog0, const float* left, const float* min_disp, const float* max_disp, const double* pose_host, int V,
                                   float* views, float* disps, float* cover, int B, int N, int H, int W, void* stream) {
    FALNET_ENTER(stream);
    if (int r = med_check_shape("med_pose_fwd", "", B, N, H, W)) return r;
    FALNET_CHECK_ARG((int64_t)(H + 2) * W + 2 <= (1ll << 30), "med_pose_fwd: H=%d W=%d: a plane of more than 2^30 pixels", H, W);
    FALNET_CHECK_ARG(V >= 1 && V <= PO_MAXV, "med_pose_fwd: V=%d outside [1,%d]", V, PO_MAXV);
    FALNET_CHECK_ARG(views || disps || cover, "med_pose_fwd: no output requested");
    FALNET_CHECK_ARG(dlog0 && min_disp && max_disp && pose_host, "med_pose_fwd: null input");
    FALNET_CHECK_ARG(!views || left, "med_pose_fwd: views requested without left image");
    const int tiles_x = (W + PO_TX - 1) / PO_TX, tiles_y = (H + PO_TY - 1) / PO_TY;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * B * V;
    FALNET_CHECK_ARG(blocks < (1ll << 31), "med_pose_fwd: B=%d V=%d H=%d W=%d: too many tiles for one launch", B, V, H, W);
    PoseT poses;
    for (int v = 0; v < PO_MAXV; ++v) {
        for (int i = 0; i < 12; ++i) {
            poses.r[v][i] = v < V ? pose_host[v * 12 + i] : 0.0;
            FALNET_CHECK_ARG(isfinite(poses.r[v][i]), "med_pose_fwd: pose %d entry %d is not finite", v, i);
        }
        FALNET_CHECK_ARG(v >= V || poses.r[v][6] != 0.0 || poses.r[v][7] != 0.0 || poses.r[v][8] != 0.0,
                         "med_pose_fwd: pose %d: the third row of A is all zero (no pixel has a depth)", v);
    }
    const dim3 grid((unsigned)blocks), block(PO_THREADS);
    if (views)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(med_pose_kernel<true>), grid, block, 0, (hipStream_t)stream, dlog0, left, min_disp, max_disp, poses, V, views, disps, cover,
                           N, H, W, tiles_x, tiles_x * tiles_y);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(med_pose_kernel<false>), grid, block, 0, (hipStream_t)stream, dlog0, left, min_disp, max_disp, poses, V, views, disps, cover,
                           N, H, W, tiles_x, tiles_x * tiles_y);
    FALNET_RETURN_LAUNCH();
}
