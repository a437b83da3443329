// Views and disparities along the baseline from the MED head's logits (inference only; no backward, no statistics output).
//
// The logits of one forward describe the scene; the view at fraction t of the baseline shifts plane n by t * s_n, s_n = d_n (W-1)/W:
//   s = t s_n   k = floor(s)   a = s - k
//   L'_n(x) = (1-a) dlog0_n[x+k] + a dlog0_n[x+k+1]       taps outside [0, W-1] read 0 on BOTH sides (the out-of-row logit is 0, not -inf)
//   P_n(x)  = softmax_n L'_n(x)
//   view(c, x) = sum_n P_n(x) ((1-a) left_c[x+k] + a left_c[x+k+1])          disp(x) = sum_n d_n P_n(x)   (full-baseline pixels)
// t = 1 is falnet_med_head_fwd's p_im0 (the same arithmetic in the same order), t = 0 gives back the left image, t < 0 renders to the other
// side of the left camera.  Up to 8 views per launch read every logit row once from HBM.
//
// Split: a workgroup of 512 threads owns 512 consecutive columns of one image row -- ONE pixel per thread with the six
// accumulators (running max, sum, three colours, disparity) of all its views in registers -- and stages, CH plane rows at a time, only the
// window of the row its taps can reach: [x0 + min k - 2, x0 + 511 + max k + 1] over the launch's views and planes.  Rows wider than 512 are
// covered by several workgroups whose windows overlap; the overlap is re-read from L2.
#include <limits.h>
#include "med_planes.h"

#define SW_THREADS 512
#define SW_MAXV 8
#define SW_CH 8      // planes per online-softmax chunk, as the head
#define SW_FB_THREADS 256

struct SweepT {  // the baseline fractions, by value in the kernel arguments
    float t[SW_MAXV];
};

// plane n of view t: disparity d (pixels), shift t * d (W-1)/W split into k = floor and a.  d and the full shift are the head's own
// (med_planes.h), so that t = 1 gives its table bit for bit.  k is clamped as a FLOAT before the conversion: max_disp comes from device
// memory and is not bounded by the entry point; |k| <= W + 2 already puts both taps of every pixel outside the row.
__device__ __forceinline__ void sweep_plane(float mn, float mx, float t, int n, int N, int W, float& d, int& k, float& a) {
    d = med_plane_disp(mn, mx, n, N);
    const float st = t * med_plane_shift(d, W);
    const float kf = floorf(st);
    a = st - kf;
    k = (int)fminf(fmaxf(kf, -(float)(W + 2)), (float)(W + 2));
}

__device__ __forceinline__ float sweep_t(const SweepT& ts, int v) {  // ts.t[v] without an indexed copy of the argument
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < SW_MAXV; ++u) t = v == u ? ts.t[u] : t;
    return t;
}

// LDS: tk[VG][N] | ta[VG][N] | td[N] | win[4] | lrow[3][WP] | prow[CH][WP]
// Column c of a staged row is global column lo4 + c, lo4 a multiple of 4 (16-byte fills); global columns < 0 and >= W are staged as zeros.
// The first tap is clamped into [-2, W], so the second (first + 1) lies in [-1, W + 1]: two zero columns on each side, one paired LDS read.
template <int VG, int PF>
__global__ __launch_bounds__(SW_THREADS) __attribute__((amdgpu_waves_per_eu(PF <= 5 ? 4 : 2))) void med_sweep_lds_kernel(
    const float* __restrict__ dlog0, const float* __restrict__ left, const float* __restrict__ min_disp,
    const float* __restrict__ max_disp, const SweepT ts, int V, float* __restrict__ views, float* __restrict__ disps, int N, int H, int W,
    int nblk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* tk = reinterpret_cast<int*>(smem);
    float* ta = reinterpret_cast<float*>(smem) + VG * N;
    float* td = ta + VG * N;
    int* win = reinterpret_cast<int*>(td + N);
    const int WP = (W + 12) & ~3;  // row pitch in floats: >= W + 9
    float* lrow = reinterpret_cast<float*>(smem + ((size_t)(2 * VG * N + N + 4) * 4 + 15) / 16 * 16);  // [3][WP]
    float* prow = lrow + 3 * WP;                                                                    // [CH][WP]
    const int cb = blockIdx.x % nblk, row = blockIdx.x / nblk;
    const int b = row / H, y = row % H;
    const int x0 = cb * SW_THREADS;
    const int64_t HW = (int64_t)H * W;
    const bool want_views = views != nullptr, want_disps = disps != nullptr;

    if (threadIdx.x == 0) {
        win[0] = INT_MAX;
        win[1] = INT_MIN;
    }
    __syncthreads();
    {
        const float mn = min_disp[b], mx = max_disp[b];
        for (int i = threadIdx.x; i < VG * N; i += SW_THREADS) {
            const int v = i / N, n = i % N;
            float d, a;
            int k;
            sweep_plane(mn, mx, sweep_t(ts, v), n, N, W, d, k, a);
            tk[i] = k;
            ta[i] = a;
            if (v == 0) td[n] = d;
            if (v < V) {  // integer extrema in LDS: order-independent
                atomicMin(&win[0], k);
                atomicMax(&win[1], k);
            }
        }
    }
    __syncthreads();
    const int xlast = min(x0 + SW_THREADS - 1, W - 1);
    const int lo = min(max(x0 + win[0], -2), W);          // first tap of the leftmost pixel
    const int hi = min(max(xlast + win[1], -2), W) + 1;   // second tap of the rightmost pixel
    const int lo4 = ((lo + 4) & ~3) - 4;                  // multiple of 4, -4 <= lo4 <= lo
    const int cnt4 = (hi - lo4 + 4) >> 2;                 // float4 groups per staged row: 4 cnt4 <= W + 9 <= WP
    const int ncol = 4 * cnt4;

    const int64_t rowoff = (int64_t)y * W;
    for (int i = threadIdx.x; i < 3 * ncol; i += SW_THREADS) {
        const int c = i / ncol, col = i % ncol, g = lo4 + col;
        lrow[c * WP + col] = (want_views && g >= 0 && g < W) ? left[((int64_t)b * 3 + c) * HW + rowoff + g] : 0.f;
    }
    const float* Lrow = dlog0 + (int64_t)b * N * HW + rowoff;
    const bool vec4 = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(Lrow) & 15) == 0);

    const int x = x0 + threadIdx.x;
    const bool live = x < W;
    float m[VG], z[VG], p0[VG], p1[VG], p2[VG], dd[VG];
#pragma unroll
    for (int v = 0; v < VG; ++v) {
        m[v] = -INFINITY;
        z[v] = p0[v] = p1[v] = p2[v] = dd[v] = 0.f;
    }
    // register prefetch of the next chunk's window (vec4 path), as the head's forward: PF float4 per thread hold CH rows of <= (W + 9) / 4
    // float4 over 512 threads (the launch picks PF from W)
    float4 pf[PF];
    auto fetch = [&](int n0) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int i = threadIdx.x + u * SW_THREADS;
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < SW_CH * cnt4) {
                const int j = i / cnt4, g = lo4 + 4 * (i % cnt4);
                if (n0 + j < N && g >= 0 && g < W) val = *reinterpret_cast<const float4*>(Lrow + (int64_t)(n0 + j) * HW + g);  // W % 4 == 0: g + 3 < W
            }
            pf[u] = val;
        }
    };
    if (vec4) fetch(0);
    for (int n0 = 0; n0 < N; n0 += SW_CH) {
        __syncthreads();  // previous chunk fully consumed (and lrow ready)
        if (vec4) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int i = threadIdx.x + u * SW_THREADS;
                if (i < SW_CH * cnt4) *reinterpret_cast<float4*>(prow + (i / cnt4) * WP + 4 * (i % cnt4)) = pf[u];
            }
        } else {
            for (int i = threadIdx.x; i < SW_CH * ncol; i += SW_THREADS) {
                const int j = i / ncol, col = i % ncol, g = lo4 + col;
                prow[j * WP + col] = (n0 + j < N && g >= 0 && g < W) ? Lrow[(int64_t)(n0 + j) * HW + g] : 0.f;
            }
        }
        __syncthreads();
        if (vec4 && n0 + SW_CH < N) fetch(n0 + SW_CH);
        if (!live) continue;
#pragma unroll
        for (int v = 0; v < VG; ++v) {
            if (v >= V) break;
            float lw[SW_CH];
            int ix[SW_CH];
            float cm = -INFINITY;
#pragma unroll
            for (int j = 0; j < SW_CH; ++j) {
                const int n = n0 + j;
                if (n < N) {
                    ix[j] = min(max(x + tk[v * N + n], -2), W) - lo4;
                    const float a = ta[v * N + n];
                    const float* pr = prow + j * WP + ix[j];
                    lw[j] = (1.f - a) * pr[0] + a * pr[1];  // zero columns: the out-of-row logit is 0, not -inf
                } else {
                    ix[j] = 0;
                    lw[j] = -INFINITY;
                }
                cm = fmaxf(cm, lw[j]);
            }
            if (cm > m[v]) {
                const float s = __expf(m[v] - cm);
                z[v] *= s;
                p0[v] *= s;
                p1[v] *= s;
                p2[v] *= s;
                dd[v] *= s;
                m[v] = cm;
            }
#pragma unroll
            for (int j = 0; j < SW_CH; ++j) {
                const int n = n0 + j;
                if (n < N) {
                    const float e = __expf(lw[j] - m[v]);
                    z[v] += e;
                    if (want_disps) dd[v] += td[n] * e;
                    if (want_views) {
                        const float a = ta[v * N + n];
                        const float* lr = lrow + ix[j];
                        p0[v] += e * ((1.f - a) * lr[0] + a * lr[1]);
                        p1[v] += e * ((1.f - a) * lr[WP] + a * lr[WP + 1]);
                        p2[v] += e * ((1.f - a) * lr[2 * WP] + a * lr[2 * WP + 1]);
                    }
                }
            }
        }
    }
    if (!live) return;
    const int64_t pix = rowoff + x;
#pragma unroll
    for (int v = 0; v < VG; ++v) {
        if (v >= V) break;
        const float r = 1.f / z[v];
        if (want_views) {
            float* o = views + ((int64_t)b * V + v) * 3 * HW + pix;
            o[0] = p0[v] * r;
            o[HW] = p1[v] * r;
            o[2 * HW] = p2[v] * r;
        }
        if (want_disps) disps[((int64_t)b * V + v) * HW + pix] = dd[v] / z[v];
    }
}

// Rows wider than 2048: taps straight from global memory, as med_head_fwd_kernel.  One workgroup per (image row, view); LDS holds only the
// view's plane table.
__global__ __launch_bounds__(SW_FB_THREADS) void med_sweep_kernel(
    const float* __restrict__ dlog0, const float* __restrict__ left, const float* __restrict__ min_disp,
    const float* __restrict__ max_disp, const SweepT ts, int V, float* __restrict__ views, float* __restrict__ disps, int N, int H, int W) {
    __shared__ int tk[MED_MAXN];
    __shared__ float ta[MED_MAXN], td[MED_MAXN];
    const int b = blockIdx.x / H, y = blockIdx.x % H, v = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const float t = sweep_t(ts, v);
    for (int n = threadIdx.x; n < N; n += SW_FB_THREADS) sweep_plane(min_disp[b], max_disp[b], t, n, N, W, td[n], tk[n], ta[n]);
    __syncthreads();
    const bool want_views = views != nullptr, want_disps = disps != nullptr;
    const int64_t rowoff = (int64_t)y * W;
    const float* Lrow = dlog0 + (int64_t)b * N * HW + rowoff;
    const float* lr0 = left ? left + (int64_t)b * 3 * HW + rowoff : nullptr;
    auto tap = [&](const float* p, int i) -> float { return (i >= 0 && i < W) ? p[i] : 0.f; };  // zero padding on both sides
    for (int x = threadIdx.x; x < W; x += SW_FB_THREADS) {
        float m = -INFINITY, z = 0.f, p0 = 0.f, p1 = 0.f, p2 = 0.f, dd = 0.f;
        for (int n0 = 0; n0 < N; n0 += SW_CH) {
            float lw[SW_CH];
            float cm = -INFINITY;
#pragma unroll
            for (int j = 0; j < SW_CH; ++j) {
                const int n = n0 + j;
                if (n < N) {
                    const float* Ln = Lrow + (int64_t)n * HW;
                    const int i0 = x + tk[n];
                    const float a = ta[n];
                    lw[j] = (1.f - a) * tap(Ln, i0) + a * tap(Ln, i0 + 1);
                } else {
                    lw[j] = -INFINITY;
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
                m = cm;
            }
#pragma unroll
            for (int j = 0; j < SW_CH; ++j) {
                const int n = n0 + j;
                if (n < N) {
                    const float e = __expf(lw[j] - m);
                    z += e;
                    if (want_disps) dd += td[n] * e;
                    if (want_views) {
                        const int i0 = x + tk[n];
                        const float a = ta[n];
                        p0 += e * ((1.f - a) * tap(lr0, i0) + a * tap(lr0, i0 + 1));
                        p1 += e * ((1.f - a) * tap(lr0 + HW, i0) + a * tap(lr0 + HW, i0 + 1));
                        p2 += e * ((1.f - a) * tap(lr0 + 2 * HW, i0) + a * tap(lr0 + 2 * HW, i0 + 1));
                    }
                }
            }
        }
        const int64_t pix = rowoff + x;
        if (want_views) {
            const float r = 1.f / z;
            float* o = views + ((int64_t)b * V + v) * 3 * HW + pix;
            o[0] = p0 * r;
            o[HW] = p1 * r;
            o[2 * HW] = p2 * r;
        }
        if (want_disps) disps[((int64_t)b * V + v) * HW + pix] = dd / z;
    }
}

// ---------------------------------------------------------------------------------------- C-ABI
static size_t sweep_lds_bytes(int vg, int N, int W) {
    const size_t WP = (size_t)((W + 12) & ~3);
    return ((size_t)(2 * vg * N + N + 4) * 4 + 15) / 16 * 16 + (3 + SW_CH) * WP * sizeof(float);
}

template <int VG, int PF>
static int sweep_launch(const float* dlog0, const float* left, const float* min_disp, const float* max_disp, const SweepT& ts, int V, float* views,
                        float* disps, int B, int N, int H, int W, hipStream_t stream) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&med_sweep_lds_kernel<VG, PF>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const size_t lds = sweep_lds_bytes(VG, N, W);
    FALNET_CHECK_ARG(lds <= 64 * 1024 || attr == hipSuccess, "med_sweep_fwd: W=%d needs %zu bytes of LDS and the device refused more than 64 KiB", W, lds);
    const int nblk = (W + SW_THREADS - 1) / SW_THREADS;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(med_sweep_lds_kernel<VG, PF>), dim3((unsigned)((int64_t)B * H * nblk)), dim3(SW_THREADS), lds, stream, dlog0, left, min_disp, max_disp, ts,
                       V, views, disps, N, H, W, nblk);
    return 0;
}

extern "C" int falnet_med_sweep_fwd(const float* dlog0, const float* left, const float* min_disp, const float* max_disp, const float* t_host, int V,
                                    float* views, float* disps, int B, int N, int H, int W, void* stream) {
    FALNET_ENTER(stream);
    if (int r = med_check_shape("med_sweep_fwd", "", B, N, H, W)) return r;
    FALNET_CHECK_ARG((int64_t)B * H * ((W + SW_THREADS - 1) / SW_THREADS) < (1ll << 31), "med_sweep_fwd: B=%d H=%d W=%d: too many rows for one launch", B, H, W);
    FALNET_CHECK_ARG(V >= 1 && V <= SW_MAXV, "med_sweep_fwd: V=%d outside [1,%d]", V, SW_MAXV);
    FALNET_CHECK_ARG(views || disps, "med_sweep_fwd: no output requested");
    FALNET_CHECK_ARG(dlog0 && min_disp && max_disp && t_host, "med_sweep_fwd: null input");
    FALNET_CHECK_ARG(!views || left, "med_sweep_fwd: views requested without left image");
    SweepT ts;
    for (int v = 0; v < SW_MAXV; ++v) {
        ts.t[v] = v < V ? t_host[v] : 0.f;
        FALNET_CHECK_ARG(isfinite(ts.t[v]) && fabsf(ts.t[v]) <= 2.f, "med_sweep_fwd: baseline fraction t[%d]=%g is not a finite value in [-2,2]", v, (double)ts.t[v]);
    }
    if (W > 4 * SW_THREADS) {
        hipLaunchKernelGGL(med_sweep_kernel, dim3(B * H, V), dim3(SW_FB_THREADS), 0, (hipStream_t)stream, dlog0, left, min_disp, max_disp, ts, V, views, disps,
                           N, H, W);
        FALNET_RETURN_LAUNCH();
    }
    // prefetch depth: CH rows of at most (W + 9) / 4 float4 over 512 threads -> 8 (W + 9) / 4 <= 512 PF
    const int pf = W <= 759 ? 3 : (W <= 1271 ? 5 : 9);
    const int vg = V == 1 ? 1 : (V == 2 ? 2 : (V <= 4 ? 4 : 8));
    int r = -1;
#define SWEEP_CASE(G, P) \
    if (vg == G && pf == P) r = sweep_launch<G, P>(dlog0, left, min_disp, max_disp, ts, V, views, disps, B, N, H, W, (hipStream_t)stream)
#define SWEEP_VG(G) SWEEP_CASE(G, 3); SWEEP_CASE(G, 5); SWEEP_CASE(G, 9)
    SWEEP_VG(1);
    SWEEP_VG(2);
    SWEEP_VG(4);
    SWEEP_VG(8);
#undef SWEEP_VG
#undef SWEEP_CASE
    if (r) return r;
    FALNET_RETURN_LAUNCH();
}
