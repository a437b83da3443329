// Fused flat Adam for gfx950 (torch.optim.Adam, Train_Stage1_K.py:177-180): the stand-alone optimiser kernels.  The arithmetic is adam.h,
// shared with the pack-fused kernels of pack.hip; here are the two ways of walking the flat buffer (float4 lanes over a whole row, a list
// of element ranges) and the step-count tick.  7 f32 streams per element (read p,g,m,v; write p,m,v): 28 B/param, pure HBM streaming.
// Not one of the autotuned sources (ops.py: _TUNE_SOURCES).
#include <math.h>
#include "adam.h"
#include "common.h"

#define ADAM_THREADS 256

// The arithmetic of every kernel below is adam.h; the loops and their loads and stores stay in the __global__ functions.  A loop moved
// into a shared helper is optimised on its own before it is inlined, and the kernels then come out as other instruction streams -- the
// float4 kernels with the OTHER multiply of the first moment fused into its add, i.e. other bits (tools/isa_identity.py shows it).
// Hence a macro for the one piece three kernels share: float4 `i` of a flat row, p, g, m, v being the kernel's arguments.
#define ADAM_FLAT4(c, grad, i)                                                                         \
    do {                                                                                               \
        float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];       \
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];             \
        float *P = &pp.x, *G = &gg.x, *M = &mm.x, *V = &vv.x;                                          \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) adam_update(c, grad, P[j], G[j], M[j], V[j]);    \
        reinterpret_cast<float4*>(p)[i] = pp;                                                          \
        reinterpret_cast<float4*>(m)[i] = mm;                                                          \
        reinterpret_cast<float4*>(v)[i] = vv;                                                          \
    } while (0)

// Coefficients formed on the host (falnet_adam_step); any n: the n & 3 elements behind the last float4 are a scalar tail.
__global__ __launch_bounds__(ADAM_THREADS) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                            float step_size, float b1, float b2, float eps,
                                                            float rsqrt_bc2, float grad_scale) {
    const AdamCoef c{b1, b2, eps, grad_scale, step_size, rsqrt_bc2};
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) ADAM_FLAT4(c, AdamGrad(), i);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (n4 << 2) + threadIdx.x;
        float gi = g[i], mi = m[i], vi = v[i], pi = p[i];
        adam_update(c, AdamGrad(), pi, gi, mi, vi);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
}

// Adam with its hyper-state on the device (adam.h: adam_begin).
__global__ __launch_bounds__(ADAM_THREADS) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                                const float* __restrict__ state, float b1, float b2, float eps,
                                                                float grad_scale, const float* __restrict__ scaler) {
    AdamCoef c;
    if (!adam_begin(c, state, b1, b2, eps, grad_scale, scaler)) return;
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) ADAM_FLAT4(c, AdamGrad(), i);
}
// The same update over a list of element ranges of the flat buffer (the parameters falnet_adam_pack_batched does not own: biases, the two
// factors of the composed logits weights): ranges[2 r] = first element, ranges[2 r + 1] = count; blockIdx.y = range.
__global__ __launch_bounds__(ADAM_THREADS) void adam_ranges_kernel(float* __restrict__ p, int64_t g_off, int64_t m_off, int64_t v_off,
                                                                   const int64_t* __restrict__ ranges, const float* __restrict__ state, float b1, float b2,
                                                                   float eps, float grad_scale, const float* __restrict__ scaler) {
    AdamCoef c;
    if (!adam_begin(c, state, b1, b2, eps, grad_scale, scaler)) return;
    const int64_t beg = ranges[2 * blockIdx.y], cnt = ranges[2 * blockIdx.y + 1];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        float* wp = p + beg + i;
        float w = *wp, gi = wp[g_off], mi = wp[m_off], vi = wp[v_off];
        adam_update(c, AdamGrad(), w, gi, mi, vi);
        *wp = w;
        wp[m_off] = mi;
        wp[v_off] = vi;
    }
}
__global__ void adam_tick_kernel(float* state, const float* __restrict__ scaler) {
    if (scaler == nullptr || scaler[2] == 0.f) state[1] += 1.0f;  // a skipped (overflowed) step does not count
}

// ---- weight decay / bias decay (adam.h: AdamGradL2) ----
// Range form: decays[r] belongs to ranges[2 r], ranges[2 r + 1] (a range never spans two parameters: plan.py cuts them at the boundaries).
__global__ __launch_bounds__(ADAM_THREADS) void adam_ranges_wd_kernel(float* __restrict__ p, int64_t g_off, int64_t m_off, int64_t v_off,
                                                                      const int64_t* __restrict__ ranges, const double* __restrict__ decays,
                                                                      const float* __restrict__ state, float b1, float b2, float eps, float grad_scale,
                                                                      const float* __restrict__ scaler) {
    AdamCoef c;
    if (!adam_begin(c, state, b1, b2, eps, grad_scale, scaler)) return;
    const int64_t beg = ranges[2 * blockIdx.y], cnt = ranges[2 * blockIdx.y + 1];
    const AdamGradL2 grad{decays[blockIdx.y]};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        float* wp = p + beg + i;
        float w = *wp, gi = wp[g_off], mi = wp[m_off], vi = wp[v_off];
        adam_update(c, grad, w, gi, mi, vi);
        *wp = w;
        wp[m_off] = mi;
        wp[v_off] = vi;
    }
}
// Flat form (the stand-alone update: no plan yet, pack fusion off, stream capture): the float4 streaming loop of adam_dev_kernel; the
// decay of a float4 comes from a segment table -- seg_end[s] = exclusive end ELEMENT of segment s (ascending, multiples of 4 because the
// slices are 16-B aligned, seg_end[n_seg - 1] >= n), seg_decay[s] its decay -- staged in LDS once per block and searched per float4
// (<= 10 LDS reads beside 7 x 16 B of HBM traffic).  An index past the last end falls into the last segment: the lookup cannot leave the table.
#define ADAM_WD_MAX_SEG 1024
__global__ __launch_bounds__(ADAM_THREADS) void adam_dev_wd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                   float* __restrict__ v, int64_t n, const int64_t* __restrict__ seg_end,
                                                                   const double* __restrict__ seg_decay, int n_seg, const float* __restrict__ state,
                                                                   float b1, float b2, float eps, float grad_scale, const float* __restrict__ scaler) {
    __shared__ int64_t s_end4[ADAM_WD_MAX_SEG];  // in float4 units
    __shared__ double s_decay[ADAM_WD_MAX_SEG];
    if (!adam_unscale(grad_scale, scaler)) return;  // grid-uniform, before the barrier
    for (int s = threadIdx.x; s < n_seg; s += blockDim.x) {
        s_end4[s] = seg_end[s] >> 2;
        s_decay[s] = seg_decay[s];
    }
    __syncthreads();
    AdamCoef c;
    adam_coefficients(c, state, b1, b2, eps, grad_scale);
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        int lo = 0, hi = n_seg - 1;  // first segment whose end lies beyond float4 i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (i < s_end4[mid]) hi = mid;
            else lo = mid + 1;
        }
        const AdamGradL2 grad{s_decay[lo]};
        ADAM_FLAT4(c, grad, i);
    }
}

extern "C" int falnet_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                                float eps, int step, float grad_scale, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adam_step: bad argument");
    FALNET_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step: buffers must be 16-B aligned");
    const double bc1 = 1.0 - pow((double)b1, step), bc2 = 1.0 - pow((double)b2, step);
    const float step_size = (float)(lr / bc1), rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
    hipLaunchKernelGGL(adam_kernel, dim3(2048), dim3(ADAM_THREADS), 0, (hipStream_t)stream, p, g, m, v, n, step_size, b1,
                       b2, eps, rsqrt_bc2, grad_scale);
    FALNET_RETURN_LAUNCH();
}

static int adam_dev_launch(float* p, const float* g, float* m, float* v, int64_t n, float* state, float b1, float b2, float eps, float grad_scale,
                           const float* scaler, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(p && g && m && v && state && n > 0 && (n & 3) == 0, "adam_step_dev: bad argument (n must be a multiple of 4)");
    FALNET_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step_dev: buffers must be 16-B aligned");
    hipLaunchKernelGGL(adam_dev_kernel, dim3(2048), dim3(ADAM_THREADS), 0, (hipStream_t)stream, p, g, m, v, n, state, b1, b2, eps, grad_scale, scaler);
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, scaler);
    FALNET_RETURN_LAUNCH();
}
extern "C" int falnet_adam_ranges(float* p, int64_t g_off, int64_t m_off, int64_t v_off, const int64_t* ranges_dev, int n_ranges, const float* state,
                                  float b1, float b2, float eps, float grad_scale, const float* scaler, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(p && ranges_dev && n_ranges > 0 && state && g_off != 0 && m_off != 0 && v_off != 0, "adam_ranges: bad argument");
    hipLaunchKernelGGL(adam_ranges_kernel, dim3(48, n_ranges), dim3(ADAM_THREADS), 0, (hipStream_t)stream, p, g_off, m_off, v_off, ranges_dev, state, b1, b2, eps,
                       grad_scale, scaler);
    FALNET_RETURN_LAUNCH();
}
extern "C" int falnet_adam_tick(float* state, const float* scaler, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(state, "adam_tick: bad argument");
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, scaler);
    FALNET_RETURN_LAUNCH();
}
extern "C" int falnet_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, float b1, float b2,
                                    float eps, float grad_scale, void* stream) {
    return adam_dev_launch(p, g, m, v, n, state, b1, b2, eps, grad_scale, nullptr, stream);
}
extern "C" int falnet_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, float* state, float b1, float b2,
                                        float eps, float grad_scale, const float* scaler, void* stream) {
    FALNET_CHECK_ARG(scaler, "adam_step_guarded: scaler is NULL");
    return adam_dev_launch(p, g, m, v, n, state, b1, b2, eps, grad_scale, scaler, stream);
}
extern "C" int falnet_adam_ranges_wd(float* p, int64_t g_off, int64_t m_off, int64_t v_off, const int64_t* ranges_dev, const double* decays_dev,
                                     int n_ranges, const float* state, float b1, float b2, float eps, float grad_scale, const float* scaler,
                                     void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(p && ranges_dev && decays_dev && n_ranges > 0 && n_ranges <= 65535 && state && g_off != 0 && m_off != 0 && v_off != 0,
                     "adam_ranges_wd: bad argument");
    hipLaunchKernelGGL(adam_ranges_wd_kernel, dim3(48, n_ranges), dim3(ADAM_THREADS), 0, (hipStream_t)stream, p, g_off, m_off, v_off, ranges_dev, decays_dev,
                       state, b1, b2, eps, grad_scale, scaler);
    FALNET_RETURN_LAUNCH();
}
extern "C" int falnet_adam_step_wd(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end_dev, const double* seg_decay_dev,
                                   int n_seg, float* state, float b1, float b2, float eps, float grad_scale, const float* scaler, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(p && g && m && v && state && n > 0 && (n & 3) == 0, "adam_step_wd: bad argument (n must be a multiple of 4)");
    FALNET_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step_wd: buffers must be 16-B aligned");
    FALNET_CHECK_ARG(seg_end_dev && seg_decay_dev && n_seg > 0 && n_seg <= ADAM_WD_MAX_SEG, "adam_step_wd: 1 .. %d segments", ADAM_WD_MAX_SEG);
    hipLaunchKernelGGL(adam_dev_wd_kernel, dim3(2048), dim3(ADAM_THREADS), 0, (hipStream_t)stream, p, g, m, v, n, seg_end_dev, seg_decay_dev, n_seg, state,
                       b1, b2, eps, grad_scale, scaler);
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, scaler);
    FALNET_RETURN_LAUNCH();
}
