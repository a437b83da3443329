// The Adam update (torch.optim.Adam, Train_Stage1_K.py:177-180), written ONCE for every kernel that applies it: the flat and range kernels of
// adam.hip and the pack-fused kernels of pack.hip.  One FlatAdam.step() sends a weight through the pack-fused kernel, a bias through the range
// kernel and, without a plan or under stream capture, the same parameters through the flat kernel: an element must get the same bits whichever
// path updates it (tests/test_gpu_pack.py: test_adam_paths_agree_bit_for_bit).  Device-only; all f32 arithmetic except the decayed gradient.
// Not part of common.h on purpose: that file is hashed into the autotune cache header (ops.py: _TUNE_SOURCES), this one is not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct AdamCoef { float b1, b2, eps, grad_scale, step_size, rsqrt_bc2; };

// Start of every kernel whose hyper-state lives on the device: state = {lr, t}, scaler = the loss scaler's {scale, good_steps, overflow_flag,
// skipped_steps} or NULL.  A captured hipGraph replays the same launch arguments, so the step count (bias corrections) advances in device
// memory (adam_tick_kernel), not in a kernel argument.  Returns false when the step is skipped: a non-finite gradient somewhere skips the
// whole update, decay included (uniform over the grid, so a kernel may return before a barrier).
__device__ __forceinline__ bool adam_unscale(float& grad_scale, const float* __restrict__ scaler) {
    if (scaler != nullptr) {
        if (scaler[2] != 0.f) return false;
        grad_scale /= scaler[0];
    }
    return true;
}
__device__ __forceinline__ void adam_coefficients(AdamCoef& c, const float* __restrict__ state, float b1, float b2, float eps, float grad_scale) {
    const float t = state[1] + 1.0f;
    c.b1 = b1, c.b2 = b2, c.eps = eps, c.grad_scale = grad_scale;
    c.step_size = state[0] / (1.0f - powf(b1, t));
    c.rsqrt_bc2 = rsqrtf(1.0f - powf(b2, t));
}
__device__ __forceinline__ bool adam_begin(AdamCoef& c, const float* __restrict__ state, float b1, float b2, float eps, float grad_scale,
                                           const float* __restrict__ scaler) {
    if (!adam_unscale(grad_scale, scaler)) return false;
    adam_coefficients(c, state, b1, b2, eps, grad_scale);
    return true;
}

// The gradient the moments are fed.  The two forms keep their own arithmetic: the undecayed one is NOT the decayed one at decay = 0 (f32
// product vs one rounding of a double fma), and it is the benchmarked step.
struct AdamGrad {
    __device__ __forceinline__ float operator()(const AdamCoef& c, float, float g) const { return g * c.grad_scale; }
};
// ---- weight decay / bias decay (torch.optim.Adam's L2 form, NOT AdamW; the two param groups of Train_Stage1_K.py:177-180) ----
// gr = g * grad_scale + decay * p, then the moments and the step exactly as without.  The decay differs per PARAMETER (bias_decay for the
// biases, weight_decay for the weights) and the flat buffer does not know which element is which, so the range and flat kernels read it from
// a small device table.  No extra memory stream: p is loaded anyway.  The 16-B padding elements between slices hold p = g = 0: gr = 0,
// m = v = 0 and the step is 0 / (0 + eps) = 0, so they stay exactly 0 whatever decay their segment carries.
// gr is formed in DOUBLE from a double decay and rounded to f32 once.  Where g and decay * p cancel (|gr| << |g|; with real gradients a few
// elements per million), an f32 sum -- or a decay rounded to f32 -- leaves gr with an absolute error of 2^-24 |g|, and while the second
// moment is still young the step lr * m / (sqrt(v) + eps) ~ lr * gr / |gr| amplifies it: torch's own f32 Adam lands an order of magnitude outside the
// tests' float64 bound there, this form stays inside it.  Three conversions and one f64 FMA per element beside 28 B of HBM traffic.
struct AdamGradL2 {
    double decay;
    __device__ __forceinline__ float operator()(const AdamCoef& c, float w, float g) const {
        return (float)fma(decay, (double)w, (double)g * (double)c.grad_scale);  // (the product of two floats is exact in double)
    }
};

template <typename Grad>
__device__ __forceinline__ void adam_update(const AdamCoef& c, const Grad& grad, float& p, float g, float& m, float& v) {
    const float gr = grad(c, p, g);
    m = c.b1 * m + (1.f - c.b1) * gr;
    v = c.b2 * v + (1.f - c.b2) * gr * gr;
    p -= c.step_size * m / (sqrtf(v) * c.rsqrt_bc2 + c.eps);
}
