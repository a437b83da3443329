// Per-pixel statistics of the MED head's distribution over the N disparity planes (inference only; no backward, not replayable).
//
//   p_n = softmax_n dlog0_n        d_n = the head's plane table (med_plane_disp, med_planes.h)
//   a   = FIRST index of the largest stored logit (an exact comparison)        win = {n : |n - a| <= 1} within [0, N-1]
//   mean    mu = sum p_n d_n                      (falnet_med_head_fwd's disp)
//   std     sqrt(sum p_n (d_n - mu)^2)            from the CENTRED sum, a second pass over the pixel's planes in registers
//   entropy (ln S - sum p_n (l_n - m)) / ln N     m = l_a, S = sum exp(l_n - m); ln S = log1p(S - 1) with S - 1 summed WITHOUT plane a's exact 1:
//                                                 at a peaked pixel S = 1 + eps and logf(S) would lose eps to the rounding of S
//   arg     a                                     conf  sum_win p_n           peak  sum_win p_n d_n / sum_win p_n
//
// Form: nothing here shifts a plane, so a pixel needs only its own N logits.  One thread owns one pixel and holds its
// planes in registers (NP = 8, 64 or 128 of them, the bounds of the head's three forms; the loops are fully unrolled, every index is a
// constant); a workgroup owns 256 consecutive pixels of one sample's H W plane, so every plane is one coalesced 1 KiB read per workgroup and
// all N reads of a thread are independent and in flight together.  Each logit is fetched once; the passes after it (maximum and arg-max,
// sums, centred sum) run on registers.  No cross-lane step, no atomics: a launch repeats bit for bit.
#include "med_planes.h"

#define ST_THREADS 256
#define ST_NOUT 6

template <int NP>
__global__ __launch_bounds__(ST_THREADS) void med_stats_kernel(const float* __restrict__ dlog0, const float* __restrict__ min_disp,
                                                               const float* __restrict__ max_disp, unsigned which, int K,
                                                               float* __restrict__ out, int N, int64_t HW, int nblk) {
    __shared__ float td[NP];
    const int b = blockIdx.x / nblk, cb = blockIdx.x % nblk;
    {
        const float mn = min_disp[b], mx = max_disp[b];
        for (int n = threadIdx.x; n < N; n += ST_THREADS) td[n] = med_plane_disp(mn, mx, n, N);  // the head's d
    }
    __syncthreads();
    const int64_t pix = (int64_t)cb * ST_THREADS + threadIdx.x;
    if (pix >= HW) return;
    const float* L = dlog0 + (int64_t)b * N * HW + pix;
    float l[NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) l[n] = n < N ? L[(int64_t)n * HW] : -INFINITY;

    float m = l[0];
    int a = 0;
#pragma unroll
    for (int n = 1; n < NP; ++n) {
        if (n < N && l[n] > m) {  // strictly greater: the first index of the maximum stays
            m = l[n];
            a = n;
        }
    }
    float S = 0.f, Sx = 0.f, dacc = 0.f, T = 0.f, cw = 0.f, pw = 0.f;
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        if (n < N) {
            const float t = l[n] - m;
            const float e = __expf(t);
            l[n] = e;  // the logit is not needed again
            S += e;
            dacc += td[n] * e;
            T += e * t;
            const int dn = n - a;
            Sx += dn != 0 ? e : 0.f;  // S - 1: plane a's term is __expf(0) = 1 exactly
            if (dn >= -1 && dn <= 1) {
                cw += e;
                pw += td[n] * e;
            }
        }
    }
    const float mu = dacc / S;
    float var = 0.f;
    if (which & 2u) {
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            if (n < N) {
                const float c = td[n] - mu;
                var += l[n] * (c * c);
            }
        }
    }
    float* o = out + (int64_t)b * K * HW + pix;
    if (which & 1u) { *o = mu; o += HW; }
    if (which & 2u) { *o = sqrtf(var / S); o += HW; }
    if (which & 4u) { *o = (log1pf(Sx) - T / S) / logf((float)N); o += HW; }
    if (which & 8u) { *o = (float)a; o += HW; }
    if (which & 16u) { *o = cw / S; o += HW; }
    if (which & 32u) { *o = pw / cw; }
}

// ---------------------------------------------------------------------------------------- C-ABI
extern "C" int falnet_med_stats_fwd(const float* dlog0, const float* min_disp, const float* max_disp, unsigned which, float* out, int B, int N,
                                    int H, int W, void* stream) {
    FALNET_ENTER(stream);
    if (int r = med_check_shape("med_stats_fwd", "", B, N, H, W)) return r;
    FALNET_CHECK_ARG(which != 0 && which < (1u << ST_NOUT), "med_stats_fwd: which=0x%x selects no output or one above bit %d", which, ST_NOUT - 1);
    FALNET_CHECK_ARG(dlog0 && min_disp && max_disp && out, "med_stats_fwd: null pointer");
    const int64_t HW = (int64_t)H * W;
    const int64_t nblk = (HW + ST_THREADS - 1) / ST_THREADS;
    FALNET_CHECK_ARG((int64_t)B * nblk < (1ll << 31), "med_stats_fwd: B=%d H=%d W=%d: too many pixels for one launch", B, H, W);
    const int K = __builtin_popcount(which);
    const dim3 grid((unsigned)((int64_t)B * nblk));
#define STATS_LAUNCH(NP) \
    hipLaunchKernelGGL(med_stats_kernel<NP>, grid, dim3(ST_THREADS), 0, (hipStream_t)stream, dlog0, min_disp, max_disp, which, K, out, N, HW, (int)nblk)
    if (N <= 8) STATS_LAUNCH(8);
    else if (N <= 64) STATS_LAUNCH(64);
    else STATS_LAUNCH(MED_MAXN);
#undef STATS_LAUNCH
    FALNET_RETURN_LAUNCH();
}
