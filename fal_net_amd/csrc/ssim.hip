// Structural similarity (Wang et al. 2004) of the synthesised view against the real one, in two forms that share one windowed-moment routine:
//   * the METRIC: the 11 x 11 Gaussian window (sigma 1.5) on the 0..255 images that get_psnr forms, in f64 -> one column of a MetricTable row;
//   * the LOSS:   the 3 x 3 box of Monodepth on the 0..1 images, in f32, mean((1 - S) / 2), with its adjoint with respect to the synthesised view.
// Both take VALID windows only (no padding): (H - 2R) x (W - 2R) window centres per plane.
//
// One workgroup owns one tile of one of the B * C planes.  It stages the tile plus its halo in LDS as f32, `windowed_moments` forms the five
// windowed sums (x, y, x^2, y^2, x y) separably -- a row pass into LDS, then a column pass that hands the finished moments of every window
// centre to the caller -- and the kernel turns them into S.  The loss's backward is the SAME kernel with a wider centre region: S and the three
// adjoint maps A, Bm, Cm are formed on tile + R, and every pixel of the tile gathers the windows that contain it.
//
// Reductions follow metrics.hip: one partial sum per workgroup (a double, wave shuffles then the four waves in order) in a caller-provided workspace,
// then a finalising kernel that adds them in a fixed order.  No floating-point atomics: two calls give the same bits in either deterministic mode.
//
// The file is compiled with -ffp-contract=off: the metric's operands are formed in f32 as torch forms them (an add, a multiply, a rounding half to
// even); a fused multiply-add there moves pixels across a rounding boundary.
#include "common.h"
#include "ordered.h"

#define SSIM_THREADS 256
// output tiles.  The f64 row-pass maps of the metric are the large item: 5 x (16 + 10) x 32 doubles = 33 KB, 42 KB with the staged images -- three
// workgroups per CU.  The loss's backward holds 5 x 20 x 66 floats of row sums, the 20 x 68 images and three 18 x 66 adjoint maps: 52 KB.
#define SSIM_MET_R 5
#define SSIM_MET_TY 16
#define SSIM_MET_TX 32
#define SSIM_LOSS_R 1
#define SSIM_LOSS_TY 16
#define SSIM_LOSS_TX 64

template <typename T, int R> struct SsimArgs {
    const float* x;  // the synthesised view (the gradient is with respect to it)
    const float* y;  // the label
    float mean[3];
    int C, H, W, tiles_x, tiles_y;
    T c1, c2;
    T g[2 * R + 1];  // 1-D window weights, sum 1; the window is their outer product
};

// a * b + c: one fused multiply-add in f32 (the loss: the training step's arithmetic), a multiply and an add in f64 (the metric keeps the plain
// f64 chain of metrics.hip; the file's -ffp-contract=off holds for everything that is not spelled out here)
__device__ __forceinline__ float mad(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double mad(double a, double b, double c) { return a * b + c; }

// ---- windowed moments, written once -----------------------------------------------------------------------------------------------------------
// xs, ys: (OH + 2R) x (OW + 2R) staged values in LDS (complete: the caller has synchronised).  rowm: 5 x (OH + 2R) x OW values of LDS.
// f(r, c, mx, my, mxx, myy, mxy) is called once for every window centre (r, c) of the OH x OW region, with the weighted sums of x, y, x^2, y^2, x y
// over the window whose top-left staged element is (r, c).  Ends without a barrier.
template <typename T, int R, int OH, int OW, typename F>
__device__ __forceinline__ void windowed_moments(const float* xs, const float* ys, const T (&g)[2 * R + 1], T* rowm, F&& f) {
    constexpr int IH = OH + 2 * R, IW = OW + 2 * R, PL = IH * OW;
    for (int i = threadIdx.x; i < PL; i += SSIM_THREADS) {  // row pass
        const int r = i / OW, c = i - r * OW;
        const float* px = xs + r * IW + c;
        const float* py = ys + r * IW + c;
        T sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            const T xv = (T)px[k], yv = (T)py[k], w = g[k];
            sx = mad(w, xv, sx);
            sy = mad(w, yv, sy);
            sxx = mad(w, xv * xv, sxx);
            syy = mad(w, yv * yv, syy);
            sxy = mad(w, xv * yv, sxy);
        }
        rowm[i] = sx;
        rowm[PL + i] = sy;
        rowm[2 * PL + i] = sxx;
        rowm[3 * PL + i] = syy;
        rowm[4 * PL + i] = sxy;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OH * OW; i += SSIM_THREADS) {  // column pass
        const int r = i / OW, c = i - r * OW;
        const T* p = rowm + r * OW + c;
        T m[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            const T w = g[k];
#pragma unroll
            for (int j = 0; j < 5; ++j) m[j] = mad(w, p[j * PL + k * OW], m[j]);
        }
        f(r, c, m[0], m[1], m[2], m[3], m[4]);
    }
}

// ---- the kernel: metric, loss value, loss value + gradient, gradient alone --------------------------------------------------------------------
// METRIC: operands x = rint(clamp((x + mean) * 255, 0, 255)), y = (y + mean) * 255 (get_psnr's), the partial sum is of S.
// loss  : operands x + mean, y + mean, the partial sum is of (1 - S) / 2.
// GRAD  : ga (+)= the adjoint, upstream scalar u = -gscale[0] * scale_grad / 2 per window; every element of ga is written.
// partials: one double per workgroup, or nullptr (gradient alone).
template <typename T, int R, int TY, int TX, bool GRAD, bool METRIC>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_kernel(SsimArgs<T, R> a, float scale_grad, const float* __restrict__ gscale, float* __restrict__ ga,
                                                            int add, double* __restrict__ partials) {
    constexpr int E = GRAD ? R : 0;  // window centres beyond the tile on each side
    constexpr int OH = TY + 2 * E, OW = TX + 2 * E, IH = OH + 2 * R, IW = OW + 2 * R;
    __shared__ float xs[IH * IW], ys[IH * IW];
    __shared__ T rowm[5 * IH * OW];
    __shared__ float adj[GRAD ? 3 * OH * OW : 1];
    __shared__ double red[SSIM_THREADS / 64];
    const int tile = blockIdx.x;
    const int tx0 = (tile % a.tiles_x) * TX, ty0 = ((tile / a.tiles_x) % a.tiles_y) * TY, plane = tile / (a.tiles_x * a.tiles_y);
    const float mean = a.mean[plane % a.C];
    const size_t base = (size_t)plane * a.H * a.W;
    for (int i = threadIdx.x; i < IH * IW; i += SSIM_THREADS) {  // stage the tile with its halo; 0 outside the image (those windows are not valid)
        const int ly = i / IW, lx = i - ly * IW;
        const int y = ty0 - E - R + ly, x = tx0 - E - R + lx;
        float xv = 0.f, yv = 0.f;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const size_t o = base + (size_t)y * a.W + x;
            xv = a.x[o] + mean;
            yv = a.y[o] + mean;
            if (METRIC) {
                xv = rintf(fminf(fmaxf(xv * 255.f, 0.f), 255.f));  // torch.round: half to even
                yv = yv * 255.f;
            }
        }
        xs[i] = xv;
        ys[i] = yv;
    }
    __syncthreads();
    const T u = GRAD ? (T)(-0.5f * scale_grad * (gscale ? gscale[0] : 1.f)) : (T)0;
    T acc = 0;
    windowed_moments<T, R, OH, OW>(xs, ys, a.g, rowm, [&](int r, int c, T mx, T my, T mxx, T myy, T mxy) {
        const int py = ty0 - E + r, px = tx0 - E + c;  // the window's centre in the image
        const bool valid = py >= R && py < a.H - R && px >= R && px < a.W - R;
        const T vx = mxx - mx * mx, vy = myy - my * my, cxy = mxy - mx * my;
        const T n1 = 2 * (mx * my) + a.c1, n2 = 2 * cxy + a.c2, d1 = mx * mx + my * my + a.c1, d2 = vx + vy + a.c2;
        const T dd = d1 * d2, S = n1 * n2 / dd;
        if (valid && r >= E && r < E + TY && c >= E && c < E + TX) acc += METRIC ? S : (1 - S) / 2;  // every valid centre is in one tile
        if constexpr (GRAD) {
            const T id1 = 1 / d1, id2 = 1 / d2, idd = id1 * id2;
            const T s_mx = 2 * my * n2 * idd - 2 * mx * S * id1, s_vx = -S * id2, s_cxy = 2 * n1 * idd;
            const int o = r * OW + c;
            adj[o] = valid ? (float)(u * (s_mx - 2 * mx * s_vx - my * s_cxy)) : 0.f;  // A
            adj[OH * OW + o] = valid ? (float)(2 * u * s_vx) : 0.f;                     // Bm
            adj[2 * OH * OW + o] = valid ? (float)(u * s_cxy) : 0.f;                    // Cm
        }
    });
    if constexpr (GRAD) {
        __syncthreads();
        // a thread owns RPT vertically adjacent pixels of one column: the windows that contain them have their centres within R, so the three adjoint
        // maps are summed along x once per row (RPT + 2R rows), then along y per pixel
        constexpr int RPT = TY * TX / SSIM_THREADS;
        static_assert(TY * TX % SSIM_THREADS == 0 && SSIM_THREADS % TX == 0, "a thread owns whole column pieces");
        const int lx = threadIdx.x % TX, ly0 = (threadIdx.x / TX) * RPT;
        T h[3][RPT + 2 * R];
#pragma unroll
        for (int rr = 0; rr < RPT + 2 * R; ++rr) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const float* p = adj + m * OH * OW + (ly0 + rr) * OW + lx;
                T t = 0;
#pragma unroll
                for (int dx = 0; dx <= 2 * R; ++dx) t = mad(a.g[dx], (T)p[dx], t);
                h[m][rr] = t;
            }
        }
        const int x = tx0 + lx;
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int ly = ly0 + r, y = ty0 + ly;
            if (y >= a.H || x >= a.W) continue;
            T sa = 0, sb = 0, sc = 0;
#pragma unroll
            for (int dy = 0; dy <= 2 * R; ++dy) {
                sa = mad(a.g[dy], h[0][r + dy], sa);
                sb = mad(a.g[dy], h[1][r + dy], sb);
                sc = mad(a.g[dy], h[2][r + dy], sc);
            }
            const int q = (ly + E + R) * IW + lx + E + R;
            const float gq = (float)mad(sc, (T)ys[q], mad(sb, (T)xs[q], sa));
            const size_t o = base + (size_t)y * a.W + x;
            ga[o] = add ? ga[o] + gq : gq;
        }
    }
    if (partials) {  // block-uniform
        double v = wave_sum_f64((double)acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int i = 0; i < SSIM_THREADS / 64; ++i) s += red[i];
            partials[blockIdx.x] = s;
        }
    }
}

// ---- finaliser: the n partial sums in a fixed order -> the metric's column, or the loss scalar -------------------------------------------------
// thread t adds partials t, t + 256, ... in that order, thread 0 then adds the 256 sums in index order.  The plain sum is left in partials[n], the
// workspace's last word, for a caller that wants the term by itself (the training step reports it beside the weighted total it joins).
__global__ __launch_bounds__(SSIM_THREADS) void ssim_finalize_kernel(double* __restrict__ partials, int n, double count, double* __restrict__ row,
                                                                     float scale, float* __restrict__ out, int accumulate) {
    __shared__ double s[SSIM_THREADS];
    double t = 0.0;
    for (int i = threadIdx.x; i < n; i += SSIM_THREADS) t += partials[i];
    s[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int i = 0; i < SSIM_THREADS; ++i) total += s[i];
    partials[n] = total;
    if (row) row[FALNET_MET_SSIM] = total / count;
    else out[0] = (accumulate ? out[0] : 0.f) + (float)((double)scale * total);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
static inline int64_t ssim_tiles(int planes, int H, int W, int ty, int tx) { return (int64_t)planes * ((H + ty - 1) / ty) * ((W + tx - 1) / tx); }

extern "C" int64_t falnet_ssim_workspace_bytes(int B, int C, int H, int W, int radius) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || (radius != SSIM_MET_R && radius != SSIM_LOSS_R)) return 0;
    return 8 * (1 + (radius == SSIM_MET_R ? ssim_tiles(B * C, H, W, SSIM_MET_TY, SSIM_MET_TX) : ssim_tiles(B * C, H, W, SSIM_LOSS_TY, SSIM_LOSS_TX)));
}

extern "C" int falnet_ssim_metric(const float* out, const float* label, float mean_r, float mean_g, float mean_b, int B, int H, int W, double* row,
                                  void* workspace, void* stream) {
    FALNET_ENTER(stream);
    constexpr int R = SSIM_MET_R;
    FALNET_CHECK_ARG(out && label && row && workspace, "ssim_metric: null argument");
    FALNET_CHECK_ARG(B > 0 && H >= 2 * R + 1 && W >= 2 * R + 1, "ssim_metric: %d x %d x %d is smaller than one %d x %d window", B, H, W, 2 * R + 1, 2 * R + 1);
    FALNET_CHECK_ARG((int64_t)B * 3 * H * W < ((int64_t)1 << 31), "ssim_metric: more than 2^31 values");
    FALNET_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)row & 7) == 0, "ssim_metric: workspace and row must be 8-byte aligned");
    SsimArgs<double, R> a;
    a.x = out, a.y = label;
    a.mean[0] = mean_r, a.mean[1] = mean_g, a.mean[2] = mean_b;
    a.C = 3, a.H = H, a.W = W;
    a.tiles_x = (W + SSIM_MET_TX - 1) / SSIM_MET_TX, a.tiles_y = (H + SSIM_MET_TY - 1) / SSIM_MET_TY;
    a.c1 = (0.01 * 255) * (0.01 * 255), a.c2 = (0.03 * 255) * (0.03 * 255);
    double sum = 0.0;
    for (int k = 0; k <= 2 * R; ++k) sum += (a.g[k] = exp(-(double)((k - R) * (k - R)) / (2.0 * 1.5 * 1.5)));
    for (int k = 0; k <= 2 * R; ++k) a.g[k] /= sum;
    const int n = (int)ssim_tiles(B * 3, H, W, SSIM_MET_TY, SSIM_MET_TX);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ssim_kernel<double, R, SSIM_MET_TY, SSIM_MET_TX, false, true>), dim3(n), dim3(SSIM_THREADS), 0, (hipStream_t)stream, a,
                       0.f, (const float*)nullptr, (float*)nullptr, 0, (double*)workspace);
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3(1), dim3(SSIM_THREADS), 0, (hipStream_t)stream, (double*)workspace, n,
                       (double)B * 3.0 * (double)(H - 2 * R) * (double)(W - 2 * R), row, 0.f, (float*)nullptr, 0);
    FALNET_RETURN_LAUNCH();
}

// value (out != NULL) and / or gradient (ga != NULL) of the loss in one launch
static int ssim_loss_launch(const char* who, const float* synth, const float* label, float mean_r, float mean_g, float mean_b, int B, int C, int H, int W,
                            int radius, float scale_out, float* out, int accumulate, float scale_grad, const float* gscale, float* ga, int add,
                            void* workspace, void* stream) {
    constexpr int R = SSIM_LOSS_R;
    FALNET_CHECK_ARG(radius == R, "%s: the loss is built for the 3 x 3 window (radius 1), got radius %d", who, radius);
    FALNET_CHECK_ARG(synth && label && (out || ga) && (!out || workspace), "%s: null argument", who);
    FALNET_CHECK_ARG(B > 0 && C >= 1 && C <= 3, "%s: need B > 0 and 1 to 3 channels", who);
    FALNET_CHECK_ARG(H >= 2 * R + 1 && W >= 2 * R + 1, "%s: %d x %d is smaller than one %d x %d window", who, H, W, 2 * R + 1, 2 * R + 1);
    FALNET_CHECK_ARG((int64_t)B * C * H * W < ((int64_t)1 << 31), "%s: more than 2^31 values", who);
    FALNET_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
    SsimArgs<float, R> a;
    a.x = synth, a.y = label;
    a.mean[0] = mean_r, a.mean[1] = mean_g, a.mean[2] = mean_b;
    a.C = C, a.H = H, a.W = W;
    a.tiles_x = (W + SSIM_LOSS_TX - 1) / SSIM_LOSS_TX, a.tiles_y = (H + SSIM_LOSS_TY - 1) / SSIM_LOSS_TY;
    a.c1 = 0.01f * 0.01f, a.c2 = 0.03f * 0.03f;
    for (int k = 0; k <= 2 * R; ++k) a.g[k] = 1.f / 3.f;
    const int n = (int)ssim_tiles(B * C, H, W, SSIM_LOSS_TY, SSIM_LOSS_TX);
    double* partials = out ? (double*)workspace : nullptr;
    if (ga)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ssim_kernel<float, R, SSIM_LOSS_TY, SSIM_LOSS_TX, true, false>), dim3(n), dim3(SSIM_THREADS), 0, (hipStream_t)stream,
                           a, scale_grad, gscale, ga, add, partials);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ssim_kernel<float, R, SSIM_LOSS_TY, SSIM_LOSS_TX, false, false>), dim3(n), dim3(SSIM_THREADS), 0, (hipStream_t)stream,
                           a, 0.f, (const float*)nullptr, (float*)nullptr, 0, partials);
    if (out)
        hipLaunchKernelGGL(ssim_finalize_kernel, dim3(1), dim3(SSIM_THREADS), 0, (hipStream_t)stream, partials, n, 1.0, (double*)nullptr,
                           scale_out, out, accumulate);
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_ssim_loss_fwd(const float* synth, const float* label, float mean_r, float mean_g, float mean_b, int B, int C, int H, int W, int radius,
                                    float scale, float* out, int accumulate, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(out, "ssim_loss_fwd: null output");
    return ssim_loss_launch("ssim_loss_fwd", synth, label, mean_r, mean_g, mean_b, B, C, H, W, radius, scale, out, accumulate, 0.f, nullptr, nullptr, 0,
                            workspace, stream);
}

extern "C" int falnet_ssim_loss_bwd(const float* synth, const float* label, float mean_r, float mean_g, float mean_b, int B, int C, int H, int W, int radius,
                                    float scale, const float* gscale, float* ga, int accumulate, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(ga, "ssim_loss_bwd: null gradient");
    return ssim_loss_launch("ssim_loss_bwd", synth, label, mean_r, mean_g, mean_b, B, C, H, W, radius, 0.f, nullptr, 0, scale, gscale, ga, accumulate, nullptr,
                            stream);
}

extern "C" int falnet_ssim_loss_fwd_bwd(const float* synth, const float* label, float mean_r, float mean_g, float mean_b, int B, int C, int H, int W,
                                        int radius, float scale_out, float* out, float scale_grad, const float* gscale, float* ga, int add_grad,
                                        void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(out && ga, "ssim_loss_fwd_bwd: null output or gradient");
    return ssim_loss_launch("ssim_loss_fwd_bwd", synth, label, mean_r, mean_g, mean_b, B, C, H, W, radius, scale_out, out, 1, scale_grad, gscale, ga, add_grad,
                            workspace, stream);
}
