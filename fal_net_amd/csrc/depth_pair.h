// The per-pixel f64 depth chain of the depth metrics (myUtils.py:196-334), written ONCE for the kernels that count or order pixels by it: the
// median select and the error sums of metrics.hip and the sparsification curves of sparsify.hip.  The `< 1.25^n` counts are discontinuous in
// these values and the tests compare them with numpy's as integers, so every operation here is the host's, in the host's order.
// CONTRACT: every file that includes this header is compiled with -ffp-contract=off (_build.FILE_FLAGS; tests/test_sparsify_host.py holds
// it): no fused multiply-add, correctly rounded f64 division.
// Not part of common.h on purpose: that file is hashed into the autotune cache header (ops.py: _TUNE_SOURCES), this one is not.
#pragma once
#include "common.h"

struct DepthArgs {
    const float* pred;  // predicted disparity, H x W
    const float* gt;    // ground truth, H x W: a disparity (kitti2015) or a depth (eigen, make3d)
    int W, y0, x0, rh, rw;  // row pitch and the region that counts (the Eigen crop, or the whole frame)
    int mode;
    double fb;     // focal * baseline, formed by the caller exactly as the host chain forms it
    double max_d;  // make3d: the mask is 0 < gt < max_d
};

// pixel i of the region -> (gt depth, predicted depth) in f64 as the host forms them and idx, its flat index in the H x W maps; false where
// the ground truth is masked out.
//   kitti2015: depth = fb / (d + (1 - [d > 0])) for both maps; eigen / make3d: gt is a depth already.  A prediction <= 0 takes the d + 1 denominator.
__device__ __forceinline__ bool depth_pair(const DepthArgs& a, uint32_t i, double& g, double& p, size_t& idx) {
    const uint32_t r = i / (uint32_t)a.rw, c = i - r * (uint32_t)a.rw;
    idx = (size_t)(a.y0 + r) * a.W + (a.x0 + c);
    const float gf = a.gt[idx];
    if (!(gf > 0.f)) return false;
    if (a.mode == FALNET_DEPTH_MAKE3D && !((double)gf < a.max_d)) return false;
    const float pf = a.pred[idx];
    p = a.fb / ((double)pf + (1.0 - (pf > 0.f ? 1.0 : 0.0)));
    g = a.mode == FALNET_DEPTH_KITTI2015 ? a.fb / ((double)gf + (1.0 - 1.0)) : (double)gf;
    return true;
}
__device__ __forceinline__ bool depth_pair(const DepthArgs& a, uint32_t i, double& g, double& p) {
    size_t idx;
    return depth_pair(a, i, g, p, idx);
}

// the optional median scale, the clamp of both depths to [min_d, max_d] (g and p are left clamped) -> t = max(g / p, p / g)
__device__ __forceinline__ double depth_scale_clamp(double& g, double& p, bool scaled, double factor, double min_d, double max_d) {
    if (scaled) p = factor * p;
    p = fmin(fmax(p, min_d), max_d);
    g = fmin(fmax(g, min_d), max_d);
    return fmax(g / p, p / g);
}

// host: the checks every entry point of the chain shares, and the region that counts.  `who` names the entry point in the messages.
static int depth_args(DepthArgs& a, const float* pred, const float* gt, int H, int W, int mode, double fb, double max_d, const char* who) {
    FALNET_CHECK_ARG(pred && gt, "%s: null map", who);
    FALNET_CHECK_ARG(mode == FALNET_DEPTH_KITTI2015 || mode == FALNET_DEPTH_EIGEN || mode == FALNET_DEPTH_MAKE3D,
                     "%s: unknown mode %d (0 kitti2015, 1 eigen, 2 make3d)", who, mode);
    FALNET_CHECK_ARG(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "%s: frame %d x %d must hold between 1 and 2^31 pixels", who, H, W);
    FALNET_CHECK_ARG(fb > 0.0, "%s: focal * baseline must be positive", who);
    a.pred = pred, a.gt = gt, a.W = W, a.mode = mode, a.fb = fb, a.max_d = max_d;
    a.y0 = 0, a.x0 = 0, a.rh = H, a.rw = W;
    if (mode == FALNET_DEPTH_EIGEN) {  // rows H - 219 : H - 4, columns 44 : 1180 (myUtils.py:256-277)
        FALNET_CHECK_ARG(H >= 219 && W >= 1180, "%s: frame %d x %d is smaller than the Eigen crop (rows H - 219 : H - 4, columns 44 : 1180)", who, H, W);
        a.y0 = H - 219, a.x0 = 44, a.rh = 215, a.rw = 1136;
    }
    return 0;
}
