// The MED head's disparity planes, written once: the plane limit, the table's arithmetic and the shape check that the head (med_head.hip,
// med_head2.hip) and the readers of its logits (med_sweep.hip, med_stats.hip, med_pose.hip) share.  The sweep's t = 1 view is held to the head's
// p_im0 and the pure-baseline pose to the sweep bit for bit: both rest on these being the same operations in the same order everywhere.
#pragma once
#include <math.h>
#include "common.h"

#define MED_MAXN 128  // planes per sample

struct PlaneTab {  // the head's per-sample plane table in LDS
    float d[MED_MAXN];  // disparity of plane n in pixels (FAL_netB.py:223-225)
    float a[MED_MAXN];  // fractional part of the shift s_n = d_n (W-1)/W
    int k[MED_MAXN];    // integer part
};

// disparity of plane n of N in pixels: exponential spacing from min_disp (n = 0) to max_disp (n = N - 1)
__device__ __forceinline__ float med_plane_disp(float mn, float mx, int n, int N) {
    const float c = (float)n / (float)(N - 1);
    return mx * expf(logf(mx / mn) * (c - 1.0f));
}

// shift of a plane of disparity d in pixels of a row of W: 2d/W normalised * (W-1)/2 (align_corners=True)
__device__ __forceinline__ float med_plane_shift(float d, int W) { return d * (float)(W - 1) / (float)W; }

// a shift split into its integer part k and fraction a
__device__ __forceinline__ void med_split_shift(float s, int& k, float& a) {
    const float kf = floorf(s);
    k = (int)kf;
    a = s - kf;
}

// The shapes falnet_med_head_fwd accepts, for every entry point that takes the head's logits; `who` names the entry in the message and
// `wide` ends the width refusal.  The width limit is the head's backward LDS: its table and five rows of W + 3 floats in 160 KiB.
static inline int med_check_shape(const char* who, const char* wide, int B, int N, int H, int W) {
    FALNET_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: empty shape B=%d H=%d W=%d", who, B, H, W);
    FALNET_CHECK_ARG(N >= 2 && N <= MED_MAXN, "%s: N=%d outside [2,%d]", who, N, MED_MAXN);
    FALNET_CHECK_ARG((size_t)(W + 3) * 5 * sizeof(float) + sizeof(PlaneTab) <= 160 * 1024, "%s: W=%d too wide%s", who, W, wide);
    return 0;
}
