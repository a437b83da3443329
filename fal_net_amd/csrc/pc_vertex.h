// The point cloud's vertex (myUtils.py:339-373), written ONCE for dump.hip (falnet_point_cloud) and mesh.hip (falnet_mesh_build): a mesh vertex is
// the cloud's vertex of the same pixel, bit for bit.  Every operation is a correctly rounded f32 operation in the host's order; the includers are
// compiled with -ffp-contract=off.  Device code is __forceinline__ and there is no __global__ in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct PcParams {
    float m0, m1, m2, rgb_scale;  // colour = (img + mean) * rgb_scale
    float focal, fb;              // fb = focal * baseline, formed in double by the caller and rounded once (as torch does with the Python product)
    float cx, cy;                 // w / 2, h / 2
    int H, W;
};
struct PcVertex { float x, z, ny, r, g, b; };

// the geometry of pixel (i, j) with disparity d: x and -y from the UNCAPPED z, then z capped to [0, 200]
__device__ __forceinline__ void pc_position(const PcParams& p, float d, uint32_t i, uint32_t j, float& x, float& z, float& ny) {
    float zz = __fdiv_rn(p.fb, __fadd_rn(d, 1e-4f));
    const float u = (float)j + 0.5f, v = (float)i + 0.5f;  // affine_grid, align_corners=False: (grid + 1) / 2 * w
    x = __fmul_rn(__fdiv_rn(u - p.cx, p.focal), zz);
    ny = -__fmul_rn(__fdiv_rn(v - p.cy, p.focal), zz);
    zz = zz < 0.f ? 0.f : zz;
    z = zz > 200.f ? 200.f : zz;
}

// the capped z alone: what pc_position gives for the same disparity
__device__ __forceinline__ float pc_depth(const PcParams& p, float d) {
    float zz = __fdiv_rn(p.fb, __fadd_rn(d, 1e-4f));
    zz = zz < 0.f ? 0.f : zz;
    return zz > 200.f ? 200.f : zz;
}

// vertex g of the batch (g = b * H * W + i * W + j)
__device__ __forceinline__ PcVertex pc_vertex(const float* __restrict__ img, const float* __restrict__ disp, const PcParams& p, uint32_t g) {
    const uint32_t hw = (uint32_t)p.H * p.W, b = g / hw, pix = g - b * hw, i = pix / p.W, j = pix - i * p.W;
    PcVertex o;
    pc_position(p, disp[g], i, j, o.x, o.z, o.ny);
    const float* c = img + (size_t)b * 3 * hw + pix;
    o.r = __fmul_rn(__fadd_rn(c[0], p.m0), p.rgb_scale);
    o.g = __fmul_rn(__fadd_rn(c[hw], p.m1), p.rgb_scale);
    o.b = __fmul_rn(__fadd_rn(c[2 * (size_t)hw], p.m2), p.rgb_scale);
    return o;
}

// int() of the reference (truncation toward zero), saturated to a byte
__device__ __forceinline__ uint32_t trunc_u8(float v) { return v >= 255.f ? 255u : (v >= 1.f ? (uint32_t)v : 0u); }
