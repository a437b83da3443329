// Triangle mesh of one sample's predicted depth: the pixel grid triangulated, cut where depth jumps, re-indexed and written as binary-PLY
// vertex and face records in order (include/falnet_hip.h; the numpy restatement is tests/_mesh_ref.py).
//   vertex g = i W + j   the point cloud's vertex of that pixel (pc_vertex.h), valid when min_depth < z <= max_depth on the capped f32 z and, with a
//                        score map, score >= threshold (every comparison with a NaN is false);
//   quad (i, j)          corners a = (i, j), b = (i, j + 1), c = (i + 1, j), d = (i + 1, j + 1); two or more invalid corners: no triangle; one: the
//                        diagonal that avoids it; none: a-d iff |za - zd| <= |zb - zc| (f32), else b-c;
//   triangles            a-d: T0 = (a, c, d), T1 = (a, d, b); b-c: T0 = (a, c, b), T1 = (b, c, d); kept when the three vertices are valid and every
//                        edge (p, q) has max(zp, zq) <= min(zp, zq) * ratio, one f32 multiply, ratio = (float)(1 + max_jump);
//   output               the vertices some kept triangle names, in pixel order; the kept triangles in quad order, T0 before T1, with the new indices.
// Five kernels and the offset scan of compact.hip twice; no atomic, nothing decides a position but the index (the ordered compaction of ordered.h):
//   1  mesh_code_kernel     one thread per pixel = per quad origin: the z of its four corners again from the disparity (neighbouring threads read the
//                           same lines: the map is read from HBM once), one code byte per pixel -- bit 0 T0 kept, bit 1 T1 kept, bit 2 diagonal b-c;
//                           0 in the last row and column
//   2  mesh_count_kernel    workgroup g counts the used vertices (a vertex reads the codes of its four quads) and the kept faces of its ORD_TILE pixels
//   3  falnet_offset_scan   for each of the two count arrays -> exclusive offsets, counts_dev[0] and counts_dev[1]
//   4  mesh_vertex_kernel   the used flags again, ranked; the record (with its normal: a gather over the up to six kept triangles around the vertex,
//                           f64, fixed order) and the int32 index map, -1 for an unused pixel
//   5  mesh_face_kernel     the codes again, T0 and T1 ranked by two block_rank calls; the 13-byte records with the map's indices
// The 15-, 27- and 13-byte records are unaligned, but the records of one round of one workgroup are CONSECUTIVE in the output: they are laid out in
// LDS at the byte phase of their first output byte and leave as whole dwords, coalesced -- at most 7 dword stores per thread and round where byte
// stores (compact.hip) would be 27 (or 2 x 13).  The first and last dword of a round may be shared with a neighbouring round: those alone are written
// byte by byte, each byte by its one owner, so nothing is read back and nothing beyond the kept records is written.
// Every + - * / and sqrt is a correctly rounded operation in the stated order: the file is compiled with -ffp-contract=off.
// Not on the training step's path, not replayable, and not part of the autotune key (ops.py: _TUNE_SOURCES).
#include <math.h>
#include "common.h"
#include "ordered.h"
#include "pc_vertex.h"

#define MS_THREADS ORD_THREADS
#define MS_ROUNDS ORD_ROUNDS
#define MS_TILE ORD_TILE
#define MS_FACE 13    // uchar 3, three little-endian int32
#define MS_MAX_Z 200  // pc_vertex.h caps z here: max_depth stays below it, so a valid vertex is never a capped one

struct MeshArgs {  // by value in the kernel arguments
    const float* img;
    const float* disp;
    const float* score;
    PcParams p;
    float threshold, min_depth, max_depth, ratio;
    uint32_t n;  // H W
};

// the capped z of pixel g < a.n when its vertex is valid, a NaN when it is not: one float carries both
__device__ __forceinline__ float mesh_z(const MeshArgs& a, uint32_t g) {
    const float z = pc_depth(a.p, a.disp[g]);
    bool ok = z > a.min_depth && z <= a.max_depth;
    if (ok && a.score) ok = a.score[g] >= a.threshold;
    return ok ? z : __uint_as_float(0x7fc00000u);
}

__device__ __forceinline__ bool mesh_edge(float zp, float zq, float ratio) { return fmaxf(zp, zq) <= __fmul_rn(fminf(zp, zq), ratio); }

// the code byte of a quad from the z of its corners (NaN: invalid)
__device__ __forceinline__ uint32_t mesh_quad_code(float za, float zb, float zc, float zd, float ratio) {
    const bool va = za == za, vb = zb == zb, vc = zc == zc, vd = zd == zd;
    const int bad = (int)!va + (int)!vb + (int)!vc + (int)!vd;
    if (bad >= 2) return 0;
    const bool bc = bad == 1 ? (!va || !vd) : !(fabsf(__fsub_rn(za, zd)) <= fabsf(__fsub_rn(zb, zc)));
    bool t0, t1;
    if (!bc) {  // T0 = (a, c, d), T1 = (a, d, b)
        const bool ad = va && vd && mesh_edge(za, zd, ratio);
        t0 = ad && vc && mesh_edge(za, zc, ratio) && mesh_edge(zc, zd, ratio);
        t1 = ad && vb && mesh_edge(zd, zb, ratio) && mesh_edge(zb, za, ratio);
    } else {  // T0 = (a, c, b), T1 = (b, c, d)
        const bool cb = vb && vc && mesh_edge(zc, zb, ratio);
        t0 = cb && va && mesh_edge(za, zc, ratio) && mesh_edge(zb, za, ratio);
        t1 = cb && vd && mesh_edge(zc, zd, ratio) && mesh_edge(zd, zb, ratio);
    }
    return (t0 ? 1u : 0u) | (t1 ? 2u : 0u) | (bc ? 4u : 0u);
}

__global__ __launch_bounds__(MS_THREADS) void mesh_code_kernel(MeshArgs a, unsigned char* __restrict__ codes) {
    const uint32_t g = blockIdx.x * MS_THREADS + threadIdx.x;
    if (g >= a.n) return;
    const uint32_t W = (uint32_t)a.p.W, i = g / W, j = g - i * W;
    uint32_t code = 0;
    if (i + 1 < (uint32_t)a.p.H && j + 1 < W)  // g + W + 1 < n
        code = mesh_quad_code(mesh_z(a, g), mesh_z(a, g + 1), mesh_z(a, g + W), mesh_z(a, g + W + 1), a.ratio);
    codes[g] = (unsigned char)code;
}

// The kept triangles around vertex (i, j), g = i W + j < n: c[q] is the code of quad q of (i - 1, j - 1), (i - 1, j), (i, j - 1), (i, j) -- the vertex
// is its corner d, c, b, a -- or 0 where the image has no such quad; bit 2 q + t of the result: triangle t of quad q is kept and contains the vertex.
__device__ __forceinline__ uint32_t mesh_incident(const unsigned char* __restrict__ codes, uint32_t g, uint32_t i, uint32_t j, uint32_t W, uint32_t (&c)[4]) {
    c[0] = (i > 0 && j > 0) ? codes[g - W - 1] : 0u;
    c[1] = i > 0 ? codes[g - W] : 0u;  // the last column's code is 0
    c[2] = j > 0 ? codes[g - 1] : 0u;  // as is the last row's
    c[3] = codes[g];
    // which of T0, T1 contain the corner: a: a-d both, b-c T0; b: a-d T1, b-c both; c: a-d T0, b-c both; d: a-d both, b-c T1
    const uint32_t in_d = (c[0] & 4u) ? 2u : 3u, in_c = (c[1] & 4u) ? 3u : 1u, in_b = (c[2] & 4u) ? 3u : 2u, in_a = (c[3] & 4u) ? 1u : 3u;
    return (c[0] & in_d) | ((c[1] & in_c) << 2) | ((c[2] & in_b) << 4) | ((c[3] & in_a) << 6);
}

__global__ __launch_bounds__(MS_THREADS) void mesh_count_kernel(const unsigned char* __restrict__ codes, uint32_t n, uint32_t W, int64_t* __restrict__ counts_v,
                                                                int64_t* __restrict__ counts_f) {
    __shared__ int wsum_v[MS_THREADS / 64], wsum_f[MS_THREADS / 64];
    const uint32_t base = blockIdx.x * MS_TILE;
    int cv = 0, cf = 0;
#pragma unroll
    for (int r = 0; r < MS_ROUNDS; ++r) {
        const uint32_t g = base + r * MS_THREADS + threadIdx.x;
        if (g < n) {
            const uint32_t i = g / W, j = g - i * W;
            uint32_t c[4];
            cv += mesh_incident(codes, g, i, j, W, c) != 0u ? 1 : 0;
            cf += __popc(c[3] & 3u);
        }
    }
    const int tv = block_count(cv, wsum_v), tf = block_count(cf, wsum_f);
    if (threadIdx.x == 0) {
        counts_v[blockIdx.x] = (int64_t)tv;
        counts_f[blockIdx.x] = (int64_t)tf;
    }
}

// The `nbytes` output bytes from byte o0 of `out` on, staged in LDS so that byte s + k of `stage` is output byte o0 + k, s = o0 & 3: whole dwords where
// all four bytes are this round's, single bytes in the first and last dword where they are not.  `out` is 4-byte aligned.  Every thread calls it, after
// the barrier that ends the staging.
__device__ __forceinline__ void mesh_flush(const uint32_t* stage, unsigned char* __restrict__ out, int64_t o0, int nbytes) {
    const int s = (int)(o0 & 3), end = s + nbytes, ndw = (end + 3) >> 2;
    unsigned char* first = out + (o0 - s);  // the dword that holds output byte o0
    for (int d = threadIdx.x; d < ndw; d += MS_THREADS) {
        const uint32_t w = stage[d];
        const int lo = d == 0 ? s : 0, hi = end - 4 * d < 4 ? end - 4 * d : 4;
        if (lo == 0 && hi == 4) {
            reinterpret_cast<uint32_t*>(first)[d] = w;
        } else {
            for (int k = lo; k < hi; ++k) first[4 * d + k] = (unsigned char)(w >> (8 * k));
        }
    }
}

// REC bytes of the little-endian dwords w to byte `at` of the staging buffer
template <int REC, int NW>
__device__ __forceinline__ void mesh_stage(uint32_t* stage, int at, const uint32_t (&w)[NW]) {
    unsigned char* sb = reinterpret_cast<unsigned char*>(stage) + at;
#pragma unroll
    for (int k = 0; k < REC; ++k) sb[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
}

struct MeshPoint { double x, y, z; };  // PLY axes: the record's three floats

// (V1 - V0) x (V2 - V0) added to n: each component two products and a subtraction
__device__ __forceinline__ void mesh_add_cross(const MeshPoint& v0, const MeshPoint& v1, const MeshPoint& v2, double (&n)[3]) {
    const double ax = v1.x - v0.x, ay = v1.y - v0.y, az = v1.z - v0.z;
    const double bx = v2.x - v0.x, by = v2.y - v0.y, bz = v2.z - v0.z;
    n[0] += ay * bz - az * by;
    n[1] += az * bx - ax * bz;
    n[2] += ax * by - ay * bx;
}

__device__ __forceinline__ MeshPoint mesh_pick(bool second, const MeshPoint& p, const MeshPoint& q) {
    MeshPoint o;
    o.x = second ? q.x : p.x, o.y = second ? q.y : p.y, o.z = second ? q.z : p.z;
    return o;
}

// the normal of used vertex (i, j): the sum over its kept triangles `inc` (mesh_incident) in quad order, T0 before T1, normalised
__device__ __forceinline__ void mesh_normal(const MeshArgs& a, uint32_t i, uint32_t j, const uint32_t (&c)[4], uint32_t inc, float (&out)[3]) {
    const int H = a.p.H, W = a.p.W;
    MeshPoint P[3][3];  // the 3 x 3 pixels around the vertex; a pixel outside the image is clamped into it and belongs to no kept triangle
#pragma unroll
    for (int di = 0; di < 3; ++di)
#pragma unroll
        for (int dj = 0; dj < 3; ++dj) {
            int ii = (int)i + di - 1, jj = (int)j + dj - 1;
            ii = ii < 0 ? 0 : (ii > H - 1 ? H - 1 : ii);
            jj = jj < 0 ? 0 : (jj > W - 1 ? W - 1 : jj);
            float x, z, ny;
            pc_position(a.p, a.disp[(uint32_t)ii * (uint32_t)W + (uint32_t)jj], (uint32_t)ii, (uint32_t)jj, x, z, ny);
            P[di][dj].x = (double)x, P[di][dj].y = (double)z, P[di][dj].z = (double)ny;
        }
    double n[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int oi = q >> 1, oj = q & 1;  // quad q starts at (i - 1 + oi, j - 1 + oj)
        const MeshPoint &A = P[oi][oj], &B = P[oi][oj + 1], &C = P[oi + 1][oj], &D = P[oi + 1][oj + 1];
        const bool bc = (c[q] & 4u) != 0u;
        if (inc & (1u << (2 * q))) mesh_add_cross(A, C, mesh_pick(bc, D, B), n);                                          // (a, c, d) or (a, c, b)
        if (inc & (2u << (2 * q))) mesh_add_cross(mesh_pick(bc, A, B), mesh_pick(bc, D, C), mesh_pick(bc, B, D), n);  // (a, d, b) or (b, c, d)
    }
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool ok = len > 0.0 && len < (double)INFINITY;  // false for a NaN
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = ok ? (float)(n[k] / len) : 0.f;
}

template <bool NORMALS>
__global__ __launch_bounds__(MS_THREADS) void mesh_vertex_kernel(MeshArgs a, const unsigned char* __restrict__ codes, const int64_t* __restrict__ offsets,
                                                                 unsigned char* __restrict__ out, int32_t* __restrict__ map) {
    constexpr int REC = NORMALS ? 27 : 15, NW = (REC + 3) / 4;
    __shared__ int wsum[MS_THREADS / 64];
    __shared__ uint32_t stage[(MS_THREADS * REC + 3) / 4 + 1];
    const uint32_t base = blockIdx.x * MS_TILE, W = (uint32_t)a.p.W;
    int64_t pos = offsets[blockIdx.x];
    for (int r = 0; r < MS_ROUNDS; ++r) {
        const uint32_t g = base + r * MS_THREADS + threadIdx.x;
        uint32_t c[4], inc = 0, i = 0, j = 0;
        if (g < a.n) {
            i = g / W, j = g - i * W;
            inc = mesh_incident(codes, g, i, j, W, c);
        }
        const bool keep = inc != 0u;
        int total;
        const int rank = block_rank(keep, wsum, total);
        if (g < a.n) map[g] = keep ? (int32_t)(pos + rank) : -1;
        const int64_t o0 = pos * REC;
        if (keep) {
            const PcVertex v = pc_vertex(a.img, a.disp, a.p, g);
            uint32_t w[NW];
            w[0] = __float_as_uint(v.x), w[1] = __float_as_uint(v.z), w[2] = __float_as_uint(v.ny);
            if (NORMALS) {
                float nrm[3];
                mesh_normal(a, i, j, c, inc, nrm);
                w[3] = __float_as_uint(nrm[0]), w[4] = __float_as_uint(nrm[1]), w[5] = __float_as_uint(nrm[2]);
            }
            w[NW - 1] = trunc_u8(v.r) | (trunc_u8(v.g) << 8) | (trunc_u8(v.b) << 16);
            mesh_stage<REC, NW>(stage, (int)(o0 & 3) + rank * REC, w);
        }
        __syncthreads();
        mesh_flush(stage, out, o0, total * REC);  // the next round stages behind the two barriers of its block_rank
        pos += total;
    }
}

__global__ __launch_bounds__(MS_THREADS) void mesh_face_kernel(const unsigned char* __restrict__ codes, const int32_t* __restrict__ map, uint32_t n, uint32_t W,
                                                               const int64_t* __restrict__ offsets, unsigned char* __restrict__ out) {
    __shared__ int wsum[MS_THREADS / 64];
    __shared__ uint32_t stage[(2 * MS_THREADS * MS_FACE + 3) / 4 + 1];
    const uint32_t base = blockIdx.x * MS_TILE;
    int64_t pos = offsets[blockIdx.x];
    for (int r = 0; r < MS_ROUNDS; ++r) {
        const uint32_t g = base + r * MS_THREADS + threadIdx.x;
        uint32_t code = g < n ? codes[g] : 0u;
        if ((uint64_t)g + W + 1 >= n) code = 0;  // a quad's corners are pixels of the image (the code kernel leaves 0 here anyway)
        const bool k0 = (code & 1u) != 0u, k1 = (code & 2u) != 0u;
        int t0, t1;
        const int r0 = block_rank(k0, wsum, t0);
        const int r1 = block_rank(k1, wsum, t1);
        const int64_t o0 = pos * MS_FACE;
        if (k0 || k1) {
            // the faces of the round's quads below this one: their T0 plus their T1.  block_rank counts the kept threads BELOW the caller, so its
            // value is that count for a quad that keeps only the other triangle too
            const int32_t ia = map[g], ib = map[g + 1], ic = map[g + W], id = map[g + W + 1];
            const bool bc = (code & 4u) != 0u;
            const int first = r0 + r1;
            uint32_t w[4];
            if (k0) {  // (a, c, d) or (a, c, b)
                const uint32_t v0 = (uint32_t)ia, v1 = (uint32_t)ic, v2 = (uint32_t)(bc ? ib : id);
                w[0] = 3u | (v0 << 8), w[1] = (v0 >> 24) | (v1 << 8), w[2] = (v1 >> 24) | (v2 << 8), w[3] = v2 >> 24;
                mesh_stage<MS_FACE, 4>(stage, (int)(o0 & 3) + first * MS_FACE, w);
            }
            if (k1) {  // (a, d, b) or (b, c, d)
                const uint32_t v0 = (uint32_t)(bc ? ib : ia), v1 = (uint32_t)(bc ? ic : id), v2 = (uint32_t)(bc ? id : ib);
                w[0] = 3u | (v0 << 8), w[1] = (v0 >> 24) | (v1 << 8), w[2] = (v1 >> 24) | (v2 << 8), w[3] = v2 >> 24;
                mesh_stage<MS_FACE, 4>(stage, (int)(o0 & 3) + (first + (k0 ? 1 : 0)) * MS_FACE, w);
            }
        }
        __syncthreads();
        mesh_flush(stage, out, o0, (t0 + t1) * MS_FACE);
        pos += t0 + t1;
    }
}

static int64_t mesh_blocks(int64_t n) { return (n + MS_TILE - 1) / MS_TILE; }
static int64_t mesh_round8(int64_t v) { return (v + 7) & ~(int64_t)7; }
static bool mesh_shape_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 28); }

// workspace: the two count arrays side by side, the int32 index map, the code bytes
extern "C" int64_t falnet_mesh_workspace_bytes(int H, int W) {
    if (!mesh_shape_ok(H, W)) return 0;
    const int64_t n = (int64_t)H * W;
    return 2 * mesh_blocks(n) * (int64_t)sizeof(int64_t) + mesh_round8(4 * n) + mesh_round8(n);
}

extern "C" int falnet_mesh_build(const float* img, float mean_r, float mean_g, float mean_b, float rgb_scale, const float* disp, double focal, double baseline,
                                 const float* score, float threshold, float min_depth, float max_depth, double max_jump, int H, int W, int with_normals,
                                 void* vertices_out, void* faces_out, int64_t* counts_dev, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(mesh_shape_ok(H, W), "mesh_build: map %d x %d must hold between 1 and 2^28 pixels", H, W);
    FALNET_CHECK_ARG(img && disp, "mesh_build: null image or disparity");
    FALNET_CHECK_ARG(vertices_out && faces_out, "mesh_build: null output");
    FALNET_CHECK_ARG(counts_dev && workspace, "mesh_build: null counts or workspace");
    FALNET_CHECK_ARG(focal > 0.0, "mesh_build: focal length must be positive");
    FALNET_CHECK_ARG(min_depth >= 0.f && min_depth < max_depth && max_depth < (float)MS_MAX_Z, "mesh_build: need 0 <= min_depth < max_depth < %d, got %g and %g", MS_MAX_Z,
                     (double)min_depth, (double)max_depth);
    FALNET_CHECK_ARG(max_jump >= 0.0, "mesh_build: max_jump %g must be >= 0 (infinity keeps every valid triangle)", max_jump);
    FALNET_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)counts_dev) & 7) == 0, "mesh_build: workspace and counts must be 8-byte aligned");
    FALNET_CHECK_ARG((((uintptr_t)vertices_out | (uintptr_t)faces_out | (uintptr_t)img | (uintptr_t)disp | (uintptr_t)score) & 3) == 0,
                     "mesh_build: maps and outputs must be 4-byte aligned (the records leave as whole dwords)");
    hipStream_t st = (hipStream_t)stream;
    if (H < 2 || W < 2) {  // no quad: counts (0, 0), nothing else written
        hipError_t e = hipMemsetAsync(counts_dev, 0, 2 * sizeof(int64_t), st);
        if (e != hipSuccess) {
            falnet_set_error("mesh_build: clearing the counts failed: %s", hipGetErrorString(e));
            return (int)e;
        }
        return 0;
    }
    MeshArgs a;
    a.img = img, a.disp = disp, a.score = score;
    a.p.m0 = mean_r, a.p.m1 = mean_g, a.p.m2 = mean_b, a.p.rgb_scale = rgb_scale;
    a.p.focal = (float)focal, a.p.fb = (float)(focal * baseline);
    a.p.cx = (float)(W / 2.0), a.p.cy = (float)(H / 2.0);
    a.p.H = H, a.p.W = W;
    a.threshold = threshold, a.min_depth = min_depth, a.max_depth = max_depth;
    a.ratio = (float)(1.0 + max_jump);
    a.n = (uint32_t)H * (uint32_t)W;
    const int64_t nb = mesh_blocks(a.n);
    int64_t* counts_v = static_cast<int64_t*>(workspace);
    int64_t* counts_f = counts_v + nb;
    int32_t* map = reinterpret_cast<int32_t*>(counts_f + nb);
    unsigned char* codes = reinterpret_cast<unsigned char*>(map) + mesh_round8(4 * (int64_t)a.n);
    const dim3 threads(MS_THREADS), tiles((unsigned)nb);
    hipLaunchKernelGGL(mesh_code_kernel, dim3((a.n + MS_THREADS - 1) / MS_THREADS), threads, 0, st, a, codes);
    hipLaunchKernelGGL(mesh_count_kernel, tiles, threads, 0, st, (const unsigned char*)codes, a.n, (uint32_t)W, counts_v, counts_f);
    falnet_offset_scan(counts_v, nb, counts_dev, st);
    falnet_offset_scan(counts_f, nb, counts_dev + 1, st);
    if (with_normals)
        hipLaunchKernelGGL(mesh_vertex_kernel<true>, tiles, threads, 0, st, a, (const unsigned char*)codes, (const int64_t*)counts_v,
                           static_cast<unsigned char*>(vertices_out), map);
    else
        hipLaunchKernelGGL(mesh_vertex_kernel<false>, tiles, threads, 0, st, a, (const unsigned char*)codes, (const int64_t*)counts_v,
                           static_cast<unsigned char*>(vertices_out), map);
    hipLaunchKernelGGL(mesh_face_kernel, tiles, threads, 0, st, (const unsigned char*)codes, (const int32_t*)map, a.n, (uint32_t)W, (const int64_t*)counts_f,
                       static_cast<unsigned char*>(faces_out));
    FALNET_RETURN_LAUNCH();
}
