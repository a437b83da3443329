// Hole filling of a premultiplied image: background-biased pull-push (a normalised-convolution pyramid), inference only, not replayable.
//
// The definition is the one of include/falnet_hip.h (falnet_inpaint_fwd); in short, per image, with keep = weight >= floor:
//   level 0   w0 = keep ? weight : 0, c0 = keep ? values : 0, g = exp(-beta guide / guide_scale) (1 when beta = 0; guide is not read then)
//             stored triple (cg, wg, a) = (c0 g, w0 g, w0)                                    -- selects: nothing of a dropped pixel leaks
//   pull      a coarse cell sums its 2 x 2 (or fewer) fine cells as (f00 + f01) + (f10 + f11), then all C + 2 channels times 1 / a_sum if a_sum > 1
//   apex      F = div(cg, wg), G = div(wg, a), div(n, d) = d > 0 ? n / d : 0
//   push      UG = up(G'), U = div(up(F' G'), UG); F = a div(cg, wg) + (1 - a) U, G = a div(wg, a) + (1 - a) UG; out = c0 + (1 - w0) U
//             up(): the 2x tent filter, taps 1/4 and 3/4 clamped into the coarse level, rows first:
//             wy0 (wx0 X00 + wx1 X01) + wy1 (wx0 X10 + wx1 X11)
// Everywhere below a level's (F, G) is held as (P, G) with P = F G: the product rounds once, where it is made.
//
// Split.  `la` is the first level whose whole remaining pyramid (levels la..L, C + 2 channels) fits in the LDS of one
// workgroup.  The images of a call share every launch:
//   inpaint_pull_kernel   one workgroup per 64 x 64 tile of level l and image: forms level 0 from the inputs (or reads the stored triples of
//                         level l), pulls up to four levels in LDS and stores them (workspace: levels 1..L as [I][C + 2][H_l][W_l]).
//                         16-byte loads where the rows allow it (W_l % 4 == 0 and a 16-byte aligned base), a scalar path otherwise.
//   inpaint_apex_kernel   one workgroup per image: level la into LDS (formed from the inputs when la = 0), the remaining pulls, the apex and every
//                         push down to level la; (P, G) of level la goes back over its (cg, wg) in the workspace, or, when la = 0, `out` is written.
//   inpaint_push_kernel   one workgroup per 64 x 64 tile of level l and image: (P, G) of level l + n (n <= 4) with a one-cell halo into LDS, the levels
//                         between from their stored triples (halo cells are recomputed per tile: the tent filter of a halo cell reaches one
//                         coarse cell outwards), then level l: `out` from the re-formed level 0, or (P, G) over (cg, wg) of a stored level.
// No atomics and no reduction across threads: every sum has the order written above, so two calls give the same bits and image i of a batch
// equals its one-image call.  Nothing is allocated here: the caller brings the workspace.
#include <math.h>
#include "common.h"

#define IP_TS 64              // tile edge at the finest level of a pull / push launch
#define IP_THREADS 256
#define IP_MAXLEV 4           // levels per pull / push launch
#define IP_APEX_FLOATS 40000  // pyramid floats the apex workgroup holds (160,000 B of the 163,840 B a workgroup may declare)
#define IP_APEX_THREADS 1024
#define IP_MAXL 32            // a plane of at most 2^30 pixels has at most 30 pulls

struct IpIn {
    const float* values;       // [I][C][H][W]
    const float* weight;       // [I][1][H][W]
    const float* guide;        // [I][1][H][W]; not read when beta == 0
    const float* guide_scale;  // [I]
    float beta, floor;
};
struct IpDst {
    float* p[IP_MAXLEV];  // the blocks of levels l + 1 .. l + n
};
struct IpLev {
    const float* blk[IP_MAXLEV];             // blocks of levels l + 1 .. l + n: stored triples for k < n, (P, G) in channels 0..C for k = n
    int H[IP_MAXLEV + 1], W[IP_MAXLEV + 1];  // sizes of levels l .. l + n
};

__device__ __forceinline__ float ip_div(float n, float d) { return d > 0.f ? n / d : 0.f; }

// four floats of row y from column x (a multiple of 4) of an H x W plane; 0 beyond the plane
__device__ __forceinline__ void ip_ld4(const float* __restrict__ plane, int y, int x, int H, int W, bool vec, float (&r)[4]) {
    r[0] = r[1] = r[2] = r[3] = 0.f;
    if (y >= H || x >= W) return;
    const float* p = plane + (size_t)y * W + x;
    if (vec) {  // W % 4 == 0: x < W implies x + 3 < W
        const float4 v = *reinterpret_cast<const float4*>(p);
        r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
    } else {
        r[0] = p[0];
        if (x + 1 < W) r[1] = p[1];
        if (x + 2 < W) r[2] = p[2];
        if (x + 3 < W) r[3] = p[3];
    }
}

// the factor g of one pixel (kept pixels only; guide is read by the caller only when beta > 0)
__device__ __forceinline__ float ip_g(float guide, float gs, float beta) { return expf(-beta * (guide / gs)); }

// the two coarse taps of fine index i in a coarse level of n cells
__device__ __forceinline__ void ip_tent(int i, int n, int& t0, int& t1, float& w0, float& w1) {
    const int h = i >> 1;
    if (i & 1) {
        t0 = h, t1 = h + 1, w0 = 0.75f, w1 = 0.25f;
    } else {
        t0 = h - 1, t1 = h, w0 = 0.25f, w1 = 0.75f;
    }
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > n - 1 ? n - 1 : t1;
}

__device__ __forceinline__ float ip_up(const float* __restrict__ x, int i00, int i01, int i10, int i11, float wx0, float wx1, float wy0, float wy1) {
    return wy0 * (wx0 * x[i00] + wx1 * x[i01]) + wy1 * (wx0 * x[i10] + wx1 * x[i11]);
}

// (P, G) of a cell of a level >= 1 from its stored triple and the upsampled coarse level
template <int C>
__device__ __forceinline__ void ip_blend(const float (&cg)[C], float wg, float a, const float (&up)[C], float ug, float (&P)[C], float& G) {
    G = a * ip_div(wg, a) + (1.f - a) * ug;
#pragma unroll
    for (int c = 0; c < C; ++c) P[c] = (a * ip_div(cg[c], wg) + (1.f - a) * ip_div(up[c], ug)) * G;
}

// all C + 2 channels of a coarse cell times 1 / a_sum where a_sum > 1
template <int CH>
__device__ __forceinline__ void ip_saturate(float (&acc)[CH]) {
    if (acc[CH - 1] > 1.f) {
        const float r = 1.f / acc[CH - 1];
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) acc[ch] *= r;
    }
}

// one pull inside LDS: the SC x SC coarse cells of a tile from its 2SC x 2SC fine cells (cells beyond the level hold zeros), also stored to the level's block
template <int CH>
__device__ __forceinline__ void ip_pull_lds(const float* sf, float* sc, int SC, float* __restrict__ g, size_t img, int cy0, int cx0, int Hc, int Wc) {
    const int SF = 2 * SC;
    const size_t nc = (size_t)Hc * Wc;
    for (int t = threadIdx.x; t < SC * SC; t += IP_THREADS) {
        const int r = t / SC, c = t % SC;
        float acc[CH];
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            const float* f = sf + ch * SF * SF + 2 * r * SF + 2 * c;
            acc[ch] = (f[0] + f[1]) + (f[SF] + f[SF + 1]);
        }
        ip_saturate<CH>(acc);
        const bool inside = cy0 + r < Hc && cx0 + c < Wc;
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            sc[ch * SC * SC + t] = acc[ch];
            if (inside) g[(img * CH + ch) * nc + (size_t)(cy0 + r) * Wc + cx0 + c] = acc[ch];
        }
    }
}

template <int C, bool FROM_INPUT>
__global__ __launch_bounds__(IP_THREADS) void inpaint_pull_kernel(const IpIn in, const float* __restrict__ src, const IpDst dst, int Hl, int Wl, int nlev,
                                                                  int tiles_x, int tiles, int vec) {
    constexpr int CH = C + 2;
    __shared__ float s1[CH * 32 * 32], s2[CH * 16 * 16], s3[CH * 8 * 8], s4[CH * 4 * 4];
    const size_t img = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, ty = tile / tiles_x, tx = tile % tiles_x;
    const size_t nl = (size_t)Hl * Wl;
    int Hc = (Hl + 1) >> 1, Wc = (Wl + 1) >> 1;
    const bool use_guide = in.beta > 0.f;
    float gs = 1.f;
    if (FROM_INPUT && use_guide) gs = in.guide_scale[img];
    {
        const size_t nc = (size_t)Hc * Wc;
        for (int it = 0; it < 2; ++it) {  // a thread: two adjacent coarse cells = 2 rows x 4 fine cells
            const int p = threadIdx.x + it * IP_THREADS, row = p >> 4, pc = p & 15;
            const int cy = ty * 32 + row, cx = tx * 32 + 2 * pc, fy = 2 * cy, fx = 2 * cx;
            float acc[2][CH];
            if (FROM_INPUT) {
                float g[2][4], w0[2][4];
                bool keep[2][4];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    float w[4], gd[4] = {0.f, 0.f, 0.f, 0.f};
                    ip_ld4(in.weight + img * nl, fy + r, fx, Hl, Wl, vec, w);
                    if (use_guide) ip_ld4(in.guide + img * nl, fy + r, fx, Hl, Wl, vec, gd);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        keep[r][j] = w[j] >= in.floor;
                        w0[r][j] = keep[r][j] ? w[j] : 0.f;
                        g[r][j] = keep[r][j] && use_guide ? ip_g(gd[j], gs, in.beta) : 1.f;
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[j][C] = (w0[0][2 * j] * g[0][2 * j] + w0[0][2 * j + 1] * g[0][2 * j + 1]) + (w0[1][2 * j] * g[1][2 * j] + w0[1][2 * j + 1] * g[1][2 * j + 1]);
                    acc[j][C + 1] = (w0[0][2 * j] + w0[0][2 * j + 1]) + (w0[1][2 * j] + w0[1][2 * j + 1]);
                }
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float cg[2][4];
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        float v[4];
                        ip_ld4(in.values + (img * C + c) * nl, fy + r, fx, Hl, Wl, vec, v);
#pragma unroll
                        for (int j = 0; j < 4; ++j) cg[r][j] = keep[r][j] ? v[j] * g[r][j] : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[j][c] = (cg[0][2 * j] + cg[0][2 * j + 1]) + (cg[1][2 * j] + cg[1][2 * j + 1]);
                }
            } else {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    float f[2][4];
                    ip_ld4(src + (img * CH + ch) * nl, fy, fx, Hl, Wl, vec, f[0]);
                    ip_ld4(src + (img * CH + ch) * nl, fy + 1, fx, Hl, Wl, vec, f[1]);
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[j][ch] = (f[0][2 * j] + f[0][2 * j + 1]) + (f[1][2 * j] + f[1][2 * j + 1]);
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                ip_saturate<CH>(acc[j]);
                const bool inside = cy < Hc && cx + j < Wc;
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    s1[ch * 1024 + row * 32 + 2 * pc + j] = acc[j][ch];
                    if (inside) dst.p[0][(img * CH + ch) * nc + (size_t)cy * Wc + cx + j] = acc[j][ch];
                }
            }
        }
    }
    if (nlev < 2) return;
    __syncthreads();
    Hc = (Hc + 1) >> 1, Wc = (Wc + 1) >> 1;
    ip_pull_lds<CH>(s1, s2, 16, dst.p[1], img, ty * 16, tx * 16, Hc, Wc);
    if (nlev < 3) return;
    __syncthreads();
    Hc = (Hc + 1) >> 1, Wc = (Wc + 1) >> 1;
    ip_pull_lds<CH>(s2, s3, 8, dst.p[2], img, ty * 8, tx * 8, Hc, Wc);
    if (nlev < 4) return;
    __syncthreads();
    Hc = (Hc + 1) >> 1, Wc = (Wc + 1) >> 1;
    ip_pull_lds<CH>(s3, s4, 4, dst.p[3], img, ty * 4, tx * 4, Hc, Wc);
}

// ---------------------------------------------------------------------------------------- apex: one workgroup per image
template <int C, bool FROM_INPUT>
__global__ __launch_bounds__(IP_APEX_THREADS) void inpaint_apex_kernel(const IpIn in, float* __restrict__ lev, float* __restrict__ out, int Hs, int Ws, int nlv) {
    constexpr int CH = C + 2;
    __shared__ float s[IP_APEX_FLOATS];
    __shared__ int lh[IP_MAXL], lw[IP_MAXL], lo[IP_MAXL];
    const size_t img = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int h = Hs, w = Ws, o = 0;
        for (int k = 0; k <= nlv; ++k) {
            lh[k] = h, lw[k] = w, lo[k] = o;
            o += CH * h * w;
            h = (h + 1) >> 1, w = (w + 1) >> 1;
        }
    }
    __syncthreads();
    const int n0 = Hs * Ws;
    if (FROM_INPUT) {
        const bool use_guide = in.beta > 0.f;
        const float gs = use_guide ? in.guide_scale[img] : 1.f;
        for (int i = tid; i < n0; i += IP_APEX_THREADS) {
            const float w = in.weight[img * n0 + i];
            const bool keep = w >= in.floor;
            const float w0 = keep ? w : 0.f;
            const float g = keep && use_guide ? ip_g(in.guide[img * n0 + i], gs, in.beta) : 1.f;
#pragma unroll
            for (int c = 0; c < C; ++c) s[c * n0 + i] = keep ? in.values[(img * C + c) * n0 + i] * g : 0.f;
            s[C * n0 + i] = w0 * g;
            s[(C + 1) * n0 + i] = w0;
        }
    } else {
        for (int i = tid; i < CH * n0; i += IP_APEX_THREADS) s[i] = lev[img * CH * n0 + i];
    }
    __syncthreads();
    for (int k = 0; k < nlv; ++k) {  // the remaining pulls
        const int Hf = lh[k], Wf = lw[k], nf = Hf * Wf, Wc = lw[k + 1], nc = lh[k + 1] * Wc;
        const float* fine = s + lo[k];
        float* coarse = s + lo[k + 1];
        for (int i = tid; i < nc; i += IP_APEX_THREADS) {
            const int y = i / Wc, x = i % Wc, b = 2 * y * Wf + 2 * x;
            const bool hx = 2 * x + 1 < Wf, hy = 2 * y + 1 < Hf;
            float acc[CH];
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const float* f = fine + ch * nf + b;
                acc[ch] = (f[0] + (hx ? f[1] : 0.f)) + ((hy ? f[Wf] : 0.f) + (hx && hy ? f[Wf + 1] : 0.f));
            }
            ip_saturate<CH>(acc);
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) coarse[ch * nc + i] = acc[ch];
        }
        __syncthreads();
    }
    if (FROM_INPUT && nlv == 0) {  // L = 0, the 1 x 1 image: out = c0 + (1 - w0) F_0
        if (tid == 0) {
            const float wg = s[C], w0 = s[C + 1];
#pragma unroll
            for (int c = 0; c < C; ++c) out[img * C + c] = (w0 > 0.f ? in.values[img * C + c] : 0.f) + (1.f - w0) * ip_div(s[c], wg);
        }
        return;
    }
    if (tid == 0) {  // the apex, 1 x 1
        float* p = s + lo[nlv];
        const float wg = p[C], G = ip_div(wg, p[C + 1]);
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = ip_div(p[c], wg) * G;
        p[C] = G;
    }
    __syncthreads();
    for (int k = nlv - 1; k >= 0; --k) {  // the pushes, in place: (cg, wg) of a level becomes its (P, G)
        const int Hf = lh[k], Wf = lw[k], nf = Hf * Wf, Hc = lh[k + 1], Wc = lw[k + 1], nc = Hc * Wc;
        float* fine = s + lo[k];
        const float* coarse = s + lo[k + 1];
        for (int i = tid; i < nf; i += IP_APEX_THREADS) {
            const int y = i / Wf, x = i % Wf;
            int y0, y1, x0, x1;
            float wy0, wy1, wx0, wx1;
            ip_tent(y, Hc, y0, y1, wy0, wy1);
            ip_tent(x, Wc, x0, x1, wx0, wx1);
            const int i00 = y0 * Wc + x0, i01 = y0 * Wc + x1, i10 = y1 * Wc + x0, i11 = y1 * Wc + x1;
            const float ug = ip_up(coarse + C * nc, i00, i01, i10, i11, wx0, wx1, wy0, wy1);
            float up[C];
#pragma unroll
            for (int c = 0; c < C; ++c) up[c] = ip_up(coarse + c * nc, i00, i01, i10, i11, wx0, wx1, wy0, wy1);
            const float a = fine[(C + 1) * nf + i];
            if (FROM_INPUT && k == 0) {  // a = w0 here, and a kept pixel has w0 > 0
#pragma unroll
                for (int c = 0; c < C; ++c) out[(img * C + c) * n0 + i] = (a > 0.f ? in.values[(img * C + c) * n0 + i] : 0.f) + (1.f - a) * ip_div(up[c], ug);
            } else {
                float cg[C], P[C], G;
#pragma unroll
                for (int c = 0; c < C; ++c) cg[c] = fine[c * nf + i];
                ip_blend<C>(cg, fine[C * nf + i], a, up, ug, P, G);
#pragma unroll
                for (int c = 0; c < C; ++c) fine[c * nf + i] = P[c];
                fine[C * nf + i] = G;
            }
        }
        __syncthreads();
    }
    if (!FROM_INPUT)
        for (int i = tid; i < (C + 1) * n0; i += IP_APEX_THREADS) lev[img * CH * n0 + i] = s[i];
}

// ---------------------------------------------------------------------------------------- push: 64 x 64 tiles of level l from (P, G) of level l + n
#define IP_RS(k) ((IP_TS >> (k)) + 2)  // region edge at level l + k: the tile's cells and a one-cell halo

template <int C, bool TO_OUT>
__global__ __launch_bounds__(IP_THREADS) void inpaint_push_kernel(const IpIn in, float* __restrict__ lev, float* __restrict__ out, const IpLev lv, int nlev,
                                                                  int tiles_x, int tiles, int vec) {
    constexpr int CH = C + 2, CP = C + 1;
    __shared__ float sr[CP * (IP_RS(1) * IP_RS(1) + IP_RS(2) * IP_RS(2) + IP_RS(3) * IP_RS(3) + IP_RS(4) * IP_RS(4))];
    const size_t img = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, ty = tile / tiles_x, tx = tile % tiles_x;
    int roff[IP_MAXLEV + 1];
    roff[1] = 0;
#pragma unroll
    for (int k = 1; k < IP_MAXLEV; ++k) roff[k + 1] = roff[k] + CP * IP_RS(k) * IP_RS(k);
    {  // (P, G) of level l + n
        const int S = IP_RS(nlev), oy = ((ty * IP_TS) >> nlev) - 1, ox = ((tx * IP_TS) >> nlev) - 1, Hn = lv.H[nlev], Wn = lv.W[nlev];
        const size_t nn = (size_t)Hn * Wn;
        float* r = sr + roff[nlev];
        for (int t = threadIdx.x; t < S * S; t += IP_THREADS) {
            const int y = oy + t / S, x = ox + t % S;
            const bool inside = y >= 0 && y < Hn && x >= 0 && x < Wn;
#pragma unroll
            for (int ch = 0; ch < CP; ++ch) r[ch * S * S + t] = inside ? lv.blk[nlev - 1][(img * CH + ch) * nn + (size_t)y * Wn + x] : 0.f;
        }
    }
    __syncthreads();
    for (int k = nlev - 1; k >= 1; --k) {  // the levels between, from their stored triples
        const int S = IP_RS(k), oy = ((ty * IP_TS) >> k) - 1, ox = ((tx * IP_TS) >> k) - 1, Hk = lv.H[k], Wk = lv.W[k];
        const int SC = IP_RS(k + 1), oyc = ((ty * IP_TS) >> (k + 1)) - 1, oxc = ((tx * IP_TS) >> (k + 1)) - 1, Hc = lv.H[k + 1], Wc = lv.W[k + 1];
        const size_t nk = (size_t)Hk * Wk;
        float* r = sr + roff[k];
        const float* rc = sr + roff[k + 1];
        const float* blk = lv.blk[k - 1] + img * CH * nk;
        for (int t = threadIdx.x; t < S * S; t += IP_THREADS) {
            const int y = oy + t / S, x = ox + t % S;
            float P[C], G = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) P[c] = 0.f;
            if (y >= 0 && y < Hk && x >= 0 && x < Wk) {
                int y0, y1, x0, x1;
                float wy0, wy1, wx0, wx1;
                ip_tent(y, Hc, y0, y1, wy0, wy1);
                ip_tent(x, Wc, x0, x1, wx0, wx1);
                y0 = min(max(y0 - oyc, 0), SC - 1), y1 = min(max(y1 - oyc, 0), SC - 1), x0 = min(max(x0 - oxc, 0), SC - 1), x1 = min(max(x1 - oxc, 0), SC - 1);
                const int i00 = y0 * SC + x0, i01 = y0 * SC + x1, i10 = y1 * SC + x0, i11 = y1 * SC + x1;
                const float ug = ip_up(rc + C * SC * SC, i00, i01, i10, i11, wx0, wx1, wy0, wy1);
                float up[C], cg[C];
                const size_t at = (size_t)y * Wk + x;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    up[c] = ip_up(rc + c * SC * SC, i00, i01, i10, i11, wx0, wx1, wy0, wy1);
                    cg[c] = blk[c * nk + at];
                }
                ip_blend<C>(cg, blk[C * nk + at], blk[(C + 1) * nk + at], up, ug, P, G);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) r[c * S * S + t] = P[c];
            r[C * S * S + t] = G;
        }
        __syncthreads();
    }
    // level l: a thread takes four adjacent cells of a row
    const int H0 = lv.H[0], W0 = lv.W[0], Hc = lv.H[1], Wc = lv.W[1], SC = IP_RS(1), oyc = ((ty * IP_TS) >> 1) - 1, oxc = ((tx * IP_TS) >> 1) - 1;
    const size_t n0 = (size_t)H0 * W0;
    const float* rc = sr;
    for (int it = 0; it < 4; ++it) {
        const int q = threadIdx.x + it * IP_THREADS, y = ty * IP_TS + (q >> 4), xq = tx * IP_TS + 4 * (q & 15);
        if (y >= H0 || xq >= W0) continue;
        int y0, y1;
        float wy0, wy1;
        ip_tent(y, Hc, y0, y1, wy0, wy1);
        y0 = min(max(y0 - oyc, 0), SC - 1), y1 = min(max(y1 - oyc, 0), SC - 1);
        float ug[4], up[C][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int x0, x1;
            float wx0, wx1;
            ip_tent(min(xq + j, W0 - 1), Wc, x0, x1, wx0, wx1);
            x0 = min(max(x0 - oxc, 0), SC - 1), x1 = min(max(x1 - oxc, 0), SC - 1);
            const int i00 = y0 * SC + x0, i01 = y0 * SC + x1, i10 = y1 * SC + x0, i11 = y1 * SC + x1;
            ug[j] = ip_up(rc + C * SC * SC, i00, i01, i10, i11, wx0, wx1, wy0, wy1);
#pragma unroll
            for (int c = 0; c < C; ++c) up[c][j] = ip_up(rc + c * SC * SC, i00, i01, i10, i11, wx0, wx1, wy0, wy1);
        }
        const size_t at = (size_t)y * W0 + xq;
        if (TO_OUT) {
            float w[4];
            ip_ld4(in.weight + img * n0, y, xq, H0, W0, vec, w);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float v[4], o[4];
                ip_ld4(in.values + (img * C + c) * n0, y, xq, H0, W0, vec, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool keep = w[j] >= in.floor;
                    o[j] = (keep ? v[j] : 0.f) + (1.f - (keep ? w[j] : 0.f)) * ip_div(up[c][j], ug[j]);
                }
                float* po = out + (img * C + c) * n0 + at;
                if (vec) {
                    *reinterpret_cast<float4*>(po) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (xq + j < W0) po[j] = o[j];
                }
            }
        } else {
            float* blk = lev + img * CH * n0;
            float cg[C][4], wg[4], a[4];
#pragma unroll
            for (int c = 0; c < C; ++c) ip_ld4(blk + c * n0, y, xq, H0, W0, vec, cg[c]);
            ip_ld4(blk + C * n0, y, xq, H0, W0, vec, wg);
            ip_ld4(blk + (C + 1) * n0, y, xq, H0, W0, vec, a);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (xq + j >= W0) continue;
                float cgj[C], upj[C], P[C], G;
#pragma unroll
                for (int c = 0; c < C; ++c) cgj[c] = cg[c][j], upj[c] = up[c][j];
                ip_blend<C>(cgj, wg[j], a[j], upj, ug[j], P, G);
#pragma unroll
                for (int c = 0; c < C; ++c) blk[c * n0 + at + j] = P[c];
                blk[C * n0 + at + j] = G;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- C-ABI
static int ip_dims(int H, int W, int* hs, int* ws) {
    int L = 0;
    hs[0] = H, ws[0] = W;
    while (hs[L] > 1 || ws[L] > 1) {
        hs[L + 1] = (hs[L] + 1) >> 1, ws[L + 1] = (ws[L] + 1) >> 1;
        ++L;
    }
    return L;
}

static bool ip_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W <= (1ll << 30); }

extern "C" int falnet_inpaint_levels(int H, int W) {
    if (!ip_shape_ok(H, W)) return -1;
    int hs[IP_MAXL], ws[IP_MAXL];
    return ip_dims(H, W, hs, ws);
}

extern "C" int64_t falnet_inpaint_workspace_bytes(int C, int H, int W, int images) {
    if (!ip_shape_ok(H, W) || C < 1 || C > 4 || images < 1) return -1;
    int hs[IP_MAXL], ws[IP_MAXL];
    const int L = ip_dims(H, W, hs, ws);
    int64_t cells = 0;
    for (int l = 1; l <= L; ++l) cells += (int64_t)hs[l] * ws[l];
    return cells * (C + 2) * images * 4;
}

template <int C>
static void ip_launch(const IpIn& in, float* out, float* wsp, int I, int H, int W, hipStream_t st) {
    constexpr int CH = C + 2;
    int hs[IP_MAXL], ws[IP_MAXL];
    const int L = ip_dims(H, W, hs, ws);
    float* blk[IP_MAXL];  // the block of level l >= 1
    int64_t cells = 0;
    blk[0] = nullptr;
    for (int l = 1; l <= L; ++l) {
        blk[l] = wsp + cells * CH * I;
        cells += (int64_t)hs[l] * ws[l];
    }
    int la = L;  // the first level whose remaining pyramid fits the apex workgroup
    for (int64_t rest = CH; la > 0; --la) {
        rest += (int64_t)CH * hs[la - 1] * ws[la - 1];
        if (rest > IP_APEX_FLOATS) break;
    }
    auto aligned = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    const int vec0 = W % 4 == 0 && aligned(in.values) && aligned(in.weight) && aligned(out) && (!(in.beta > 0.f) || aligned(in.guide));
    auto grid_of = [&](int l, int& tiles_x, int& tiles) {
        tiles_x = (ws[l] + IP_TS - 1) / IP_TS;
        tiles = tiles_x * ((hs[l] + IP_TS - 1) / IP_TS);
        return dim3((unsigned)((int64_t)tiles * I));
    };
    if (la == 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(inpaint_apex_kernel<C, true>), dim3(I), dim3(IP_APEX_THREADS), 0, st, in, (float*)nullptr, out, H, W, L);
        return;
    }
    int steps[IP_MAXL], nsteps = 0;  // the levels at which a pull starts (and a push ends)
    for (int l = 0; l < la; l += IP_MAXLEV) steps[nsteps++] = l;
    for (int s = 0; s < nsteps; ++s) {
        const int l = steps[s], n = la - l < IP_MAXLEV ? la - l : IP_MAXLEV;
        IpDst dst;
        for (int k = 0; k < IP_MAXLEV; ++k) dst.p[k] = k < n ? blk[l + 1 + k] : nullptr;
        int tiles_x, tiles;
        const dim3 grid = grid_of(l, tiles_x, tiles);
        if (l == 0)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(inpaint_pull_kernel<C, true>), grid, dim3(IP_THREADS), 0, st, in, (const float*)nullptr, dst, H, W, n, tiles_x, tiles, vec0);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(inpaint_pull_kernel<C, false>), grid, dim3(IP_THREADS), 0, st, in, (const float*)blk[l], dst, hs[l], ws[l], n, tiles_x,
                               tiles, (int)(ws[l] % 4 == 0 && (int64_t)hs[l] * ws[l] % 4 == 0 && aligned(blk[l])));
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(inpaint_apex_kernel<C, false>), dim3(I), dim3(IP_APEX_THREADS), 0, st, in, blk[la], (float*)nullptr, hs[la], ws[la], L - la);
    for (int s = nsteps - 1; s >= 0; --s) {
        const int l = steps[s], n = la - l < IP_MAXLEV ? la - l : IP_MAXLEV;
        IpLev lv;
        for (int k = 0; k <= IP_MAXLEV; ++k) lv.H[k] = k <= n ? hs[l + k] : 1, lv.W[k] = k <= n ? ws[l + k] : 1;
        for (int k = 0; k < IP_MAXLEV; ++k) lv.blk[k] = k < n ? blk[l + 1 + k] : nullptr;
        int tiles_x, tiles;
        const dim3 grid = grid_of(l, tiles_x, tiles);
        if (l == 0)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(inpaint_push_kernel<C, true>), grid, dim3(IP_THREADS), 0, st, in, (float*)nullptr, out, lv, n, tiles_x, tiles, vec0);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(inpaint_push_kernel<C, false>), grid, dim3(IP_THREADS), 0, st, in, blk[l], (float*)nullptr, lv, n, tiles_x, tiles,
                               (int)(ws[l] % 4 == 0 && (int64_t)hs[l] * ws[l] % 4 == 0 && aligned(blk[l])));
    }
}

extern "C" int falnet_inpaint_fwd(const float* values, const float* weight, const float* guide, const float* guide_scale, float beta, float floor, float* out,
                                  void* workspace, int64_t workspace_bytes, int I, int C, int H, int W, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(I >= 1 && H >= 1 && W >= 1, "inpaint_fwd: empty shape I=%d H=%d W=%d", I, H, W);
    FALNET_CHECK_ARG(C >= 1 && C <= 4, "inpaint_fwd: C=%d outside [1,4]", C);
    FALNET_CHECK_ARG((int64_t)H * W <= (1ll << 30), "inpaint_fwd: H=%d W=%d: a plane of more than 2^30 pixels", H, W);
    FALNET_CHECK_ARG(isfinite(beta) && beta >= 0.f && beta <= 8.f, "inpaint_fwd: beta=%g outside [0,8]", (double)beta);
    FALNET_CHECK_ARG(floor > 0.f && floor <= 1.f, "inpaint_fwd: floor=%g outside (0,1]", (double)floor);
    FALNET_CHECK_ARG(values && weight && out, "inpaint_fwd: null values, weight or out");
    FALNET_CHECK_ARG(beta == 0.f || (guide && guide_scale), "inpaint_fwd: beta=%g > 0 needs guide and guide_scale", (double)beta);
    const int64_t elems = (int64_t)I * C * H * W;
    FALNET_CHECK_ARG(out + elems <= values || values + elems <= out, "inpaint_fwd: out overlaps values");
    const int64_t need = falnet_inpaint_workspace_bytes(C, H, W, I);
    FALNET_CHECK_ARG(workspace_bytes >= need && (workspace || need == 0), "inpaint_fwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    FALNET_CHECK_ARG(need == 0 || (((uintptr_t)workspace) & 3) == 0, "inpaint_fwd: workspace must be 4-byte aligned");
    FALNET_CHECK_ARG((int64_t)((W + IP_TS - 1) / IP_TS) * ((H + IP_TS - 1) / IP_TS) * I < (1ll << 31), "inpaint_fwd: I=%d H=%d W=%d: too many tiles for one launch", I, H, W);
    const IpIn in = {values, weight, beta > 0.f ? guide : nullptr, beta > 0.f ? guide_scale : nullptr, beta, floor};
    float* wsp = (float*)workspace;
    const hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: ip_launch<1>(in, out, wsp, I, H, W, st); break;
        case 2: ip_launch<2>(in, out, wsp, I, H, W, st); break;
        case 3: ip_launch<3>(in, out, wsp, I, H, W, st); break;
        default: ip_launch<4>(in, out, wsp, I, H, W, st); break;
    }
    FALNET_RETURN_LAUNCH();
}
