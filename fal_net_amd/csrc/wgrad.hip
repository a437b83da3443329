// Weight gradients of the convolutions (conv.hip) on the gfx950 matrix cores: the per-tap, halo-patch, stride-2 and first-layer kernels,
// the reduction of their split slabs into the OIHW f32 gradient, the bias gradients, and the falnet_wgrad dispatcher (which also launches
// the row- / wave-streaming forms of wgrad_rows.hip and wgrad_wave.hip).  Not one of the autotuned sources (ops.py: _TUNE_SOURCES):
// a change here leaves every cached convolution choice valid.
#include <stdlib.h>
#include "common.h"
#include "conv_epilogue.h"  // f32x16
#include "wgrad_dispatch.h"

#define CONV_THREADS 256  // threads of wgrad_kernel's workgroup

// ------------------------------------------------------------------------------------------ wgrad
// dW[co, tap, ci] = sum_p G[p, co] * In[nbr(p, tap), ci]: both operands are pixel-major (the contraction
// index is the slow one), so the LDS tiles are [pixel][channel] and the MFMA operands are read transposed:
//   bf16: ds_read_b64_tr_b16 (two per 8-element fragment);  f32: one ds_read_b32 per lane (A[m][k]: m on lanes).
// Workgroup = 64 couts x 64 cins for one (tap, pixel split); 4 waves 2x2, 32x32 each; 64 pixels per K step.
#define WG_BM 64
#define WG_BN 64
#define WG_KP 64

typedef short s16x4 __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(CONV_THREADS) void wgrad_kernel(const falnet_wgrad_t p, int w_rows) {
    constexpr int EPS = 16 / sizeof(T);
    constexpr int ROW_ELEMS = 64;                          // channels per tile row
    constexpr int SEGS = ROW_ELEMS / EPS;                  // 16-B segments per row (8 bf16 / 16 f32)
    constexpr int PITCH = ROW_ELEMS * sizeof(T) + 16;      // bytes
    constexpr int LOADS = WG_KP * SEGS / CONV_THREADS;     // per operand per thread (2 bf16 / 4 f32)
    __shared__ __attribute__((aligned(16))) char lds[2 * 2 * WG_KP * PITCH];
    auto Gbuf = [&](int b) -> char* { return lds + b * 2 * WG_KP * PITCH; };
    auto Ibuf = [&](int b) -> char* { return lds + b * 2 * WG_KP * PITCH + WG_KP * PITCH; };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ci0 = blockIdx.x * WG_BN;   // packed input-channel offset (over all sources)
    const int co0 = blockIdx.y * WG_BM;
    const int tap = blockIdx.z % p.ntaps, split = blockIdx.z / p.ntaps;
    const int dy = p.tap_dy[tap], dx = p.tap_dx[tap];
    const int c_first = p.src[0].C;  // packed channels [0, c_first) come from source 0, the rest from source 1

    const int64_t M = (int64_t)p.B * p.TH * p.TW;
    const int64_t per = ((M + p.nsplit - 1) / p.nsplit + WG_KP - 1) / WG_KP * WG_KP;
    const int64_t pbeg = (int64_t)split * per, pend = pbeg + per < M ? pbeg + per : M;
    const int niter = pbeg < pend ? (int)((pend - pbeg + WG_KP - 1) / WG_KP) : 0;

    uint4 greg[LOADS], ireg[LOADS];
    int64_t pcur = pbeg;
    auto gload = [&]() {
#pragma unroll
        for (int i = 0; i < LOADS; ++i) {
            const int idx = tid + i * CONV_THREADS;
            const int row = idx / SEGS, seg = idx % SEGS;
            const int64_t m = pcur + row;
            uint4 g = make_uint4(0, 0, 0, 0), v = make_uint4(0, 0, 0, 0);
            if (m < pend) {
                if (co0 + seg * EPS < p.gC)
                    g = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.gout) + m * p.gC + co0 + seg * EPS);
                const int tx = (int)(m % p.TW), ty = (int)((m / p.TW) % p.TH), b = (int)(m / ((int64_t)p.TW * p.TH));
                int vy = ty * p.isy + dy, vx = tx * p.isx + dx;
                const int cpk = ci0 + seg * EPS;  // packed channel of this 16-B segment
                const falnet_src_t& S = p.src[cpk < c_first ? 0 : 1];
                const int cloc = cpk < c_first ? cpk : cpk - c_first;
                if (vy >= 0 && vy < p.IH && vx >= 0 && vx < p.IW && cpk < p.cin_total) {
                    if ((S.H != p.IH) || (S.W != p.IW)) {
                        vy = (2 * S.H == p.IH) ? (vy >> 1) : (int)(((int64_t)vy * S.H) / p.IH);
                        vx = (2 * S.W == p.IW) ? (vx >> 1) : (int)(((int64_t)vx * S.W) / p.IW);
                    }
                    v = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(S.ptr) + (int64_t)b * S.sb +
                                                        (int64_t)vy * S.sy + (int64_t)vx * S.sx + cloc);
                }
            }
            greg[i] = g;
            ireg[i] = v;
        }
        pcur += WG_KP;
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LOADS; ++i) {
            const int idx = tid + i * CONV_THREADS;
            const int row = idx / SEGS, seg = idx % SEGS;
            *reinterpret_cast<uint4*>(Gbuf(buf) + row * PITCH + seg * 16) = greg[i];
            *reinterpret_cast<uint4*>(Ibuf(buf) + row * PITCH + seg * 16) = ireg[i];
        }
    };

    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;

    if (niter > 0) {
        gload();
        lstore(0);
    }
    __syncthreads();
    for (int it = 0; it < niter; ++it) {
        const int cur = it & 1;
        if (it + 1 < niter) gload();
        const char* G = Gbuf(cur);
        const char* I = Ibuf(cur);
        if constexpr (sizeof(T) == 2) {
            // lane group g16 = lane>>4: k-half = g16>>1, 16-channel block = g16&1; lane i=lane&15 supplies row q=i>>2, cols 4*(i&3)
            const int i16 = lane & 15, g16 = lane >> 4;
            const int kh = g16 >> 1, cb = g16 & 1, q = i16 >> 2, pc = i16 & 3;
#pragma unroll
            for (int ks = 0; ks < WG_KP / 16; ++ks) {
                const int krow = ks * 16 + kh * 8 + q;
                const int acol = (wm * 32 + cb * 16 + pc * 4) * 2, bcol = (wn * 32 + cb * 16 + pc * 4) * 2;
                typedef s16x4 __attribute__((address_space(3))) * lds_v4;
                s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(G + krow * PITCH + acol));
                s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(G + (krow + 4) * PITCH + acol));
                s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(I + krow * PITCH + bcol));
                s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(I + (krow + 4) * PITCH + bcol));
                typedef short s16x8 __attribute__((ext_vector_type(8)));
                s16x8 av = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
                s16x8 bv = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
                acc = H16<T>::mma(__builtin_bit_cast(s16x8_t, av), __builtin_bit_cast(s16x8_t, bv), acc);
            }
        } else {
            const int r = lane & 31, h = lane >> 5;
#pragma unroll
            for (int ks = 0; ks < WG_KP / 2; ++ks) {
                const float a = *reinterpret_cast<const float*>(G + (ks * 2 + h) * PITCH + (wm * 32 + r) * 4);
                const float b = *reinterpret_cast<const float*>(I + (ks * 2 + h) * PITCH + (wn * 32 + r) * 4);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
        if (it + 1 < niter) lstore(cur ^ 1);
        __syncthreads();
    }
    // partial[split][tap][co][ci]
    const int r = lane & 31, h = lane >> 5;
    const int ci = ci0 + wn * 32 + r;
    if (ci < p.cin_total) {
        float* dst = p.partial + (((int64_t)split * p.ntaps + tap) * w_rows) * p.cin_total;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int co = co0 + wm * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
            if (co < w_rows) dst[(int64_t)co * p.cin_total + ci] = acc[j];
        }
    }
}

// ------------------------------------------------------------------------------------------ wgrad, halo-patch form
// Dense 3x3 stride-1 layers (the bulk of the weight-gradient FLOPs): a workgroup owns a 32x32 (cout x cin)
// channel block for ALL nine taps and walks a range of 4x32-position patches.  Per patch the gout rows
// [128 px][32 cout] and the input halo [6x34 px][32 cin] are staged ONCE in LDS (the per-tap kernel re-read both
// nine times); wave w contracts image row w of the patch (K = 32 positions) into its nine 32x32 accumulators,
// operands read transposed (bf16: ds_read_b64_tr_b16) as in wgrad_kernel.  The four waves' accumulators are
// summed through LDS at the end and the workgroup writes ONE f32 slab [9][32][32] into
// partial[split][tap][co][ci].  Next patch is prefetched into registers behind the MFMAs.
#define WP_TH 4
#define WP_TW 32
#define WP_PW (WP_TW + 2)
#define WP_NPIX ((WP_TH + 2) * WP_PW)

#define WP_THREADS 192  // three waves: wave w owns the tap row dy = w-1 (taps 3w..3w+2)

// Bias gradient from the gout tile a weight-gradient workgroup has in LDS ([plane][pixel][32 channels], zero-filled outside the
// image): every thread owns one 16-B channel segment and strides over the tile's pixels, accumulating in registers across
// all patches of the workgroup; bias_grad_flush sums the pixel groups through LDS and issues one atomic per channel.
template <typename T, int COT, int NTHR>
__device__ __forceinline__ void bias_grad_accumulate(const char* G, int tid, float (&bsum)[16 / (int)sizeof(T)]) {
    constexpr int EPS = 16 / (int)sizeof(T), SEGS = 32 / EPS, NSEG = SEGS * COT, PSTEP = NTHR / NSEG;
    static_assert(NTHR % NSEG == 0, "threads map evenly onto channel segments");
    constexpr int NPIXT = WP_TH * WP_TW, G_PLANE = NPIXT * 32 * (int)sizeof(T);
    const int sg = tid % NSEG, pg = tid / NSEG;
    const char* base = G + (sg / SEGS) * G_PLANE + (sg % SEGS) * 16;
    for (int px = pg; px < NPIXT; px += PSTEP) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + px * 32 * (int)sizeof(T));
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned w = (&v.x)[i];
                bsum[2 * i] += H16<T>::lo(w);
                bsum[2 * i + 1] += H16<T>::hi(w);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) bsum[i] += __uint_as_float((&v.x)[i]);
        }
    }
}
template <typename T, int COT, int NTHR>
__device__ __forceinline__ void bias_grad_flush(float* lds_f /* >= NTHR * EPS floats, all waves past their last LDS use */, int tid,
                                                const float (&bsum)[16 / (int)sizeof(T)], float* db, int co0, int gC) {
    constexpr int EPS = 16 / (int)sizeof(T), SEGS = 32 / EPS, NSEG = SEGS * COT, PSTEP = NTHR / NSEG;
#pragma unroll
    for (int i = 0; i < EPS; ++i) lds_f[tid * EPS + i] = bsum[i];
    __syncthreads();
    if (tid < NSEG * EPS) {
        const int sg = tid / EPS, i = tid % EPS;
        float t = 0.f;
        for (int pg = 0; pg < PSTEP; ++pg) t += lds_f[(pg * NSEG + sg) * EPS + i];
        const int co = co0 + (sg / SEGS) * 32 + (sg % SEGS) * EPS + i;
        if (co < gC) atomicAdd(db + co, t);
    }
}

// CIT x COT = 32-channel tiles per workgroup along cin / cout (1x1, or 2x2 for bf16 layers with >= 64 channels on both
// sides): every wave then owns 3 taps x CIT x COT accumulator tiles, and one A (gout) fragment feeds 3*CIT MFMAs, one B
// (input) fragment COT of them -- half the LDS reads and half the global bytes per MFMA of the 1x1 form, whose ~2.7
// transposed reads per MFMA and 21 KB per 72 MFMAs sit on the LDS / CU load path.  Channel planes are stored separately
// ([plane][pixel][32 channels], 64-B rows) so the transposed-read addressing is the same for every plane.
template <typename T, int CIT, int COT>
__global__ __launch_bounds__(WP_THREADS) void wgrad3x3_patch_kernel(const falnet_wgrad_t p, int w_rows, int tiles_x, int tiles_y,
                                                                    int patches_per_split) {
    constexpr int EPS = 16 / (int)sizeof(T);
    constexpr int ROWB_ = 32 * (int)sizeof(T);      // bytes of 32 channels
    constexpr int SEGS = ROWB_ / 16;                // 4 (bf16) / 8 (f32)
    // no row padding: a ds_read_b64_tr_b16 32-lane half reads 4 rows x 64 B = exactly the 64 banks once
    constexpr int PITCH = ROWB_;
    constexpr int G_PLANE = WP_TH * WP_TW * PITCH, I_PLANE = WP_NPIX * PITCH;
    constexpr int G_BYTES = COT * G_PLANE, I_BYTES = CIT * I_PLANE;
    constexpr int G_LOADS = WP_TH * WP_TW * SEGS * COT, I_LOADS = WP_NPIX * SEGS * CIT;
    constexpr int G_SLOTS = (G_LOADS + WP_THREADS - 1) / WP_THREADS;
    constexpr int I_SLOTS = (I_LOADS + WP_THREADS - 1) / WP_THREADS;
    __shared__ __attribute__((aligned(16))) char lds[2 * (G_BYTES + I_BYTES)];
    auto Gbuf = [&](int b) -> char* { return lds + b * (G_BYTES + I_BYTES); };
    auto Ibuf = [&](int b) -> char* { return lds + b * (G_BYTES + I_BYTES) + G_BYTES; };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ci0 = blockIdx.x * 32 * CIT, co0 = blockIdx.y * 32 * COT, split = blockIdx.z;
    const int c_first = p.src[0].C;
    // per cin tile: source, channel offset inside it, resize flags (workgroup-uniform; a 64-channel block may straddle
    // the two sources of a fused concat)
    const T* t_ptr[CIT];
    int64_t t_sb[CIT], t_sy[CIT], t_sx[CIT];
    int t_H[CIT], t_W[CIT];
    bool t_ok[CIT];
#pragma unroll
    for (int t = 0; t < CIT; ++t) {
        const int c = ci0 + 32 * t;
        const bool second = c >= c_first;
        t_ok[t] = c < p.cin_total;
        t_ptr[t] = reinterpret_cast<const T*>(second ? p.src[1].ptr : p.src[0].ptr) + (second ? c - c_first : c);
        t_sb[t] = second ? p.src[1].sb : p.src[0].sb;
        t_sy[t] = second ? p.src[1].sy : p.src[0].sy;
        t_sx[t] = second ? p.src[1].sx : p.src[0].sx;
        t_H[t] = second ? p.src[1].H : p.src[0].H;
        t_W[t] = second ? p.src[1].W : p.src[0].W;
    }
    const int npatch = p.B * tiles_x * tiles_y;
    const int pbeg = split * patches_per_split, pend = min(pbeg + patches_per_split, npatch);

    // halo slots: (row, col) of the 6x34 patch per slot (division by 34 hoisted out of the patch loop); with CIT = 2 the
    // eight 16-B segments of a pixel are consecutive lanes (one full 128-B line when both tiles share a source)
    short i_row[I_SLOTS], i_col[I_SLOTS];
#pragma unroll
    for (int u = 0; u < I_SLOTS; ++u) {
        const int pix = (tid + u * WP_THREADS) / (SEGS * CIT);
        i_row[u] = (short)(pix / WP_PW);
        i_col[u] = (short)(pix % WP_PW);
    }

    // Interior patches (the vast majority) take a fast path: every slot's element offset relative to the patch origin is
    // loop-invariant (also through an exact 2x nearest upsampling: origins are even), so a load is one 64-bit add -- the
    // general path costs ~25 VALU per load, i.e. ~8 VALU per MFMA of this kernel (PMC), as much issue time as the MFMAs.
    int g_off[G_SLOTS], i_off[I_SLOTS];
    bool fast_ok = true;  // every tile's source is at the launch size or exactly half of it
#pragma unroll
    for (int t = 0; t < CIT; ++t)
        fast_ok = fast_ok && (t_H[t] == p.IH || 2 * t_H[t] == p.IH) && (t_W[t] == p.IW || 2 * t_W[t] == p.IW) &&
                  (int64_t)p.B * t_sb[t] < (1ll << 31);
    fast_ok = fast_ok && (int64_t)p.B * p.TH * p.TW * p.gC < (1ll << 31) && co0 + 32 * COT <= p.gC && ci0 + 32 * CIT <= p.cin_total;
#pragma unroll
    for (int u = 0; u < G_SLOTS; ++u) {
        const int idx = tid + u * WP_THREADS;
        const int seg = idx % (SEGS * COT), pix = idx / (SEGS * COT);
        g_off[u] = ((pix / WP_TW) * p.TW + pix % WP_TW) * p.gC + seg * EPS;
    }
#pragma unroll
    for (int u = 0; u < I_SLOTS; ++u) {
        const int idx = tid + u * WP_THREADS;
        const int seg8 = idx % (SEGS * CIT), seg = seg8 % SEGS;
        const bool t1 = CIT > 1 && seg8 >= SEGS;
        const int hs = (t1 ? t_H[CIT - 1] : t_H[0]) != p.IH ? 1 : 0, ws = (t1 ? t_W[CIT - 1] : t_W[0]) != p.IW ? 1 : 0;
        const int ry = (i_row[u] - 1) >> hs, rx = (i_col[u] - 1) >> ws;  // arithmetic shifts: -1 stays -1
        i_off[u] = (int)(ry * (t1 ? t_sy[CIT - 1] : t_sy[0]) + rx * (t1 ? t_sx[CIT - 1] : t_sx[0])) + seg * EPS;
    }
    struct Regs { uint4 g[G_SLOTS]; uint4 i[I_SLOTS]; };
    auto gload = [&](int patch, Regs& R) {
        int q = patch;
        const int tix = q % tiles_x;
        q /= tiles_x;
        const int tiy = q % tiles_y;
        const int b = q / tiles_y;
        const int y0 = tiy * WP_TH, x0 = tix * WP_TW;
        const T* gbase = reinterpret_cast<const T*>(p.gout) + ((int64_t)b * p.TH * p.TW) * p.gC + co0;
        if (fast_ok && y0 >= 1 && x0 >= 1 && y0 + WP_TH + 1 <= p.IH && x0 + WP_TW + 1 <= p.IW && y0 + WP_TH <= p.TH && x0 + WP_TW <= p.TW) {
            const T* gb = gbase + ((int64_t)y0 * p.TW + x0) * p.gC;
#pragma unroll
            for (int u = 0; u < G_SLOTS; ++u) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (tid + u * WP_THREADS < G_LOADS) v = *reinterpret_cast<const uint4*>(gb + g_off[u]);
                R.g[u] = v;
            }
            const T* ib[CIT];
#pragma unroll
            for (int t = 0; t < CIT; ++t) {
                const int hs = t_H[t] != p.IH ? 1 : 0, ws = t_W[t] != p.IW ? 1 : 0;
                ib[t] = t_ptr[t] + (int64_t)b * t_sb[t] + (int64_t)(y0 >> hs) * t_sy[t] + (int64_t)(x0 >> ws) * t_sx[t];
            }
#pragma unroll
            for (int u = 0; u < I_SLOTS; ++u) {
                const int idx = tid + u * WP_THREADS;
                const bool t1 = CIT > 1 && idx % (SEGS * CIT) >= SEGS;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (idx < I_LOADS) v = *reinterpret_cast<const uint4*>((t1 ? ib[CIT - 1] : ib[0]) + i_off[u]);
                R.i[u] = v;
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < G_SLOTS; ++u) {
            const int idx = tid + u * WP_THREADS;
            const int seg = idx % (SEGS * COT), pix = idx / (SEGS * COT);
            const int y = y0 + pix / WP_TW, x = x0 + pix % WP_TW;  // WP_TW = 32: shifts
            uint4 v = make_uint4(0, 0, 0, 0);
            if (idx < G_LOADS && y < p.TH && x < p.TW && co0 + seg * EPS < p.gC)
                v = *reinterpret_cast<const uint4*>(gbase + ((int64_t)y * p.TW + x) * p.gC + seg * EPS);
            R.g[u] = v;
        }
#pragma unroll
        for (int u = 0; u < I_SLOTS; ++u) {
            const int idx = tid + u * WP_THREADS;
            const int seg8 = idx % (SEGS * CIT), t = seg8 / SEGS, seg = seg8 % SEGS;
            const bool t1 = CIT > 1 && t == 1;
            uint4 v = make_uint4(0, 0, 0, 0);
            int vy = y0 - 1 + i_row[u], vx = x0 - 1 + i_col[u];
            if (idx < I_LOADS && (t1 ? t_ok[CIT - 1] : t_ok[0]) && vy >= 0 && vy < p.IH && vx >= 0 && vx < p.IW) {
                const int sH = t1 ? t_H[CIT - 1] : t_H[0], sW = t1 ? t_W[CIT - 1] : t_W[0];
                if (sH != p.IH) vy = (2 * sH == p.IH) ? (vy >> 1) : (int)(((int64_t)vy * sH) / p.IH);
                if (sW != p.IW) vx = (2 * sW == p.IW) ? (vx >> 1) : (int)(((int64_t)vx * sW) / p.IW);
                const T* ib = t1 ? t_ptr[CIT - 1] : t_ptr[0];
                v = *reinterpret_cast<const uint4*>(ib + (int64_t)b * (t1 ? t_sb[CIT - 1] : t_sb[0]) + (int64_t)vy * (t1 ? t_sy[CIT - 1] : t_sy[0]) +
                                                    (int64_t)vx * (t1 ? t_sx[CIT - 1] : t_sx[0]) + seg * EPS);
            }
            R.i[u] = v;
        }
    };
    auto lstore = [&](int buf, const Regs& R) {
#pragma unroll
        for (int u = 0; u < G_SLOTS; ++u) {
            const int idx = tid + u * WP_THREADS;
            const int seg8 = idx % (SEGS * COT), pix = idx / (SEGS * COT);
            if (idx < G_LOADS) *reinterpret_cast<uint4*>(Gbuf(buf) + (seg8 / SEGS) * G_PLANE + (pix * SEGS + seg8 % SEGS) * 16) = R.g[u];
        }
#pragma unroll
        for (int u = 0; u < I_SLOTS; ++u) {
            const int idx = tid + u * WP_THREADS;
            const int seg8 = idx % (SEGS * CIT), pix = idx / (SEGS * CIT);
            if (idx < I_LOADS) *reinterpret_cast<uint4*>(Ibuf(buf) + (seg8 / SEGS) * I_PLANE + (pix * SEGS + seg8 % SEGS) * 16) = R.i[u];
        }
    };

    f32x16 acc[3][CIT][COT];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int a = 0; a < CIT; ++a)
#pragma unroll
            for (int c = 0; c < COT; ++c)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[t][a][c][j] = 0.f;

    auto compute = [&](int cur) {
        const char* G = Gbuf(cur);
        const char* I = Ibuf(cur) + wave * (WP_PW * PITCH);   // tap row dy = wave-1: halo rows shifted by `wave`
        if constexpr (sizeof(T) == 2) {
            const int i16 = lane & 15, g16 = lane >> 4;
            const int kh = g16 >> 1, cb = g16 & 1, q = i16 >> 2, pc = i16 & 3;
            typedef s16x4 __attribute__((address_space(3))) * lds_v4;
            const int lane_off = (kh * 8 + q) * PITCH + (cb * 16 + pc * 4) * 2;
            const char* gl = G + lane_off;
            const char* il = I + lane_off;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {  // K = 128 positions: image row ks>>1 of the patch, 16-position half ks&1
                const int goff = ks * 16 * PITCH;
                s16x8_t av[COT];
#pragma unroll
                for (int c = 0; c < COT; ++c) {
                    s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(gl + c * G_PLANE + goff));
                    s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(gl + c * G_PLANE + goff + 4 * PITCH));
                    av[c] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
                }
#pragma unroll
                for (int a = 0; a < CIT; ++a)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int ioff = a * I_PLANE + ((ks >> 1) * WP_PW + (ks & 1) * 16 + dx) * PITCH;
                        s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(il + ioff));
                        s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(il + ioff + 4 * PITCH));
                        const s16x8_t bv = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                        for (int c = 0; c < COT; ++c) acc[dx][a][c] = H16<T>::mma(av[c], bv, acc[dx][a][c]);
                    }
            }
        } else {
            const int r = lane & 31, h = lane >> 5;
#pragma unroll 8
            for (int ks = 0; ks < 64; ++ks) {  // 2 positions per MFMA
                const int pos = ks * 2 + h;     // 0..127 inside the patch
                float av[COT];
#pragma unroll
                for (int c = 0; c < COT; ++c) av[c] = *reinterpret_cast<const float*>(G + c * G_PLANE + pos * PITCH + r * 4);
                const int ipix = (pos >> 5) * WP_PW + (pos & 31);
#pragma unroll
                for (int a = 0; a < CIT; ++a)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const float bb = *reinterpret_cast<const float*>(I + a * I_PLANE + (ipix + dx) * PITCH + r * 4);
#pragma unroll
                        for (int c = 0; c < COT; ++c) acc[dx][a][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c], bb, acc[dx][a][c], 0, 0, 0);
                    }
            }
        }
    };

    // distance-1 prefetch (a second register set for distance 2 costs a wave of occupancy and measured slower)
    Regs R0;
    if (pbeg < pend) {
        gload(pbeg, R0);
        lstore(0, R0);
    }
    __syncthreads();
    const bool do_bias = p.bias_grad != nullptr && blockIdx.x == 0;  // one cin tile per cout slice sums the bias gradient
    float bsum[EPS];
#pragma unroll
    for (int i = 0; i < EPS; ++i) bsum[i] = 0.f;
    for (int patch = pbeg; patch < pend; ++patch) {
        const int cur = (patch - pbeg) & 1;
        if (patch + 1 < pend) gload(patch + 1, R0);
        compute(cur);
        if (do_bias) bias_grad_accumulate<T, COT, WP_THREADS>(Gbuf(cur), tid, bsum);
        if (patch + 1 < pend) lstore(cur ^ 1, R0);
        __syncthreads();
    }
    if (do_bias) bias_grad_flush<T, COT, WP_THREADS>(reinterpret_cast<float*>(lds), tid, bsum, p.bias_grad, co0, p.cout);
    // every wave owns its three taps: no cross-wave reduction
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int a = 0; a < CIT; ++a) {
        const int ci = ci0 + 32 * a + r;
        if (ci < p.cin_total) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                float* dst = p.partial + (((int64_t)split * 9 + wave * 3 + dx) * w_rows) * p.cin_total;
#pragma unroll
                for (int c = 0; c < COT; ++c)
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int co = co0 + 32 * c + (j & 3) + 8 * (j >> 2) + 4 * h;
                        if (co < w_rows) dst[(int64_t)co * p.cin_total + ci] = acc[dx][a][c][j];
                    }
            }
        }
    }
}

// Stride-2 3x3 weight gradient (encoder convs conv1..conv6, FAL_netB.py:101-111), bf16: the same wave-per-tap-row scheme
// as the dense kernel on a 4x32 block of OUTPUT positions; the (2*4+1)x(2*32+1) input region is loaded as whole contiguous
// rows and de-interleaved by row / column parity into four LDS planes (even/odd rows x even/odd columns), so that the
// pixels tap (ky,kx) needs for 16 consecutive outputs (2x+kx-1: stride 2 in the image) are 16 CONSECUTIVE rows of one
// plane -- the transposed reads and their conflict-free 64-B pitch are exactly those of the dense kernel.
//   tap ky: rows 2y+ky-1 -> ky=1: odd region rows (index y), ky=0 / 2: even region rows (index y / y+1); columns alike.
// (The per-tap gather kernel it replaces ran these layers at 65-130 TFLOP/s on the longest chain of the backward pass.)
#define WS2_RH (2 * WP_TH + 1)   // region rows
#define WS2_RW (2 * WP_TW + 1)   // region columns
template <typename T, int COT>
__global__ __launch_bounds__(WP_THREADS, 2) void wgrad3x3_s2_kernel(const falnet_wgrad_t p, int w_rows, int tiles_x, int tiles_y,
                                                                 int patches_per_split) {
    constexpr int EPS = 8, SEGS = 4, PITCH = 64;
    constexpr int NE_R = WP_TH + 1, NO_R = WP_TH, NE_C = WP_TW + 1, NO_C = WP_TW;  // even / odd region rows and columns
    // plane (row parity, column parity) -> pixel offset of its first pixel; E = even region index
    constexpr int P_EE = 0, P_EO = P_EE + NE_R * NE_C, P_OE = P_EO + NE_R * NO_C, P_OO = P_OE + NO_R * NE_C, I_PIX = P_OO + NO_R * NO_C;
    static_assert(I_PIX == WS2_RH * WS2_RW, "the four planes tile the region");
    constexpr int G_PLANE = WP_TH * WP_TW * PITCH;
    constexpr int G_BYTES = COT * G_PLANE, I_BYTES = I_PIX * PITCH;
    constexpr int G_LOADS = WP_TH * WP_TW * SEGS * COT, I_LOADS = I_PIX * SEGS;
    constexpr int G_SLOTS = (G_LOADS + WP_THREADS - 1) / WP_THREADS, I_SLOTS = (I_LOADS + WP_THREADS - 1) / WP_THREADS;
    // ONE LDS buffer (54 KB with COT = 2) + register prefetch of the next block: two workgroups per CU overlap each other
    __shared__ __attribute__((aligned(16))) char lds[G_BYTES + I_BYTES];
    auto Gbuf = [&](int) -> char* { return lds; };
    auto Ibuf = [&](int) -> char* { return lds + G_BYTES; };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32 * COT, split = blockIdx.z;
    const int c_first = p.src[0].C;
    const bool second = ci0 >= c_first;
    const T* s_ptr = reinterpret_cast<const T*>(second ? p.src[1].ptr : p.src[0].ptr) + (second ? ci0 - c_first : ci0);
    const int64_t s_sb = second ? p.src[1].sb : p.src[0].sb, s_sy = second ? p.src[1].sy : p.src[0].sy, s_sx = second ? p.src[1].sx : p.src[0].sx;
    const int npatch = p.B * tiles_x * tiles_y;
    const int pbeg = split * patches_per_split, pend = min(pbeg + patches_per_split, npatch);

    // region slots: (row, column, 16-B segment) -> LDS offset inside the parity plane (loop-invariant)
    short i_row[I_SLOTS], i_col[I_SLOTS];
    int i_lds[I_SLOTS];
#pragma unroll
    for (int u = 0; u < I_SLOTS; ++u) {
        const int idx = tid + u * WP_THREADS;
        const int seg = idx % SEGS, pix = idx / SEGS;
        const int r = pix / WS2_RW, c = pix % WS2_RW;
        i_row[u] = (short)r;
        i_col[u] = (short)c;
        const int base = (r & 1) ? ((c & 1) ? P_OO : P_OE) : ((c & 1) ? P_EO : P_EE);
        const int pw = (c & 1) ? NO_C : NE_C;
        i_lds[u] = idx < I_LOADS ? (base + (r >> 1) * pw + (c >> 1)) * PITCH + seg * 16 : -1;
    }
    struct Regs { uint4 g[G_SLOTS]; uint4 i[I_SLOTS]; };
    auto gload = [&](int patch, Regs& R) {
        int q = patch;
        const int tix = q % tiles_x;
        q /= tiles_x;
        const int tiy = q % tiles_y;
        const int b = q / tiles_y;
        const int y0 = tiy * WP_TH, x0 = tix * WP_TW;
        const T* gbase = reinterpret_cast<const T*>(p.gout) + ((int64_t)b * p.TH * p.TW) * p.gC + co0;
#pragma unroll
        for (int u = 0; u < G_SLOTS; ++u) {
            const int idx = tid + u * WP_THREADS;
            const int seg = idx % (SEGS * COT), pix = idx / (SEGS * COT);
            const int y = y0 + pix / WP_TW, x = x0 + pix % WP_TW;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (idx < G_LOADS && y < p.TH && x < p.TW && co0 + seg * EPS < p.gC)
                v = *reinterpret_cast<const uint4*>(gbase + ((int64_t)y * p.TW + x) * p.gC + seg * EPS);
            R.g[u] = v;
        }
        const T* ibase = s_ptr + (int64_t)b * s_sb;
#pragma unroll
        for (int u = 0; u < I_SLOTS; ++u) {
            const int idx = tid + u * WP_THREADS;
            uint4 v = make_uint4(0, 0, 0, 0);
            const int vy = 2 * y0 - 1 + i_row[u], vx = 2 * x0 - 1 + i_col[u];
            if (idx < I_LOADS && vy >= 0 && vy < p.IH && vx >= 0 && vx < p.IW)
                v = *reinterpret_cast<const uint4*>(ibase + (int64_t)vy * s_sy + (int64_t)vx * s_sx + (idx % SEGS) * EPS);
            R.i[u] = v;
        }
    };
    auto lstore = [&](int buf, const Regs& R) {
#pragma unroll
        for (int u = 0; u < G_SLOTS; ++u) {
            const int idx = tid + u * WP_THREADS;
            const int seg8 = idx % (SEGS * COT), pix = idx / (SEGS * COT);
            if (idx < G_LOADS) *reinterpret_cast<uint4*>(Gbuf(buf) + (seg8 / SEGS) * G_PLANE + (pix * SEGS + seg8 % SEGS) * 16) = R.g[u];
        }
#pragma unroll
        for (int u = 0; u < I_SLOTS; ++u)
            if (i_lds[u] >= 0) *reinterpret_cast<uint4*>(Ibuf(buf) + i_lds[u]) = R.i[u];
    };

    f32x16 acc[3][COT];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int c = 0; c < COT; ++c)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[t][c][j] = 0.f;
    const int i16 = lane & 15, g16 = lane >> 4;
    const int kh = g16 >> 1, cb = g16 & 1, q4 = i16 >> 2, pc = i16 & 3;
    typedef s16x4 __attribute__((address_space(3))) * lds_v4;
    const int lane_off = (kh * 8 + q4) * PITCH + (cb * 16 + pc * 4) * 2;
    // wave = ky: region-row parity and row shift inside the plane
    const bool odd_rows = wave == 1;
    const int row_shift = wave == 2 ? 1 : 0;

    auto compute = [&](int cur) {
        const char* gl = Gbuf(cur) + lane_off;
        const char* il = Ibuf(cur) + lane_off;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {  // K = 128 output positions: block row ks>>1, 16-position half ks&1
            const int goff = ks * 16 * PITCH;
            s16x8_t av[COT];
#pragma unroll
            for (int c = 0; c < COT; ++c) {
                s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(gl + c * G_PLANE + goff));
                s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(gl + c * G_PLANE + goff + 4 * PITCH));
                av[c] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
            }
            const int prow = (ks >> 1) + row_shift;  // row inside the parity plane
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                // column parity odd for kx = 1; even columns start at lx (kx = 0) or lx + 1 (kx = 2)
                const int pw = kx == 1 ? NO_C : NE_C;
                const int pbase = odd_rows ? (kx == 1 ? P_OO : P_OE) : (kx == 1 ? P_EO : P_EE);
                const int ioff = (pbase + prow * pw + (ks & 1) * 16 + (kx == 2 ? 1 : 0)) * PITCH;
                s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(il + ioff));
                s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(il + ioff + 4 * PITCH));
                const s16x8_t bv = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int c = 0; c < COT; ++c) acc[kx][c] = H16<T>::mma(av[c], bv, acc[kx][c]);
            }
        }
    };

    Regs R0;
    if (pbeg < pend) {
        gload(pbeg, R0);
        lstore(0, R0);
    }
    __syncthreads();
    const bool do_bias = p.bias_grad != nullptr && blockIdx.x == 0;
    float bsum[EPS];
#pragma unroll
    for (int i = 0; i < EPS; ++i) bsum[i] = 0.f;
    for (int patch = pbeg; patch < pend; ++patch) {
        if (patch + 1 < pend) gload(patch + 1, R0);
        compute(0);
        if (do_bias) bias_grad_accumulate<T, COT, WP_THREADS>(Gbuf(0), tid, bsum);
        __syncthreads();  // every wave is done reading this block
        if (patch + 1 < pend) lstore(0, R0);
        __syncthreads();
    }
    if (do_bias) bias_grad_flush<T, COT, WP_THREADS>(reinterpret_cast<float*>(lds), tid, bsum, p.bias_grad, co0, p.cout);
    const int r = lane & 31, h = lane >> 5;
    const int ci = ci0 + r;
    if (ci < p.cin_total) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            float* dst = p.partial + (((int64_t)split * 9 + wave * 3 + kx) * w_rows) * p.cin_total;
#pragma unroll
            for (int c = 0; c < COT; ++c)
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int co = co0 + 32 * c + (j & 3) + 8 * (j >> 2) + 4 * h;
                    if (co < w_rows) dst[(int64_t)co * p.cin_total + ci] = acc[kx][c][j];
                }
        }
    }
}

// First layer (Cin = 3) weight gradient, bf16 gout: dW[co][c][tap] = sum_p gout[p][co] * x[c][p + tap] straight from the PLANAR f32
// image (variant 6) -- the generic kernels need an NHWC copy of the image padded to 32 channels (a 67 MB conversion per step
// for 3 real channels).  GEMM view: D[co 32][k 32] += A[co][p] B[p][k], k = c*9 + tap (27 used): A fragments are the dense
// kernel's transposed gout reads, B fragments eight consecutive image columns (f32 -> bf16) of the lane's (c, tap) row in
// the LDS patch.  Four waves split the eight 16-position K steps of a 4x32 block; partial sums are reduced through LDS and
// written as a standard [tap][co][cin_pad] slab (the batched reduce un-pads it).
#define WC3_THREADS 256
template <typename T>
__global__ __launch_bounds__(WC3_THREADS) void wgrad3x3_c3_kernel(const falnet_wgrad_t p, int w_rows, int tiles_x, int tiles_y,
                                                                  int patches_per_split) {
    constexpr int PITCH = 64, SEGS = 4;
    constexpr int G_BYTES = WP_TH * WP_TW * PITCH, X_FLOATS = 3 * (WP_TH + 2) * WP_PW;
    constexpr int G_LOADS = WP_TH * WP_TW * SEGS, G_SLOTS = (G_LOADS + WC3_THREADS - 1) / WC3_THREADS;
    constexpr int X_SLOTS = (X_FLOATS + WC3_THREADS - 1) / WC3_THREADS;
    constexpr int BUF_BYTES = G_BYTES + ((X_FLOATS * 4 + 15) / 16) * 16;
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES > 4 * 32 * 33 * 4 ? 2 * BUF_BYTES : 4 * 32 * 33 * 4];
    auto Gbuf = [&](int b) -> char* { return lds + b * BUF_BYTES; };
    auto Xbuf = [&](int b) -> float* { return reinterpret_cast<float*>(lds + b * BUF_BYTES + G_BYTES); };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.z;
    const float* x = reinterpret_cast<const float*>(p.src[0].ptr);
    const int64_t HW = (int64_t)p.IH * p.IW;
    const int npatch = p.B * tiles_x * tiles_y;
    const int pbeg = split * patches_per_split, pend = min(pbeg + patches_per_split, npatch);

    struct Regs { uint4 g[G_SLOTS]; float xv[X_SLOTS]; };
    auto gload = [&](int patch, Regs& R) {
        int q = patch;
        const int tix = q % tiles_x;
        q /= tiles_x;
        const int tiy = q % tiles_y;
        const int b = q / tiles_y;
        const int y0 = tiy * WP_TH, x0 = tix * WP_TW;
        const T* gbase = reinterpret_cast<const T*>(p.gout) + ((int64_t)b * p.TH * p.TW) * p.gC;
#pragma unroll
        for (int u = 0; u < G_SLOTS; ++u) {
            const int idx = tid + u * WC3_THREADS;
            const int seg = idx % SEGS, pix = idx / SEGS;
            const int y = y0 + pix / WP_TW, xx = x0 + pix % WP_TW;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (idx < G_LOADS && y < p.TH && xx < p.TW) v = *reinterpret_cast<const uint4*>(gbase + ((int64_t)y * p.TW + xx) * p.gC + seg * 8);
            R.g[u] = v;
        }
#pragma unroll
        for (int u = 0; u < X_SLOTS; ++u) {
            const int idx = tid + u * WC3_THREADS;
            const int c = idx / ((WP_TH + 2) * WP_PW), rem = idx % ((WP_TH + 2) * WP_PW);
            const int vy = y0 - 1 + rem / WP_PW, vx = x0 - 1 + rem % WP_PW;
            R.xv[u] = (idx < X_FLOATS && vy >= 0 && vy < p.IH && vx >= 0 && vx < p.IW) ? x[((int64_t)b * 3 + c) * HW + (int64_t)vy * p.IW + vx] : 0.f;
        }
    };
    auto lstore = [&](int buf, const Regs& R) {
#pragma unroll
        for (int u = 0; u < G_SLOTS; ++u) {
            const int idx = tid + u * WC3_THREADS;
            if (idx < G_LOADS) *reinterpret_cast<uint4*>(Gbuf(buf) + idx * 16) = R.g[u];
        }
#pragma unroll
        for (int u = 0; u < X_SLOTS; ++u) {
            const int idx = tid + u * WC3_THREADS;
            if (idx < X_FLOATS) Xbuf(buf)[idx] = R.xv[u];
        }
    };

    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    const int i16 = lane & 15, g16 = lane >> 4;
    const int kh = g16 >> 1, cb = g16 & 1, q4 = i16 >> 2, pc = i16 & 3;
    typedef s16x4 __attribute__((address_space(3))) * lds_v4;
    const int lane_off = (kh * 8 + q4) * PITCH + (cb * 16 + pc * 4) * 2;
    const int r = lane & 31, h = lane >> 5;
    const bool kvalid = r < 27;
    const int kc = r / 9, kt = r % 9;
    const int koff = (kc * (WP_TH + 2) + kt / 3) * WP_PW + kt % 3;  // patch offset of this lane's (channel, tap)

    const bool do_bias = p.bias_grad != nullptr;
    float bsum[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bsum[i] = 0.f;
    Regs R0;
    if (pbeg < pend) {
        gload(pbeg, R0);
        lstore(0, R0);
    }
    __syncthreads();
    for (int patch = pbeg; patch < pend; ++patch) {
        const int cur = (patch - pbeg) & 1;
        if (patch + 1 < pend) gload(patch + 1, R0);
        const char* gl = Gbuf(cur) + lane_off;
        const float* X = Xbuf(cur);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int ks = wave * 2 + kk;  // 16-position K step: block row ks>>1, half ks&1
            s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(gl + ks * 16 * PITCH));
            s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(gl + ks * 16 * PITCH + 4 * PITCH));
            const s16x8_t av = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
            s16x8_t bv;
            const float* xr = X + koff + (ks >> 1) * WP_PW + (ks & 1) * 16 + h * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[j] = (short)H16<T>::bits(kvalid ? xr[j] : 0.f);
            acc = H16<T>::mma(av, bv, acc);
        }
        if (do_bias) bias_grad_accumulate<T, 1, WC3_THREADS>(Gbuf(cur), tid, bsum);
        if (patch + 1 < pend) lstore(cur ^ 1, R0);
        __syncthreads();
    }
    if (do_bias) {
        bias_grad_flush<T, 1, WC3_THREADS>(reinterpret_cast<float*>(lds), tid, bsum, p.bias_grad, 0, p.cout);
        __syncthreads();
    }
    // sum the four waves' partial tiles through LDS ([wave][co][k], pitch 33), then one thread per (co, k)
    float* red = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int co = (j & 3) + 8 * (j >> 2) + 4 * h;
        red[(wave * 32 + co) * 33 + r] = acc[j];
    }
    __syncthreads();
    for (int e = tid; e < 32 * 27; e += WC3_THREADS) {
        const int co = e / 27, k = e % 27;
        const float v = red[(0 * 32 + co) * 33 + k] + red[(1 * 32 + co) * 33 + k] + red[(2 * 32 + co) * 33 + k] + red[(3 * 32 + co) * 33 + k];
        const int c = k / 9, t = k % 9;
        if (co < w_rows) p.partial[(((int64_t)split * 9 + t) * w_rows + co) * p.cin_total + c] = v;
    }
}

// partial [nsplit][ntaps][w_rows][cin_total] -> OIHW f32, un-padding the (possibly two-group) channel axis
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int nsplit, int ntaps,
                                                           int w_rows, int cin_total, float* __restrict__ grad, int cout,
                                                           int cin, int c0_real, int c0_pad, int use_atomics) {
    // block = (output channel co, 64 packed input channels); blockIdx.z = slab group.  Reads are coalesced along
    // the packed channel axis; the [tap][ci] -> [ci][tap] transposition goes through LDS so that the OIHW
    // writes are contiguous runs of ntaps*64 floats.
    __shared__ float tile[64 * 9];
    const int co = blockIdx.x, cp0 = blockIdx.y * 64;
    const int ngroups = gridDim.z, grp = blockIdx.z;
    const int s0 = (int)((int64_t)nsplit * grp / ngroups), s1 = (int)((int64_t)nsplit * (grp + 1) / ngroups);
    const int64_t slab = (int64_t)ntaps * w_rows * cin_total;
    for (int e = threadIdx.x; e < ntaps * 64; e += blockDim.x) {
        const int t = e / 64, cl = e % 64;
        float s = 0.f;
        if (cp0 + cl < cin_total) {
            const float* src = partial + ((int64_t)t * w_rows + co) * cin_total + cp0 + cl;
            for (int k = s0; k < s1; ++k) s += src[k * slab];
        }
        tile[cl * ntaps + t] = s;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ntaps * 64; e += blockDim.x) {
        const int cl = e / ntaps, t = e % ntaps;
        const int cp = cp0 + cl;
        int ci = -1;
        if (cp < c0_pad) {
            if (cp < c0_real) ci = cp;
        } else if (c0_real + (cp - c0_pad) < cin) {
            ci = c0_real + (cp - c0_pad);
        }
        if (ci >= 0) {
            float* dst = grad + ((int64_t)co * cin + ci) * ntaps + t;
            if (use_atomics) atomicAdd(dst, tile[e]);
            else *dst = tile[e];
        }
    }
}

// db[c] += sum_p g[p, c]: every thread owns one 8-channel segment (16-B bf16 / 32-B f32 loads) and strides over
// pixels; rows of threads are summed through LDS, one atomic per channel per block.
template <typename T>
__global__ __launch_bounds__(256) void bias_grad_kernel(const T* __restrict__ g, int64_t npix, int gC, int cout,
                                                        float* __restrict__ db) {
    __shared__ float red[256 * 8];
    const int segs = gC / 8;                       // gC is a multiple of 32
    const int spb = segs < 256 ? segs : 256;       // segments handled per block pass
    const int rows = 256 / spb;
    const int sl = threadIdx.x % spb, rr = threadIdx.x / spb;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int seg = blockIdx.y * spb + sl; seg < segs; seg += gridDim.y * spb) {
        for (int64_t pix = (int64_t)blockIdx.x * rows + rr; pix < npix; pix += (int64_t)gridDim.x * rows) {
            Vec8<T> v;
            v.load(g + pix * gC + seg * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += v.get(i);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = acc[i];
        __syncthreads();
        if (rr == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float t = 0.f;
                for (int k = 0; k < rows; ++k) t += red[(k * spb + sl) * 8 + i];
                if (seg * 8 + i < cout) atomicAdd(db + seg * 8 + i, t);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    }
}

// ---- batched forms: ONE launch reduces the split-K slabs of every layer / sums every bias gradient ----------
// (a step has ~34 weight tensors and 13 biases; per-layer launches are launch-latency bound)
// Slab reduce, streaming form.  A block owns `cob` consecutive output channels of one layer (cob * cin_total <= 1024 packed
// input channels: for a fixed tap they are ONE contiguous run of the slab) and one group of slabs: thread i sums float4 i of
// that run for all NT taps over the group's slabs -- every wave load is 1 KiB contiguous, NT (x2: two slabs per trip)
// independent 16-B loads in flight per thread -- then the [tap][co][ci] sums are transposed through LDS ([co][ci][tap],
// stride-NT stores: odd stride, conflict-free) and leave as contiguous runs of the OIHW gradient: plain STORES when the
// block is the only writer (groups == 1 and the launch does not accumulate), 256-B-contiguous f32 atomics otherwise.
// (The previous form gave every block ONE output channel and 64 input channels: 256-B runs per load, 64 x 9 scalar atomics
// per block -- 3.5 TB/s on 758 MB of slabs.)
template <int NT>
__device__ __forceinline__ void wgrad_reduce_body(const falnet_reduce_t& d, int rel, float* __restrict__ tile /* 1024 * NT floats */, int accumulate) {
    const int cob = d.cin_total >= 1024 ? 1 : 1024 / d.cin_total;
    const int cblocks = (d.cout + cob - 1) / cob;
    const int grp = rel % d.groups, cb = rel / d.groups;
    if (cb >= cblocks) return;
    const int co0 = cb * cob, nco = min(cob, d.cout - co0);
    const int s0 = (int)((int64_t)d.nsplit * grp / d.groups), s1 = (int)((int64_t)d.nsplit * (grp + 1) / d.groups);
    const int64_t tapstride = (int64_t)d.w_rows * d.cin_total, slab = (int64_t)NT * tapstride;
    const int run = nco * d.cin_total;  // floats per tap of this block (a multiple of 32)
    for (int base = 0; base < run; base += 1024) {  // (one trip unless cin_total > 1024)
        const int i4 = base + threadIdx.x * 4;
        float4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i4 < run) {
            const float* src = d.partial + (int64_t)co0 * d.cin_total + i4;
            int k = s0;
            for (; k + 2 <= s1; k += 2) {
                float4 v[2][NT];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int t = 0; t < NT; ++t) v[u][t] = *reinterpret_cast<const float4*>(src + (k + u) * slab + t * tapstride);
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        acc[t].x += v[u][t].x;
                        acc[t].y += v[u][t].y;
                        acc[t].z += v[u][t].z;
                        acc[t].w += v[u][t].w;
                    }
            }
            for (; k < s1; ++k) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float4 v = *reinterpret_cast<const float4*>(src + k * slab + t * tapstride);
                    acc[t].x += v.x;
                    acc[t].y += v.y;
                    acc[t].z += v.z;
                    acc[t].w += v.w;
                }
            }
            const int l = threadIdx.x * 4;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                tile[(l + 0) * NT + t] = acc[t].x;
                tile[(l + 1) * NT + t] = acc[t].y;
                tile[(l + 2) * NT + t] = acc[t].z;
                tile[(l + 3) * NT + t] = acc[t].w;
            }
        }
        __syncthreads();
        const int nloc = min(1024, run - base);  // packed (co, ci) pairs of this trip
        for (int e = threadIdx.x; e < nloc * NT; e += blockDim.x) {
            const int l = e / NT, t = e - l * NT;
            const int g = base + l;
            const int col = g / d.cin_total, cp = g - col * d.cin_total;
            int ci = -1;
            if (cp < d.c0_pad) {
                if (cp < d.c0_real) ci = cp;
            } else if (d.c0_real + (cp - d.c0_pad) < d.cin) {
                ci = d.c0_real + (cp - d.c0_pad);
            }
            if (ci >= 0) {
                float* dst = d.grad + ((int64_t)(co0 + col) * d.cin + ci) * NT + t;
                // no-return atomics pipeline; a read-modify-write would serialise one memory round trip per element
                if (d.groups > 1 || accumulate) atomicAdd(dst, tile[e]);
                else *dst = tile[e];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_batched_kernel(const falnet_reduce_t* __restrict__ descs, int n, int accumulate) {
    __shared__ float tile[1024 * 9];
    __shared__ int entry_begin[64];
    const int li = find_entry(descs, n, entry_begin);
    const falnet_reduce_t d = descs[li];
    const int rel = blockIdx.x - d.block_begin;
    if (d.ntaps == 9) wgrad_reduce_body<9>(d, rel, tile, accumulate);
    else if (d.ntaps == 3) wgrad_reduce_body<3>(d, rel, tile, accumulate);
    else if (d.ntaps == 1) wgrad_reduce_body<1>(d, rel, tile, accumulate);
}

// Deterministic form: `ws` != nullptr -> every block writes its per-channel sums to ws[blockIdx.x][512] (plain stores) and
// bias_grad_finish_kernel adds them in block order (the atomic form's result depends on the order its blocks arrive in).
__global__ __launch_bounds__(512) void bias_grad_finish_kernel(const falnet_biasgrad_t* __restrict__ descs, const float* __restrict__ ws) {
    const falnet_biasgrad_t d = descs[blockIdx.x];
    const int c = threadIdx.x;
    if (c >= d.cout) return;
    float s = 0.f;
    for (int k = 0; k < d.blocks; ++k) s += ws[(int64_t)(d.block_begin + k) * 512 + c];
    d.db[c] += s;
}

template <typename T>
__global__ __launch_bounds__(256) void bias_grad_batched_kernel(const falnet_biasgrad_t* __restrict__ descs, int n, float* __restrict__ ws = nullptr) {
    __shared__ float red[256 * 8];
    __shared__ int entry_begin[64];
    const int li = find_entry(descs, n, entry_begin);
    const falnet_biasgrad_t d = descs[li];
    const int bx = blockIdx.x - d.block_begin, nbx = d.blocks;
    const T* g = reinterpret_cast<const T*>(d.g);
    const int segs = d.gC / 8;
    const int spb = segs < 256 ? segs : 256;
    const int rows = 256 / spb;
    const int sl = threadIdx.x % spb, rr = threadIdx.x / spb;
    for (int seg = sl; seg < segs; seg += spb) {
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int64_t pix = (int64_t)bx * rows + rr;
        const int64_t stride = (int64_t)nbx * rows;
        for (; pix + 7 * stride < d.npix; pix += 8 * stride) {  // eight independent 16-B loads in flight
            Vec8<T> v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j].load(g + (pix + j * stride) * d.gC + seg * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[i] += ((v[0].get(i) + v[1].get(i)) + (v[2].get(i) + v[3].get(i))) + ((v[4].get(i) + v[5].get(i)) + (v[6].get(i) + v[7].get(i)));
        }
        for (; pix < d.npix; pix += stride) {
            Vec8<T> v;
            v.load(g + pix * d.gC + seg * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += v.get(i);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = acc[i];
        __syncthreads();
        if (rr == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float t = 0.f;
                for (int k = 0; k < rows; ++k) t += red[(k * spb + sl) * 8 + i];
                if (seg * 8 + i < d.cout) {
                    if (ws) ws[(int64_t)blockIdx.x * 512 + seg * 8 + i] = t;
                    else atomicAdd(d.db + seg * 8 + i, t);
                }
            }
        }
        __syncthreads();
    }
}

// entries per batched launch: find_entry (common.h) stages the block_begin column in a 64-int LDS array
#define FALNET_BATCH_MAX_ENTRIES 64

extern "C" int falnet_wgrad_reduce_blocks(int cout, int cin_total, int groups) {
    if (cout <= 0 || cin_total <= 0 || groups <= 0) return -1;
    const int cob = cin_total >= 1024 ? 1 : 1024 / cin_total;
    return (cout + cob - 1) / cob * groups;
}

extern "C" int falnet_wgrad_reduce_batched(const falnet_reduce_t* descs_dev, int n, int total_blocks, int accumulate, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(descs_dev && n > 0 && n <= FALNET_BATCH_MAX_ENTRIES && total_blocks > 0, "wgrad_reduce_batched: bad argument (n <= 64)");
    hipLaunchKernelGGL(wgrad_reduce_batched_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n, accumulate ? 1 : 0);
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_bias_grad_batched(const falnet_biasgrad_t* descs_dev, int n, int total_blocks, int dtype, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(descs_dev && n > 0 && n <= FALNET_BATCH_MAX_ENTRIES && total_blocks > 0, "bias_grad_batched: bad argument (n <= 64)");
    FALNET_CHECK_ARG(!falnet_deterministic(), "bias_grad_batched: f32 atomics -- use falnet_bias_grad_batched_det in deterministic mode");
#define BIAS_B(T) hipLaunchKernelGGL(bias_grad_batched_kernel<T>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n, (float*)nullptr)
    FALNET_DISPATCH_DTYPE(dtype, BIAS_B);
#undef BIAS_B
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_bias_grad_batched_det(const falnet_biasgrad_t* descs_dev, int n, int total_blocks, int dtype, float* ws, int64_t ws_floats,
                                            void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(descs_dev && n > 0 && n <= FALNET_BATCH_MAX_ENTRIES && total_blocks > 0 && ws, "bias_grad_batched_det: bad argument (n <= 64)");
    FALNET_CHECK_ARG(ws_floats >= (int64_t)total_blocks * 512, "bias_grad_batched_det: workspace of %lld floats needed (512 per block)", (long long)total_blocks * 512);
#define BIAS_B(T) hipLaunchKernelGGL(bias_grad_batched_kernel<T>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, n, ws)
    FALNET_DISPATCH_DTYPE(dtype, BIAS_B);
#undef BIAS_B
    hipLaunchKernelGGL(bias_grad_finish_kernel, dim3(n), dim3(512), 0, (hipStream_t)stream, descs_dev, (const float*)ws);
    FALNET_RETURN_LAUNCH();
}

static inline int round32(int v) { return (v + 31) / 32 * 32; }

extern "C" int64_t falnet_wgrad_workspace_bytes(const falnet_wgrad_t* p) {
    if (!p) return -1;
    return (int64_t)p->nsplit * p->ntaps * round32(p->gC) * p->cin_total * (int64_t)sizeof(float);
}

// A/B switch for tests and profiling (conv.hip reads the same variable): FALNET_DISABLE_PATCH=1 routes dense 3x3 launches to the per-tap kernel
static bool g_disable_patch = [] { const char* e = falnet_ab_env("FALNET_DISABLE_PATCH"); return e && e[0] == '1'; }();

// kernel selection of falnet_wgrad -- ONE place (choose_wgrad_kernel), also behind falnet_wgrad_fuses_bias and falnet_wgrad_kernel_name: the
// host asks and re-derives nothing.  On WGK_BAD the error text is set.
static WgradChoice choose_wgrad_kernel(const falnet_wgrad_t& p) {
    WgradChoice c;
    const int w_rows = round32(p.gC);
    const bool h16 = p.dtype == FALNET_BF16 || p.dtype == FALNET_F16;
    const bool canon = falnet_wgrad_canonical_taps9(p);
    if (p.up2 && p.variant != 7) { falnet_set_error("wgrad: up2 (a deconv layer's gradient on the low-resolution grid) is a mode of variant 7 only"); return c; }
    if (p.variant == 6) {  // first layer: planar f32 3-channel source (src[0].ptr = [B][3][IH][IW] f32), 16-bit gout, Cout 32
        const bool ok = h16 && canon && p.isy == 1 && p.isx == 1 && p.TH == p.IH && p.TW == p.IW && p.gC == 32 && w_rows == 32 && p.cin_total == 32 && p.nsrc == 1;
        if (!ok) { falnet_set_error("wgrad: variant 6 is the Cin=3 / Cout=32 first layer in bf16 / f16 (dense 3x3, cin_total 32)"); return c; }
        c.kernel = falnet_wgrad_c3wave_applicable(p) ? WGK_C3WAVE : WGK_C3;  // the wave-streaming form where it applies, else the halo-patch form
        return c;
    }
    if (p.variant == 5) {  // stride-2 3x3 (16-bit): parity-plane halo kernel
        bool ok = h16 && canon && p.isy == 2 && p.isx == 2 && p.TW >= 16 && p.TH == (p.IH + 1) / 2 && p.TW == (p.IW + 1) / 2;
        for (int s = 0; s < p.nsrc && ok; ++s) ok = p.src[s].C % 32 == 0 && ((p.src[s].H == p.IH && p.src[s].W == p.IW) || (p.src[s].sy == 0 && p.src[s].sx == 0));
        if (!ok) { falnet_set_error("wgrad: variant 5 needs a 16-bit 3x3 stride-2 pad-1 launch with sources at the input size"); return c; }
        c.kernel = WGK_S2;
        c.cow = w_rows % 64 == 0 ? 2 : 1;
        return c;
    }
    if (p.variant == 8) {
        if (!falnet_wgrad_rows_s2_applicable(p)) { falnet_set_error("wgrad: variant 8 needs a 16-bit 3x3 stride-2 pad-1 launch with ONE source at the input size"); return c; }
        c.kernel = WGK_ROWS_S2;
        return c;
    }
    if (p.variant == 9) {
        if (!falnet_wgrad_wave_applicable(p)) { falnet_set_error("wgrad: variant 9 needs a 16-bit dense 3x3 stride-1 launch over ONE 32-channel NHWC source at the launch size, gC 32 or 64, TW >= 32"); return c; }
        c.kernel = WGK_WAVE;
        c.s2 = p.isy == 2;
        c.nco = c.s2 || p.gC == 64 ? 2 : 1;
        return c;
    }
    if (p.variant == 7) {
        if (!falnet_wgrad_rows_applicable(p)) { falnet_set_error("wgrad: variant 7 needs a 16-bit dense 3x3 stride-1 launch with sources at the launch size or half of it (up2: ONE source at the launch size; up2 = 1: nsplit a multiple of 4)"); return c; }
        c.kernel = WGK_ROWS;
        c.up2 = p.up2 == 2 ? 2 : p.up2 ? 1 : 0;
        return c;
    }
    // dense 3x3 stride-1 -> halo-patch kernel (one slab per workgroup; nsplit = pixel-range splits)
    const bool dense = canon && p.isy == 1 && p.isx == 1 && p.TH == p.IH && p.TW == p.IW && p.TW >= 16 && !g_disable_patch && p.variant != 1;
    if (dense) {
        if (p.variant == 3 || p.variant == 4) {  // 32 x 64 / 64 x 32 channels per workgroup (register staged, two workgroups per CU)
            const bool co2 = p.variant == 3;
            if (!(h16 && (co2 ? w_rows : p.cin_total) % 64 == 0)) { falnet_set_error("wgrad: variant %d needs 16-bit operands and a channel count that is a multiple of 64", p.variant); return c; }
            c.ciw = co2 ? 1 : 2;
            c.cow = co2 ? 2 : 1;
        }
        c.kernel = WGK_PATCH;
        return c;
    }
    c.kernel = WGK_TAP;
    return c;
}

static int check_wgrad_desc(const falnet_wgrad_t& p) {
    FALNET_CHECK_ARG(p.dtype == FALNET_F32 || p.dtype == FALNET_BF16 || p.dtype == FALNET_F16, "wgrad: bad dtype %d", p.dtype);
    FALNET_CHECK_ARG(p.nsrc == 1 || p.nsrc == 2, "wgrad: nsrc=%d", p.nsrc);
    int ctot = 0;
    if (p.variant != 6) {  // (variant 6 reads a planar f32 3-channel image: its own checks)
        for (int s = 0; s < p.nsrc; ++s) {
            if (int r = check_src(p.src[s], 32, "wgrad")) return r;
            ctot += p.src[s].C;
        }
        FALNET_CHECK_ARG(ctot == p.cin_total, "wgrad: sources carry %d channels, cin_total=%d", ctot, p.cin_total);
    } else {
        FALNET_CHECK_ARG(p.src[0].ptr && p.src[0].C == 3, "wgrad: variant 6 needs a 3-channel planar f32 source");
    }
    FALNET_CHECK_ARG(p.gout && p.gC > 0 && p.gC % 32 == 0 && p.nsplit >= 1 && p.ntaps >= 1 && p.ntaps <= 9, "wgrad: bad argument");
    FALNET_CHECK_ARG(p.B > 0 && p.TH > 0 && p.TW > 0, "wgrad: empty shape");
    FALNET_CHECK_ARG(p.cout >= 0 && p.cout <= p.gC, "wgrad: cout=%d exceeds gC=%d", p.cout, p.gC);
    return 0;
}

// the halo kernels of this file cut the launch into 4 x 32 patches, `pps` of them per split
struct PatchGrid {
    int w_rows, tiles_x, tiles_y, pps;
    explicit PatchGrid(const falnet_wgrad_t& p) : w_rows(round32(p.gC)), tiles_x((p.TW + WP_TW - 1) / WP_TW), tiles_y((p.TH + WP_TH - 1) / WP_TH) {
        pps = (p.B * tiles_x * tiles_y + p.nsplit - 1) / p.nsplit;
    }
};

static int launch_tap(const falnet_wgrad_t& p, const WgradChoice&, hipStream_t st) {
    const int w_rows = round32(p.gC);
    const dim3 grid((p.cin_total + WG_BN - 1) / WG_BN, (w_rows + WG_BM - 1) / WG_BM, p.ntaps * p.nsplit);
#define WG_TAP(T) hipLaunchKernelGGL(wgrad_kernel<T>, grid, dim3(CONV_THREADS), 0, st, p, w_rows)
    FALNET_DISPATCH_DTYPE(p.dtype, WG_TAP);
#undef WG_TAP
    return 0;
}

static int launch_patch(const falnet_wgrad_t& p, const WgradChoice& c, hipStream_t st) {
    const PatchGrid g(p);
#define WG_P(T, CI, CO) \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wgrad3x3_patch_kernel<T, CI, CO>), dim3(p.cin_total / (32 * CI), g.w_rows / (32 * CO), p.nsplit), dim3(WP_THREADS), 0, st, p, g.w_rows, g.tiles_x, g.tiles_y, g.pps)
#define WG_P12(T) WG_P(T, 1, 2)
#define WG_P21(T) WG_P(T, 2, 1)
#define WG_P11(T) WG_P(T, 1, 1)
    if (c.cow == 2) FALNET_DISPATCH_16(p.dtype, WG_P12);
    else if (c.ciw == 2) FALNET_DISPATCH_16(p.dtype, WG_P21);
    else FALNET_DISPATCH_DTYPE(p.dtype, WG_P11);
#undef WG_P11
#undef WG_P21
#undef WG_P12
#undef WG_P
    return 0;
}

static int launch_s2(const falnet_wgrad_t& p, const WgradChoice& c, hipStream_t st) {
    const PatchGrid g(p);
#define WG_S2(T, CO) \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wgrad3x3_s2_kernel<T, CO>), dim3(p.cin_total / 32, g.w_rows / (32 * CO), p.nsplit), dim3(WP_THREADS), 0, st, p, g.w_rows, g.tiles_x, g.tiles_y, g.pps)
#define WG_S2_2(T) WG_S2(T, 2)
#define WG_S2_1(T) WG_S2(T, 1)
    if (c.cow == 2) FALNET_DISPATCH_16(p.dtype, WG_S2_2);
    else FALNET_DISPATCH_16(p.dtype, WG_S2_1);
#undef WG_S2_1
#undef WG_S2_2
#undef WG_S2
    return 0;
}

static int launch_c3(const falnet_wgrad_t& p, const WgradChoice&, hipStream_t st) {
    const PatchGrid g(p);
#define WG_C3(T) hipLaunchKernelGGL(HIP_KERNEL_NAME(wgrad3x3_c3_kernel<T>), dim3(1, 1, p.nsplit), dim3(WC3_THREADS), 0, st, p, g.w_rows, g.tiles_x, g.tiles_y, g.pps)
    FALNET_DISPATCH_16(p.dtype, WG_C3);
#undef WG_C3
    return 0;
}

// One row per kernel: the symbol of the instantiation a choice selects (t = the mangled operand type), the function that launches it and
// whether it sums the bias gradient.  falnet_wgrad, falnet_wgrad_fuses_bias and falnet_wgrad_kernel_name all go through this table, so the
// reported symbol cannot drift from the kernel launched; a new kernel is one enum member (wgrad_dispatch.h), one branch of
// choose_wgrad_kernel and one row here.
struct WgradKernelRow {
    WgradKernel kernel;
    int (*symbol)(char* buf, int len, const char* t, const WgradChoice& c);
    int (*launch)(const falnet_wgrad_t& p, const WgradChoice& c, hipStream_t st);
    bool fuses_bias;  // (never in deterministic mode: the fused form adds with f32 atomics from every workgroup)
};
#define SYMBOL(...) [](char* buf, int len, const char* t, const WgradChoice& c) { (void)c; return snprintf(buf, len, __VA_ARGS__); }
static const WgradKernelRow wgrad_kernels[] = {
    {WGK_TAP, SYMBOL("_Z12wgrad_kernelI%sEv14falnet_wgrad_ti", t), launch_tap, false},
    {WGK_PATCH, SYMBOL("_Z21wgrad3x3_patch_kernelI%sLi%dELi%dEEv14falnet_wgrad_tiiii", t, c.ciw, c.cow), launch_patch, true},
    {WGK_S2, SYMBOL("_Z18wgrad3x3_s2_kernelI%sLi%dEEv14falnet_wgrad_tiiii", t, c.cow), launch_s2, true},
    {WGK_C3, SYMBOL("_Z18wgrad3x3_c3_kernelI%sEv14falnet_wgrad_tiiii", t), launch_c3, true},
    {WGK_C3WAVE, SYMBOL("_Z22wgrad3x3_c3wave_kernelI%sEv14falnet_wgrad_ti", t), falnet_wgrad_c3wave_launch, true},
    {WGK_ROWS, [](char* buf, int len, const char* t, const WgradChoice& c) {
         if (c.up2 == 2) return snprintf(buf, len, "_Z20wgrad3x3_up2q_kernelI%sLi2EEv14falnet_wgrad_tiiii", t);
         return snprintf(buf, len, "_Z22wgrad3x3_rows16_kernelI%sLi4ELi2ELb%dEEv14falnet_wgrad_tiiii", t, c.up2 == 1 ? 1 : 0);
     },
     falnet_wgrad_rows_launch, true},
    {WGK_ROWS_S2, SYMBOL("_Z23wgrad3x3_rows8s2_kernelI%sLi2EEv14falnet_wgrad_tiiii", t), falnet_wgrad_rows_s2_launch, true},
    {WGK_WAVE, SYMBOL("_Z22wgrad3x3_wave32_kernelI%sLi%dELb%dEEv14falnet_wgrad_ti", t, c.nco, c.s2 ? 1 : 0), falnet_wgrad_wave_launch, true},
};
#undef SYMBOL

// the choice for a checked descriptor and its row; nullptr with the error text set when the descriptor is refused
static const WgradKernelRow* wgrad_kernel_row(const falnet_wgrad_t& p, WgradChoice& c) {
    c = choose_wgrad_kernel(p);
    if (c.kernel == WGK_BAD) return nullptr;
    for (const WgradKernelRow& r : wgrad_kernels)
        if (r.kernel == c.kernel) return &r;
    falnet_set_error("wgrad: kernel %d has no table row", (int)c.kernel);
    return nullptr;
}

extern "C" int falnet_wgrad_fuses_bias(const falnet_wgrad_t* pp) {
    WgradChoice c;
    const WgradKernelRow* row = pp && check_wgrad_desc(*pp) == 0 ? wgrad_kernel_row(*pp, c) : nullptr;
    return row && row->fuses_bias && !falnet_deterministic() ? 1 : 0;
}

// Id (FALNET_WGK_*) and symbol of the kernel falnet_wgrad will launch for this descriptor (the name rocprofv3 reports): the same checks and
// the same choice, nothing issued, no pointer dereferenced, no workspace needed.
extern "C" int falnet_wgrad_kernel_name(const falnet_wgrad_t* pp, char* buf, int len) {
    FALNET_CHECK_ARG(pp && buf && len > 0, "wgrad_kernel_name: bad argument");
    if (check_wgrad_desc(*pp) != 0) return -1;
    WgradChoice c;
    const WgradKernelRow* row = wgrad_kernel_row(*pp, c);
    if (!row) return -1;
    row->symbol(buf, len, pp->dtype == FALNET_BF16 ? "DF16b" : pp->dtype == FALNET_F16 ? "DF16_" : "f", c);
    return (int)c.kernel;
}

extern "C" int falnet_wgrad(const falnet_wgrad_t* pp, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(pp, "wgrad: null descriptor");
    falnet_wgrad_t p = *pp;
    if (int r = check_wgrad_desc(p)) return r;
    FALNET_CHECK_ARG(p.partial, "wgrad: no workspace");
    if (p.cout == 0) p.cout = p.gC;
    WgradChoice c;
    const WgradKernelRow* row = wgrad_kernel_row(p, c);
    if (!row) return -1;
    if (p.bias_grad && !(row->fuses_bias && !falnet_deterministic())) {
        falnet_set_error("wgrad: bias_grad is set but the selected kernel (%d) cannot fuse it -- ask falnet_wgrad_fuses_bias first", (int)c.kernel);
        return -3;
    }
    if (int r = row->launch(p, c, (hipStream_t)stream)) return r;
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_wgrad_reduce(const float* partial, int nsplit, int ntaps, int cout_pad, int cin_total, float* grad,
                                   int cout, int cin, int c0_real, int c0_pad, int accumulate, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(partial && grad && nsplit >= 1 && ntaps >= 1 && ntaps <= 9 && cout > 0 && cin > 0 && cout <= cout_pad, "wgrad_reduce: bad argument");
    FALNET_CHECK_ARG(c0_real <= cin && c0_real <= c0_pad && c0_pad + (cin - c0_real) <= cin_total, "wgrad_reduce: channel groups do not fit");
    // slab groups: enough blocks to fill the chip when the weight tensor is small and the slab count large
    const int blocks = cout * ((cin_total + 63) / 64);
    int groups = 1;
    if (nsplit >= 16 && blocks < 1024) groups = (1024 + blocks - 1) / blocks;
    if (groups > nsplit / 8) groups = nsplit / 8 > 0 ? nsplit / 8 : 1;
    if (falnet_deterministic()) groups = 1;  // one writer per gradient element: slabs summed in slab order
    const int use_atomics = (groups > 1 || accumulate) ? 1 : 0;
    if (groups > 1 && !accumulate) {
        hipError_t e = hipMemsetAsync(grad, 0, sizeof(float) * (size_t)cout * cin * ntaps, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cout, (cin_total + 63) / 64, groups), dim3(256), 0, (hipStream_t)stream, partial,
                       nsplit, ntaps, cout_pad, cin_total, grad, cout, cin, c0_real, c0_pad, use_atomics);
    FALNET_RETURN_LAUNCH();
}

extern "C" int falnet_bias_grad(const void* g, int64_t npix, int gC, int cout, float* db, int accumulate, int dtype,
                                void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(g && db && npix > 0 && cout > 0 && cout <= gC, "bias_grad: bad argument");
    FALNET_CHECK_ARG(gC % 32 == 0 && gC <= 2048, "bias_grad: unsupported channel count %d", gC);
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(db, 0, sizeof(float) * cout, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    const int segs = gC / 8, spb = segs < 256 ? segs : 256, rows = 256 / spb;
    int64_t gx = (npix + rows * 16 - 1) / (rows * 16);
    gx = gx < 1 ? 1 : (gx > 512 ? 512 : gx);
    if (falnet_deterministic()) gx = 1;  // one block = one add per channel (slow; the batched _det form is the training path)
    const dim3 grid((unsigned)gx, 1);
#define BIAS_L(T) hipLaunchKernelGGL(bias_grad_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)g, npix, gC, cout, db)
    FALNET_DISPATCH_DTYPE(dtype, BIAS_L);
#undef BIAS_L
    FALNET_RETURN_LAUNCH();
}
