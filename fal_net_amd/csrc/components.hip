// Connected components of a batch of depth or disparity maps: per pixel the smallest pixel index of its component and the component's size
// (include/falnet_hip.h; the numpy restatement is tests/_components_ref.py).
//   valid pixel g = i W + j   lo < v && v <= hi and, with a score map, score >= threshold (every comparison with a NaN is false);
//   edge                      two 4-neighbours, both valid, with max(vp, vq) <= min(vp, vq) * ratio: one f32 multiply (the mesh's keep rule);
//   label                     the smallest index of the component, -1 for an invalid pixel; size: its pixel count, 0 for an invalid pixel.
// Four launches serve the whole batch (blockIdx.y is the image); the kernel boundaries are the only hand-offs between workgroups:
//   1  cc_tile_kernel      a workgroup of 256 threads owns a 16 x 64 tile: values staged with the right column and the row below (an invalid pixel as
//                          a NaN), the flag byte of every pixel (valid, right edge, down edge, tile root), a union-find over the tile's own edges in LDS
//                          (atomic min), flattened; parent[g] = the tile root as an index of the image.  Row-major order inside a tile agrees with
//                          the image's, so the smallest local index is the smallest index.  Clears the root-indexed counts.
//   2  cc_merge_kernel     one thread per pixel of a tile's first row (column) whose up (left) edge crosses the tile border: the lock-free union on
//                          `parent` -- both roots, then old = atomicMin(&parent[hi], lo); done when old == hi, else on with (old, lo).  Every value ever
//                          stored in parent[x] is a member of x's component and <= x, so a stale read costs an iteration, never correctness.  Parents
//                          are read with relaxed agent-scope atomic loads and changed by agent-scope atomics only: the eight XCDs share no L2.
//                          Only tile roots are ever relinked: a pixel that is no tile root keeps pointing at its tile root.
//   3  cc_flatten_kernel   per tile again; `parent` is only read in this launch (plain loads).  The tile roots walk to their roots; every other
//                          pixel takes the result of its tile root from LDS -- one walk per (tile, tile component), not per pixel -- and writes its
//                          label.  The pixels of each tile root are counted in LDS, then ONE integer atomicAdd per (tile, tile root) goes to count[root].
//   4  cc_size_kernel      size = count[label]; components, valid pixels (integer adds) and the largest size (an integer max) per image.
// No workgroup waits for another: no flag, no spin, no cooperative launch.  Every data-dependent loop (the walk of a find, the retry of a union)
// runs at most H W times -- a walk strictly descends and a retry strictly lowers `hi`, so a correct kernel never gets there -- and past that sets
// a bit of the status word and leaves.  Integer atomics only, and their results do not depend on the order of arrival: min, add and max of
// integers.  Not on the training step's path, not replayable, and not part of the autotune key (ops.py: _TUNE_SOURCES).
#include <math.h>
#include "common.h"

#define CC_THREADS 256
#define CC_TH 16
#define CC_TW 64
#define CC_PER_THREAD 4  // consecutive pixels of one tile row
#define CC_VALID 1u
#define CC_RIGHT 2u
#define CC_DOWN 4u
#define CC_ROOT 8u
#define CC_MAX_BATCH 65535         // gridDim.y; a larger batch takes one more launch set per 65535 images
#define CC_MAX_TILE_BLOCKS 4194304  // gridDim.x of the per-tile kernels, which stride over the tiles of an image

struct CcShape {  // by value in the kernel arguments
    int H, W, tiles_x, tiles;
    uint32_t n;  // H W: the cap of every data-dependent loop
};

__device__ __forceinline__ bool cc_edge(float vp, float vq, float ratio) {  // false when either is a NaN
    return fmaxf(vp, vq) <= __fmul_rn(fminf(vp, vq), ratio) && vp == vp && vq == vq;
}

__device__ __forceinline__ void cc_fail(unsigned long long* status, unsigned long long bit) { atomicOr(status, bit); }

// The root of x.  SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for a tile's parents in LDS, __HIP_MEMORY_SCOPE_AGENT for the image's.
template <int SCOPE>
__device__ __forceinline__ int cc_find(const int* p, int x, uint32_t cap, bool& bad) {
    for (uint32_t it = 0; it < cap; ++it) {  // at most cap - 1 descents and the look at the root
        const int q = __hip_atomic_load(p + x, __ATOMIC_RELAXED, SCOPE);
        if (q == x) return x;
        x = q;
    }
    bad = true;
    return x;
}

template <int SCOPE>
__device__ __forceinline__ void cc_union(int* p, int a, int b, uint32_t cap, bool& bad) {
    a = cc_find<SCOPE>(p, a, cap, bad);
    b = cc_find<SCOPE>(p, b, cap, bad);
    if (bad) return;
    for (uint32_t it = 0; it < cap; ++it) {  // max(a, b) falls with every retry
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = __hip_atomic_fetch_min(p + hi, lo, __ATOMIC_RELAXED, SCOPE);
        if (old == hi) return;  // hi was a root and now hangs below lo
        a = old, b = lo;        // hi had a parent already: that one and lo are still to be joined
    }
    bad = true;
}

// tile `t` of the image: its first row and column
__device__ __forceinline__ void cc_tile_origin(const CcShape& s, int t, int& i0, int& j0) {
    const int ty = t / s.tiles_x;
    i0 = ty * CC_TH, j0 = (t - ty * s.tiles_x) * CC_TW;
}

__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const float* __restrict__ map, const float* __restrict__ score, float threshold, float lo, float hi,
                                                             float ratio, CcShape s, int* __restrict__ parent, int* __restrict__ count,
                                                             unsigned char* __restrict__ flags, unsigned long long* status) {
    __shared__ float sv[CC_TH + 1][CC_TW + 1];
    __shared__ int par[CC_TH * CC_TW];
    const size_t img = (size_t)blockIdx.y * s.n;
    map += img, parent += img, count += img, flags += img;
    if (score) score += img;
    const int r = threadIdx.x >> 4, c0 = (threadIdx.x & 15) * CC_PER_THREAD;
    const float nanv = __uint_as_float(0x7fc00000u);
    auto value = [&](int i, int j) -> float {  // the pixel's value when it is valid, a NaN when it is not or lies outside the image
        if (i >= s.H || j >= s.W) return nanv;
        const uint32_t g = (uint32_t)i * (uint32_t)s.W + (uint32_t)j;
        const float v = map[g];
        bool ok = lo < v && v <= hi;
        if (ok && score) ok = score[g] >= threshold;
        return ok ? v : nanv;
    };
    bool bad = false;
    for (int t = blockIdx.x; t < s.tiles; t += gridDim.x) {
        int i0, j0;
        cc_tile_origin(s, t, i0, j0);
#pragma unroll
        for (int k = 0; k < CC_PER_THREAD; ++k) {
            sv[r][c0 + k] = value(i0 + r, j0 + c0 + k);
            par[r * CC_TW + c0 + k] = r * CC_TW + c0 + k;
        }
        if (threadIdx.x < CC_TW) sv[CC_TH][threadIdx.x] = value(i0 + CC_TH, j0 + (int)threadIdx.x);
        else if (threadIdx.x < CC_TW + CC_TH) sv[threadIdx.x - CC_TW][CC_TW] = value(i0 + (int)threadIdx.x - CC_TW, j0 + CC_TW);
        __syncthreads();
        uint32_t f[CC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < CC_PER_THREAD; ++k) {
            const int c = c0 + k, l = r * CC_TW + c;
            const float v = sv[r][c];
            f[k] = (v == v ? CC_VALID : 0u) | (cc_edge(v, sv[r][c + 1], ratio) ? CC_RIGHT : 0u) | (cc_edge(v, sv[r + 1][c], ratio) ? CC_DOWN : 0u);
            if ((f[k] & CC_RIGHT) && c + 1 < CC_TW) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, l + 1, s.n, bad);
            if ((f[k] & CC_DOWN) && r + 1 < CC_TH) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, l + CC_TW, s.n, bad);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CC_PER_THREAD; ++k) {
            const int c = c0 + k, l = r * CC_TW + c;
            const int i = i0 + r, j = j0 + c;
            if (i < s.H && j < s.W) {
                const uint32_t g = (uint32_t)i * (uint32_t)s.W + (uint32_t)j;
                int label = -1;
                if (f[k] & CC_VALID) {
                    const int root = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, s.n, bad);  // nothing changes par any more
                    label = (i0 + root / CC_TW) * s.W + j0 + root % CC_TW;
                    if (root == l) f[k] |= CC_ROOT;
                }
                parent[g] = label;
                count[g] = 0;
                flags[g] = (unsigned char)f[k];
            }
        }
        __syncthreads();  // the next tile stages over sv and par
    }
    if (bad) cc_fail(status, 1ull);
}

// Per image (tiles_y - 1) W threads for the pixels below a horizontal tile border, then (tiles_x - 1) H for those right of a vertical one.
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(CcShape s, uint32_t n_rows, uint32_t n_total, int* parent, const unsigned char* __restrict__ flags,
                                                              unsigned long long* status) {
    const uint32_t t = blockIdx.x * CC_THREADS + threadIdx.x;
    if (t >= n_total) return;
    const size_t img = (size_t)blockIdx.y * s.n;
    parent += img, flags += img;
    uint32_t g, nb;
    unsigned bit;
    if (t < n_rows) {
        const uint32_t ty = t / (uint32_t)s.W + 1u, j = t % (uint32_t)s.W;
        g = ty * CC_TH * (uint32_t)s.W + j, nb = g - (uint32_t)s.W, bit = CC_DOWN;
    } else {
        const uint32_t u = t - n_rows, tx = u / (uint32_t)s.H + 1u, i = u % (uint32_t)s.H;
        g = i * (uint32_t)s.W + tx * CC_TW, nb = g - 1u, bit = CC_RIGHT;
    }
    if (!(flags[nb] & bit)) return;
    bool bad = false;
    cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)nb, (int)g, s.n, bad);
    if (bad) cc_fail(status, 2ull);
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(CcShape s, const int* __restrict__ parent, const unsigned char* __restrict__ flags,
                                                                int* __restrict__ label, int* count, unsigned long long* status) {
    __shared__ int root_of[CC_TH * CC_TW];  // of a tile root: the root of its component
    __shared__ int cnt[CC_TH * CC_TW];      // of a tile root: the pixels of the tile that hang below it
    const size_t img = (size_t)blockIdx.y * s.n;
    parent += img, flags += img, label += img, count += img;
    const int r = threadIdx.x >> 4, c0 = (threadIdx.x & 15) * CC_PER_THREAD;
    bool bad = false;
    for (int t = blockIdx.x; t < s.tiles; t += gridDim.x) {
        int i0, j0;
        cc_tile_origin(s, t, i0, j0);
        uint32_t f[CC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < CC_PER_THREAD; ++k) {
            const int c = c0 + k, l = r * CC_TW + c, i = i0 + r, j = j0 + c;
            const uint32_t g = (uint32_t)i * (uint32_t)s.W + (uint32_t)j;
            f[k] = (i < s.H && j < s.W) ? flags[g] : 0u;
            cnt[l] = 0;
            root_of[l] = -1;
            if (f[k] & CC_ROOT) {
                int x = (int)g;
                uint32_t it = 0;
                for (; it < s.n; ++it) {  // parent is read-only in this launch
                    const int q = parent[x];
                    if (q == x) break;
                    x = q;
                }
                bad |= it == s.n;
                root_of[l] = x;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CC_PER_THREAD; ++k) {
            const int c = c0 + k, l = r * CC_TW + c, i = i0 + r, j = j0 + c;
            if (i < s.H && j < s.W) {
                const uint32_t g = (uint32_t)i * (uint32_t)s.W + (uint32_t)j;
                int out = -1;
                if (f[k] & CC_VALID) {
                    int lr = l;
                    if (!(f[k] & CC_ROOT)) {  // still the tile root the tile pass wrote: the merge relinks tile roots only
                        const int p = parent[g], pi = p / s.W;
                        lr = ((pi - i0) * CC_TW + (p - pi * s.W - j0)) & (CC_TH * CC_TW - 1);  // inside the tile; the mask keeps a wrong parent in LDS
                    }
                    out = root_of[lr];
                    atomicAdd(&cnt[lr], 1);
                }
                label[g] = out;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CC_PER_THREAD; ++k)
            if (f[k] & CC_ROOT) atomicAdd(&count[root_of[r * CC_TW + c0 + k]], cnt[r * CC_TW + c0 + k]);
        __syncthreads();  // the next tile clears cnt
    }
    if (bad) cc_fail(status, 4ull);
}

__device__ __forceinline__ int cc_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int cc_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(CC_THREADS) void cc_size_kernel(uint32_t n, const int* __restrict__ label, const int* __restrict__ count, int* __restrict__ size,
                                                             unsigned long long* info) {
    const size_t img = (size_t)blockIdx.y * n;
    const uint32_t g = blockIdx.x * CC_THREADS + threadIdx.x;
    int comps = 0, valid = 0, largest = 0;
    if (g < n) {
        const int l = label[img + g];
        const int sz = (l >= 0 && (uint32_t)l < n) ? count[img + l] : 0;
        size[img + g] = sz;
        valid = l >= 0 ? 1 : 0;
        comps = l == (int)g ? 1 : 0;
        largest = comps ? sz : 0;
    }
    comps = cc_wave_sum(comps), valid = cc_wave_sum(valid), largest = cc_wave_max(largest);
    if ((threadIdx.x & 63) == 0 && valid) {  // a wave without a valid pixel adds nothing
        unsigned long long* o = info + 3 * (size_t)blockIdx.y;
        if (comps) atomicAdd(o, (unsigned long long)comps);
        atomicAdd(o + 1, (unsigned long long)valid);
        if (largest) atomicMax(o + 2, (unsigned long long)largest);
    }
}

static int64_t cc_round8(int64_t v) { return (v + 7) & ~(int64_t)7; }
static bool cc_shape_ok(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return false;
    const int64_t n = (int64_t)H * W;
    return n < ((int64_t)1 << 30) && (int64_t)B * n < ((int64_t)1 << 31);
}

// workspace: the parents, the labels (used when the caller wants none), the root-indexed counts -- int32 per pixel each -- and the flag bytes
extern "C" int64_t falnet_components_workspace_bytes(int B, int H, int W) {
    if (!cc_shape_ok(B, H, W)) return 0;
    const int64_t bn = (int64_t)B * H * W;
    return 3 * cc_round8(4 * bn) + cc_round8(bn);
}

extern "C" int falnet_components(const float* map, const float* score, float threshold, float lo, float hi, float ratio, int B, int H, int W, int32_t* label,
                                 int32_t* size, int64_t* info, void* workspace, void* stream) {
    FALNET_ENTER(stream);
    FALNET_CHECK_ARG(cc_shape_ok(B, H, W), "components: %d maps of %d x %d: need B >= 1, 1 <= H W < 2^30 and B H W < 2^31", B, H, W);
    FALNET_CHECK_ARG(map && size, "components: null map or size output");
    FALNET_CHECK_ARG(info && workspace, "components: null info or workspace");
    FALNET_CHECK_ARG(lo >= 0.f && lo < hi, "components: need 0 <= lo < hi (hi may be infinite), got %g and %g", (double)lo, (double)hi);
    FALNET_CHECK_ARG(ratio >= 1.f, "components: ratio %g must be >= 1 (infinity joins all valid neighbours)", (double)ratio);
    FALNET_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)info) & 7) == 0, "components: workspace and info must be 8-byte aligned");
    FALNET_CHECK_ARG((((uintptr_t)map | (uintptr_t)score | (uintptr_t)label | (uintptr_t)size) & 3) == 0, "components: maps and outputs must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(info, 0, (3 * (size_t)B + 1) * sizeof(int64_t), st);
    if (e != hipSuccess) {
        falnet_set_error("components: clearing info failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    CcShape s;
    s.H = H, s.W = W, s.n = (uint32_t)H * (uint32_t)W;
    s.tiles_x = (W + CC_TW - 1) / CC_TW;
    const int tiles_y = (H + CC_TH - 1) / CC_TH;
    s.tiles = s.tiles_x * tiles_y;  // < 2^30 / 16
    const int64_t bn = (int64_t)B * s.n;
    int* parent = static_cast<int*>(workspace);
    int* own_label = parent + cc_round8(4 * bn) / 4;
    int* count = own_label + cc_round8(4 * bn) / 4;
    unsigned char* flags = reinterpret_cast<unsigned char*>(count + cc_round8(4 * bn) / 4);
    int* lab = label ? label : own_label;
    unsigned long long* status = reinterpret_cast<unsigned long long*>(info) + 3 * (size_t)B;
    const uint32_t n_rows = (uint32_t)(tiles_y - 1) * (uint32_t)W, n_border = n_rows + (uint32_t)(s.tiles_x - 1) * (uint32_t)H;  // < 2^27
    const unsigned tile_blocks = (unsigned)(s.tiles < CC_MAX_TILE_BLOCKS ? s.tiles : CC_MAX_TILE_BLOCKS);
    const dim3 threads(CC_THREADS);
    for (int b0 = 0; b0 < B; b0 += CC_MAX_BATCH) {  // one round for any batch a grid's second dimension holds
        const unsigned nb = (unsigned)(B - b0 < CC_MAX_BATCH ? B - b0 : CC_MAX_BATCH);
        const size_t off = (size_t)b0 * s.n;
        hipLaunchKernelGGL(cc_tile_kernel, dim3(tile_blocks, nb), threads, 0, st, map + off, score ? score + off : nullptr, threshold, lo, hi, ratio, s, parent + off,
                           count + off, flags + off, status);
        if (n_border)
            hipLaunchKernelGGL(cc_merge_kernel, dim3((n_border + CC_THREADS - 1) / CC_THREADS, nb), threads, 0, st, s, n_rows, n_border, parent + off,
                               (const unsigned char*)(flags + off), status);
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(tile_blocks, nb), threads, 0, st, s, (const int*)(parent + off), (const unsigned char*)(flags + off), lab + off,
                           count + off, status);
        hipLaunchKernelGGL(cc_size_kernel, dim3((s.n + CC_THREADS - 1) / CC_THREADS, nb), threads, 0, st, s.n, (const int*)(lab + off), (const int*)(count + off),
                           size + off, reinterpret_cast<unsigned long long*>(info) + 3 * (size_t)b0);
    }
    FALNET_RETURN_LAUNCH();
}
