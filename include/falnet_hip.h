/*
 * falnet_hip.h -- C-ABI of libfalnet_hip.so: the MI355X (gfx950) kernels behind the
 * FAL_netB hot path.
 *
 * The reference (JuanLuisGonzalez/FAL_net) has no native code: its "FFI" for this path is
 * torch.nn.functional -> aten/cuDNN.  Each entry point below replaces the aten call sites
 * named in its comment (paths relative to the reference root).  The library is loaded with
 * ctypes by fal_net_amd/_lib.py; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain `extern "C"`, raw device pointers, explicit sizes; no torch types.
 *   - every launch function takes the HIP stream (as void*) and enqueues only on it; it never
 *     allocates, never synchronises and never touches the default stream; on entry it makes the
 *     stream's device current (hipStreamGetDevice + hipSetDevice).  Workspaces are caller-owned:
 *     falnet_wgrad_workspace_bytes (split-K slabs), falnet_conv_t::splitk_ws (+ _bytes, M * w_rows
 *     floats for a split-K launch); no other entry point needs scratch memory.
 *   - return value: 0 ok, <0 bad argument (see falnet_last_error()), >0 hipError_t.
 *   - re-entrant: forward runs on the Python main thread, backward on autograd's thread.
 *   - dtype enum: activations/weights are FALNET_F32 (exact-f32 MFMA, parity path), FALNET_BF16
 *     (bf16 MFMA, f32 accumulate; throughput path) or FALNET_F16 (IEEE half MFMA, f32 accumulate:
 *     11 significant bits instead of bf16's 8; BASELINE configs[4]).  Reductions, losses, the MED
 *     head and Adam are f32 in all three.
 *   - activation layout inside the network: NHWC ("pixel-major"), channels padded to a
 *     multiple of falnet_channel_pad(dtype) with zeros.  The boundary tensors of the
 *     reference API (images, disparity, synthesised view, MED logits) are planar NCHW f32.
 *   - kernel-selection switches (A/B and tests; read once from the environment): FALNET_DISABLE_PATCH,
 *     FALNET_PATCH_KCB (conv.hip), FALNET_WR_FORM / FALNET_WR_ABL (wgrad_rows.hip), FALNET_HEAD_V1,
 *     FALNET_HEAD_BWD_V1, FALNET_HEAD_PAIR, FALNET_HEAD_FWD2, FALNET_HEAD_BWD2, FALNET_HEAD_WAVE (MED head), FALNET_MFMA16 (16x16x32 form of the
 *     weight-stationary kernel), FALNET_WS2_FULL (whole-line loads of the two-phase weight-stationary kernel, variant 16), FALNET_GEMM_WAVE
 *     (small f32 GEMM).  Host side (fal_net_amd/ops.py): FALNET_WS2 / FALNET_NO_DMA / FALNET_S2F_DMA gate autotune candidates.
 */
#ifndef FALNET_HIP_H
#define FALNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { FALNET_F32 = 0, FALNET_BF16 = 1, FALNET_F16 = 2 };
enum { FALNET_ACT_NONE = 0, FALNET_ACT_ELU = 1, FALNET_ACT_RELU = 2 };
enum { FALNET_OUT_NHWC = 0, FALNET_OUT_PLANAR_F32 = 1 };

int falnet_version(void);
const char* falnet_last_error(void);
/* channel padding granule (elements) of NHWC tensors and packed weights: 32 for every dtype */
int falnet_channel_pad(int dtype);
/* Every launch function makes the device that owns its `stream` argument current on the calling thread before it enqueues
 * (forward runs on the Python main thread, backward on autograd's worker thread: no thread-local HIP state is assumed).
 * falnet_set_device is for callers that use the NULL stream from a thread whose current device is not the tensors'. */
int falnet_set_device(int device);
/* Deterministic mode (process-wide switch, default off): every result becomes bit-identical from run to run for identical inputs,
 * launch sequence and kernel choices.  What changes: scalar loss reductions add their per-workgroup partials in workgroup order
 * (last-arriver pattern over a static scratch: run them on ONE stream per device); falnet_wgrad_fuses_bias reports 0 (the fused
 * bias gradient adds with atomics); split-K convolution launches (ksplit > 1) are refused with -2; falnet_bias_grad_batched is
 * refused in favour of falnet_bias_grad_batched_det; falnet_wgrad_reduce / falnet_bias_grad use a single writer per element.  The
 * CALLER keeps `groups` = 1 in its falnet_reduce_t tables and makes its kernel choices reproducible (fal_net_amd.ops with
 * FALNET_DETERMINISTIC=1: cached or heuristic variants, no timing).  Throughput drops (no split-K on the deep levels, a second
 * pass for the bias gradients): a debugging / regression-hunting switch, like torch.use_deterministic_algorithms. */
int falnet_set_deterministic(int on);
int falnet_get_deterministic(void);

/* One input of a convolution: NHWC tensor (or a per-sample constant when sy = sx = 0). */
typedef struct {
    const void* ptr;
    int32_t C;          /* channels consumed (multiple of the channel pad) */
    int32_t H, W;       /* physical spatial size; != (IH, IW) means nearest-upsampled on the fly */
    int64_t sb, sy, sx; /* element strides: sample, row, pixel */
} falnet_src_t;

/*
 * Implicit-GEMM convolution on MFMA: out[p, co] = epilogue(sum_{tap, src, ci} in_src[nbr(p, tap), ci] * w[co, tap, ci]).
 * One kernel serves
 *   - forward 3x3 / 1x1, stride 1 / 2            (models/FAL_netB.py:38,45,55,73,75,127,190; loss_functions.py:21-29)
 *   - the fused nearest upsample of `deconv`     (FAL_netB.py:58)   via src.H/W != IH/IW
 *   - the fused channel concat                   (FAL_netB.py:145-173) via two sources
 *   - data gradients (the autograd of the above): a dgrad is the same gather with another tap table;
 *     stride-2 dgrad is 4 launches, one per output parity class.
 * Tile space (TH x TW positions per sample): position (ty, tx) reads virtual input pixel
 * (ty*isy + dy[t], tx*isx + dx[t]) for tap t (zero outside [0,IH)x[0,IW)) and writes output pixel
 * (ty*osy + ooy, tx*osx + oox).
 * Epilogue: v = acc + bias[co]; v += addend[p, co]; v = act(v); v *= act'(actout[p, co]); store.
 */
typedef struct {
    falnet_src_t src[2];
    int32_t nsrc;
    int32_t IH, IW;            /* virtual input size */
    const void* weight;        /* packed [CoutPad][ntaps_w][CinTot] in `dtype` (falnet_pack_weights) */
    int32_t cin_total;         /* CinTot: row length per tap of the packed weight */
    int32_t ntaps;             /* taps walked by this launch (<= 9) */
    int32_t tap_dy[9], tap_dx[9], tap_w[9]; /* offsets and packed-weight tap index */
    int32_t w_taps;            /* ntaps_w of the packed weight */
    int32_t w_rows;            /* CoutPad: rows of the packed weight (multiple of 32) */
    int32_t isy, isx;
    int32_t B, TH, TW;
    int32_t osy, osx, ooy, oox;
    void* out;                 /* NHWC `dtype` [B][OH][OW][out_cstride] or planar f32 [B][Cout][OH][OW] */
    int32_t OH, OW;
    int32_t Cout;              /* channels written: NHWC -> padded count, planar -> real count */
    int32_t out_cstride;
    int32_t out_layout;
    const float* bias;         /* [CoutPad] or NULL */
    const void* addend;        /* NHWC like out, or NULL (may alias out: accumulate) */
    int32_t act;               /* FALNET_ACT_* applied to v */
    const void* actout;        /* NHWC like out: multiply by d act / d pre computed from the activation output */
    int32_t actout_kind;       /* FALNET_ACT_ELU / RELU / NONE */
    int32_t dtype;
    int32_t ksplit;            /* gather kernel: > 1 splits the K loop over blockIdx.z (f32 atomics into
                                  splitk_ws [B*TH*TW][w_rows], then an epilogue launch); for small-M layers.
                                  Variant 19: the number of 32- or 64-channel K slices (cin_total / 32 or / 64, a multiple of 4) */
    float* splitk_ws;          /* must be ALL-ZERO on entry; the split-K epilogue leaves it all-zero again (no memset per launch).
                                  Variant 19 keeps its tile counters in the last 16 KiB (zero on entry, zero again on exit) */
    int64_t splitk_ws_bytes;
    int32_t variant;           /* kernel choice: 0 heuristic, 1 gather, 2/3 halo-patch with 128-/64-B K chunks,
                                  4 halo-patch single-stage, 5 single-stage double-buffered,
                                  6/7 = 3/4 on a 16x32-position block with 8 waves, 8/9 = 3/4 on a 4x32 block;
                                  10 weight-stationary persistent kernel (<= 128 B of input channels per pixel);
                                  11 / 12 gather with 32 / 64 output channels per workgroup (more workgroups for small layers);
                                  13 LDS-DMA double-buffered persistent kernel (16-bit operands, 16x32 positions x 64 channels per
                                  workgroup, sources at the launch size or exactly half of it);
                                  15 forward 3x3 stride-2 by LDS-DMA (parity-de-interleaved patch, 16-channel chunks);
                                  18 = `deconv` forward in sub-pixel form (one source at exactly half the launch size, weight_up2 set): four 2x2
                                  convolutions of the low-resolution map, 16 instead of 36 tap-MACs per output quad (conv_dma.hip);
                                  17 = 13 on 4x32-position tiles with four waves (one row each): small maps (levels 4-6) get 4x the workgroups;
                                  20 = 13 on 8x32-position tiles with eight waves (one row each): the 32x64 maps of level 3;
                                  16 = 10 with two groups of four waves half a period apart (one in its MFMAs while the other stores,
                                  loads and runs the epilogue), half-height tiles;
                                  19 = the deepest levels (maps of at most 128 positions, 128 % (TH TW) == 0; stride 1 or 2; nine taps; 16-bit):
                                  one-shot LDS-DMA of a 32- or 64-channel K slice per workgroup, `ksplit` = cin_total / 32 or / 64 slices,
                                  f32 partial tiles in `scratch`, summed IN SLICE ORDER (deterministic) with the epilogue by the slice that
                                  arrives last at the tile's counter (the last 16 KiB of splitk_ws) -- one launch (conv_dma.hip);
                                  21 = 13 re-cut for two resident workgroups per CU: 16x32 positions x 64 channels on FOUR waves of four rows
                                  each, 16-channel K chunks (2 x 38 KiB of LDS), NHWC outputs only -- the two waves of a SIMD belong to different
                                  workgroups, so one's epilogue / chunk barrier overlaps the other's MFMAs (conv_dma.hip: conv3x3_dma2_kernel);
                                  22 = the wave program of 21 on 32x32-position tiles, eight waves, one workgroup per CU (2 x 55 KiB of LDS): 27 % fewer
                                  staged bytes and 40 % fewer fragment reads per MFMA than 13;
                                  23 = 13 on v_mfma_f32_16x16x32 (a 32x32 tile as 2 x 2 MFMAs of K = 32): the MFMA shape the chip holds a higher clock on
                                  (conv_dma.hip: conv3x3_dma16_kernel); 24 / 25 = 17 / 20 in the same way (NHWC outputs, no fused pool);
                                  26 = data gradient of a `deconv` layer (nearest 2x upsampling + 3x3 convolution, FAL_netB.py:52-58) on the LOW-resolution
                                  grid: ONE source = the upstream gradient at exactly twice the output map, weight = falnet_pack_up2_t::wdd
                                  ([w_rows][4][4 C], w_taps = ntaps = 4, cin_total = 4 C) -- a 2x2-tap convolution over pairs of upstream rows /
                                  columns, 16 instead of 36 tap-MACs per input position (conv_dma.hip: conv2x2_up2d_dma16_kernel);
                                  27 = wave-streaming kernel for 32 -> (<= 32) channel layers (conv_wave.hip: conv3x3_wave32_kernel): ONE 32-channel
                                  source at the launch size, 32-row packed weight, NHWC output, no pool / split-K; every wave streams its own
                                  32-pixel strip rows through a private LDS-DMA ring (no workgroup barrier), weights resident in registers;
                                  29 = the same wave-streaming form for ONE 64-channel source and <= 4 output channels written as planar f32, no addend /
                                  activation-gradient operand (conv_wave.hip: conv3x3_wave64p_kernel: the data gradient of VGG19's first convolution);
                                  -2 is returned when the variant does not apply */
    void* pool_out;            /* optional fused 2x2/stride-2 reduction of the (activated) output: NHWC `dtype`
                                  [B][OH/2][OW/2][out_cstride].  pool_mode 0: max (nn.MaxPool2d(2,2) after the VGG slices,
                                  loss_functions.py:21-29); pool_mode 1: sum, then multiplied by d act / d pre taken from
                                  pool_actout (the adjoint of F.interpolate(scale 2, nearest) in front of a deconv,
                                  FAL_netB.py:58, fused into that conv's data-gradient launch).  Halo-patch variants with an
                                  even number of rows per wave only (-2 otherwise); with pool_out set, `out` may be NULL
                                  (only the reduced map is kept) */
    int32_t pool_mode;
    int32_t pool_actout_kind;  /* FALNET_ACT_* of pool_actout */
    const void* pool_actout;   /* NHWC like pool_out, or NULL */
    const void* weight_up2;    /* variant 18 only, else NULL: sub-pixel weights [CoutPad][16][CinTot] in `dtype` of a 3x3 convolution over a 2x
                                  nearest-upsampled source (falnet_pack_up2_batched): pair 4 (2 py + px) + 2 a + b holds the sum of the 3x3
                                  taps that fall on low-resolution neighbour (a, b) for output parity (py, px) */
    void* scratch;             /* variant 19 only, else NULL: uninitialised device scratch for the K-slice partial tiles,
                                  ksplit * ceil(B TH TW / 128 | 256) * 128 | 256 * w_rows f32; contents are meaningless between launches;
                                  launches that share it must be stream-ordered */
    int64_t scratch_bytes;
    void* pool_code;           /* optional, variant 23 with pool_out and pool_mode 0 in a 16-bit type only (-2 otherwise): one 4-bit argmax code per
                                  pooled element, [B][OH/2][OW/2][out_cstride / 2] bytes, channel c in byte c / 2 (low nibble: even c).  The code is
                                  one-hot: bit 2 * row + column of the window element that is the FIRST maximum in row-major order (strict >, on the
                                  values as rounded to `dtype`), 0 when the pooled value is not > 0 -- all that falnet_maxpool2_bwd_codes needs, so
                                  `out` may stay NULL on a gradient-carrying pass.  Private to these two entry points */
} falnet_conv_t;
int falnet_conv2d(const falnet_conv_t* p, void* stream); /* = falnet_conv2d_wgs(p, 0, stream) */
/* The same launch under a WORKGROUP BUDGET: max_workgroups = 0 is falnet_conv2d's grid; > 0 caps the total number of workgroups of a
 * PERSISTENT launch, so that it leaves compute units to launches on other streams (a full-grid persistent workgroup holds a whole CU's
 * registers: nothing co-resides).  With ny output-channel blocks the grid is gx x ny, gx = max(1, min(max_workgroups, full) / ny), clamped
 * to the number of tiles as before; full = 256 (512 for variant 21, two workgroups per CU).  Every persistent kernel strides its tile loop
 * by the grid width, so which workgroup computes a tile does not enter the arithmetic: the result is bit-identical for every budget.
 * Budgeted: the LDS-DMA variants 13 / 17 / 20, 21 / 22, 23 / 24 / 25, 15, 18, 26 and the weight-stationary variants 10 / 16.  A family that
 * is not persistent, or sums through f32 atomics or split-K (gather 1 / 11 / 12, halo-patch 2-9, 19, wave-streaming 27 / 29), accepts the
 * argument and ignores it; falnet_conv3x3_c3 is not a persistent launcher and takes none.  < 0: refused (-1) before anything is launched. */
int falnet_conv2d_wgs(const falnet_conv_t* p, int max_workgroups, void* stream);
/* Workgroups falnet_conv2d_wgs(p, max_workgroups, .) would launch (all grid dimensions multiplied; the split-K epilogue launch of the gather
 * kernel not counted): the same checks, kernel choice and grid arithmetic, no device call.  Negative: the error code, falnet_last_error() set. */
int falnet_conv2d_workgroups(const falnet_conv_t* p, int max_workgroups);
/* First layer: 3x3 / stride 1 / pad 1 convolution of a 3-channel planar f32 image (FAL_netB.py:99 conv0, VGG19 features[0];
 * loss_functions.py:21) with the f32 OIHW weights as they are -> NHWC `dtype` [B][H][W][Cout], Cout in {32, 64}, bias + act fused. */
int falnet_conv3x3_c3(const float* x_nchw, const float* w_oihw, const float* bias, void* out, int B, int H, int W, int Cout,
                      int act, int dtype, void* stream);
/* n <= 4 gather launches of one family (same dtype / Cout / packed rows / ksplit, NHWC output) in ONE grid: the four
 * output-parity classes of a stride-2 data gradient.  ksplit > 1: every member needs its OWN all-zero splitk_ws region
 * (B*TH*TW*w_rows floats, non-overlapping); one fused epilogue launch follows and leaves the regions zero. */
/* variant 14 in descs[0]: the members must be the four output-parity classes (0,0) (0,1) (1,0) (1,1) of ONE 3x3 / stride-2 / pad-1
 * data gradient in bf16 / f16 (same gout source, packed weight, output tensor; taps as fal_net_amd/ops.py:dgrad_taps_s2); they then
 * run as one LDS-DMA halo kernel (csrc/conv_dma.hip: conv3x3_s2d_dma_kernel) instead of four gather GEMMs. */
int falnet_conv2d_multi(const falnet_conv_t* descs, int n, void* stream); /* = falnet_conv2d_multi_wgs(descs, n, 0, stream) */
/* ... under a workgroup budget (falnet_conv2d_wgs): the persistent variant-14 kernel takes it, the gather form ignores it; < 0 is refused */
int falnet_conv2d_multi_wgs(const falnet_conv_t* descs, int n, int max_workgroups, void* stream);
/* symbol (as rocprofv3 reports it) of the kernel falnet_conv2d launches for this descriptor */
int falnet_conv2d_kernel_name(const falnet_conv_t* p, char* buf, int len);

/*
 * Weight gradient (autograd of the conv2d call sites above):
 *   dW[co, tap, ci] = sum_p gout[p, co] * in[nbr(p, tap), ci]
 * split over pixel ranges into `nsplit` f32 partial slabs in the caller's workspace
 * [nsplit][ntaps][CoutPad][CinTot], then falnet_wgrad_reduce sums the slabs into the
 * OIHW f32 gradient (+= when accumulate).  `gout` is NHWC [B][TH][TW][gC] (tile space = the
 * conv's output grid); sources/taps as in falnet_conv_t.
 */
typedef struct {
    falnet_src_t src[2];
    int32_t nsrc;
    int32_t IH, IW;
    const void* gout;
    int32_t gC;                /* padded channel count of gout (CoutPad) */
    int32_t ntaps;
    int32_t tap_dy[9], tap_dx[9];
    int32_t isy, isx;
    int32_t B, TH, TW;
    int32_t cin_total;
    int32_t nsplit;
    float* partial;            /* workspace */
    int32_t dtype;
    int32_t variant;           /* 0 heuristic (halo-patch kernel, 32x32 channels per workgroup, when dense 3x3 stride 1),
                                  1 force the per-tap kernel, 3 / 4 halo-patch with 32x64 / 64x32 (cin x cout) channels per
                                  workgroup (16-bit operands), 5 parity-plane halo kernel for 3x3 stride-2 launches (16-bit),
                                  6 first layer: src[0].ptr = planar f32 [B][3][IH][IW] image (src[0].C = 3), 16-bit gout with 32
                                  channels, cin_total 32 (slab layout),
                                  7 row-streaming kernel (bf16 / f16, dense 3x3 stride 1, sources at the launch size or exactly
                                  half of it): 64 x 64 channels per workgroup, LDS-DMA row ring, gout fragments in a rolling
                                  register window; nsplit = ranges of (sample, 32-pixel column strip, row) units,
                                  9 wave-streaming kernel (csrc/wgrad_wave.hip; bf16 / f16, dense 3x3, ONE 32-channel NHWC source at the input size):
                                  stride 1 with gC 32 or 64, or stride 2 (TH = ceil(IH / 2), TW = ceil(IW / 2)) with gC 64; nsplit = workgroups =
                                  slabs, every wave streams its own (sample, strip, row) range (stride 2: its own parity plane of one range).
                                  Variant 6 takes the same wave-streaming form when IW % 4 == 0 (not in deterministic mode): FALNET_WGK_C3WAVE */
    float* bias_grad;          /* optional, halo kernels (dense 3x3 stride 1, variant 5): db[co] += sum over positions of gout[.,co]
                                  (f32 atomics, [gC]) from the gout tiles the kernel stages anyway -- replaces a falnet_bias_grad
                                  pass over the same tensor.  Only the kernels falnet_wgrad_fuses_bias() reports fuse it;
                                  falnet_wgrad returns -3 when it is set for a launch whose kernel cannot */
    int32_t cout;              /* real output channels (<= gC): bound of the fused bias gradient (bias_grad holds `cout` floats);
                                  0 = gC */
    int32_t up2;               /* variant 7 only, else 0.  != 0: the weight gradient of a `deconv` layer (nearest 2x upsampling + 3x3 convolution,
                                  FAL_netB.py:52-58) on the LOW-resolution grid: `gout` is the upstream gradient at [B][2 TH][2 TW][gC], the one source
                                  the layer's input at TH x TW (= IH x IW); 16 instead of 36 tap products per low-resolution position, and every
                                  workgroup writes its share of the full 3x3 slab, so the slab reduce is unchanged.
                                  1: nsplit = 4 x pixel ranges (split = 4 range + 2 py + px): a split multiplies the gout pixels of ONE parity
                                  class with the 2 x 2 input offsets they meet; every class walks the whole grid (wgrad3x3_rows16_kernel<T,4,2,true>).
                                  2: nsplit = pixel ranges of (sample, 32-column strip, low-resolution row) units, any count >= 1: a row step
                                  carries two low-resolution rows and ALL FOUR parity classes of gout, a quarter of the high-resolution form's
                                  steps with the input fetched once (wgrad3x3_up2q_kernel<T,2>) */
} falnet_wgrad_t;
/* 1 when the kernel falnet_wgrad selects for this descriptor sums the bias gradient itself (bias_grad honoured), else 0 */
int falnet_wgrad_fuses_bias(const falnet_wgrad_t* p);
int64_t falnet_wgrad_workspace_bytes(const falnet_wgrad_t* p);
int falnet_wgrad(const falnet_wgrad_t* p, void* stream);
/* The kernels behind falnet_wgrad.  Which one a descriptor gets is decided in ONE place in the library; a host that sizes `nsplit` per kernel
 * asks falnet_wgrad_kernel_name and restates none of the applicability rules. */
enum {
    FALNET_WGK_TAP = 0,     /* per-tap kernel: any taps, stride and dtype (variants 0 / 1 / 3 / 4 where the launch is not dense 3x3 stride 1, TW >= 16) */
    FALNET_WGK_PATCH = 1,   /* halo-patch kernel, 32x32 (variant 0), 32x64 (3) or 64x32 (4) channels per workgroup */
    FALNET_WGK_S2 = 2,      /* parity-plane halo kernel (variant 5) */
    FALNET_WGK_C3 = 3,      /* first layer, halo-patch form (variant 6) */
    FALNET_WGK_C3WAVE = 4,  /* first layer, wave-streaming form (variant 6: IW % 4 == 0, TW >= 32, a 16-byte aligned image, not in deterministic mode) */
    FALNET_WGK_ROWS = 5,    /* row-streaming kernel and its two up2 forms (variant 7) */
    FALNET_WGK_ROWS_S2 = 6, /* row-streaming kernel, stride 2 (variant 8) */
    FALNET_WGK_WAVE = 7     /* wave-streaming kernel, stride 1 and stride 2 (variant 9) */
};
/* The kernel falnet_wgrad would launch for this descriptor: the same checks and the same choice, nothing issued, no pointer dereferenced (the
 * image pointer's alignment is read), `partial` and `bias_grad` not needed.  Returns the FALNET_WGK_* id (>= 0) and writes the mangled symbol
 * of the instantiation -- the name rocprofv3 reports -- into buf; a descriptor falnet_wgrad refuses gives a negative value and the same
 * falnet_last_error text. */
int falnet_wgrad_kernel_name(const falnet_wgrad_t* p, char* buf, int len);
/* partial [nsplit][ntaps][CoutPad][CinTot] -> grad OIHW f32 [Cout][Cin][kh][kw] (taps in kh*kw+kw order) */
/* channel groups as in falnet_pack_weights: packed column cp holds real channel cp (cp < c0_real) or
 * c0_real + (cp - c0_pad) */
int falnet_wgrad_reduce(const float* partial, int nsplit, int ntaps, int cout_pad, int cin_total,
                        float* grad, int cout, int cin, int c0_real, int c0_pad, int accumulate, void* stream);
/* db[co] (+)= sum_p g[p, co]; g NHWC [npix][gC], gC a multiple of 32 dividing 256 or a multiple of 256 */
int falnet_bias_grad(const void* g, int64_t npix, int gC, int cout, float* db,
                     int accumulate, int dtype, void* stream);

/* Batched forms: device-resident descriptor tables, ONE launch for all layers of a step.  The bias form ADDS into the
 * gradient buffers (f32 atomics), the reduce form as its `accumulate` argument says: the caller zeroes the flat gradient
 * buffer once per step (or keeps it to accumulate).
 * block_begin = first blockIdx.x of the entry; a reduce entry uses ceil(cout / cob) * groups blocks with
 * cob = max(1, 1024 / cin_total) output channels per block (falnet_wgrad_reduce_blocks; block -> (channel block, slab group);
 * groups == 1: plain read-modify-write of the gradient, else f32 atomics); ntaps in {1, 3, 9}; bias entry uses `blocks` blocks. */
int falnet_wgrad_reduce_blocks(int cout, int cin_total, int groups);
typedef struct {
    const float* partial; float* grad;
    int32_t nsplit, ntaps, w_rows, cin_total, cout, cin, c0_real, c0_pad, groups, block_begin;
} falnet_reduce_t;
typedef struct {
    const void* g; float* db; int64_t npix;
    int32_t gC, cout, blocks, block_begin;
} falnet_biasgrad_t;
typedef struct {
    const float* w; void* wf; void* wd;
    int32_t cout, cin, taps, c0_real, c0_pad, cin_pad, cout_pad, block_begin;  /* entry uses (cout_pad/32)*(cin_pad/32) blocks, taps 9, 3 or 1 */
    int32_t no_update, reserved;  /* falnet_adam_pack_batched: != 0 -> this entry is only packed (a derived weight, e.g. composed logits weights) */
} falnet_pack_t;
int falnet_pack_weights_batched(const falnet_pack_t* descs_dev, int n, int total_blocks, int dtype, void* stream);
/* The optimiser step of every packed layer AND its re-pack in one pass over the f32 masters (Train_Stage1_K.py:177-180 torch.optim.Adam; the
 * arithmetic of falnet_adam_step_dev): a block updates the 32 x 32 x taps master tile it is about to pack.  g_off / m_off / v_off: element
 * offsets from a master weight to its gradient and moments (the four flat buffers share one layout).  state = {lr, t} on the device (t is NOT
 * advanced: falnet_adam_tick); scaler: NULL, or the f16 loss-scale state {scale, ., overflow flag, .} -- the update divides by the scale and
 * is skipped as a whole when the flag is set.  Parameters outside the packed layers (biases, factors of composed weights): falnet_adam_ranges. */
int falnet_adam_pack_batched(const falnet_pack_t* descs_dev, int n, int total_blocks, int dtype, int64_t g_off, int64_t m_off, int64_t v_off,
                             const float* state, float b1, float b2, float eps, float grad_scale, const float* scaler, void* stream);
/* the same update over n_ranges element ranges (ranges_dev[2 r] = first element, [2 r + 1] = count) of the flat parameter buffer p */
int falnet_adam_ranges(float* p, int64_t g_off, int64_t m_off, int64_t v_off, const int64_t* ranges_dev, int n_ranges, const float* state,
                       float b1, float b2, float eps, float grad_scale, const float* scaler, void* stream);
/* t += 1 unless the scaler's overflow flag is set (a skipped step does not count) */
int falnet_adam_tick(float* state, const float* scaler, void* stream);
/* Weight decay / bias decay (torch.optim.Adam's L2 form, not AdamW: the two param groups of Train_Stage1_K.py:177-180).  With gr the gradient
 * after grad_scale and the f16 loss-scale division: gr += decay * p, then the moments and the step of the functions above; a raised overflow
 * flag skips the update AND the decay.  The 16-B padding elements between parameter slices (p = g = 0) stay exactly 0.  The decays are
 * DOUBLES and gr is rounded to f32 once: where g and decay * p cancel, an f32 sum would put the young-moment step outside an f64 reference's reach.
 * falnet_adam_pack_batched_wd: falnet_adam_pack_batched with ONE decay for the launch -- every packed layer is a convolution weight;
 *   no_update entries are only packed.
 * falnet_adam_ranges_wd: falnet_adam_ranges with decays_dev[r] (f64) the decay of range r; a range must not span two parameters of
 *   different decay.  Neither advances t (falnet_adam_tick). */
int falnet_adam_pack_batched_wd(const falnet_pack_t* descs_dev, int n, int total_blocks, int dtype, int64_t g_off, int64_t m_off, int64_t v_off,
                                const float* state, float b1, float b2, float eps, float grad_scale, double weight_decay, const float* scaler,
                                void* stream);
int falnet_adam_ranges_wd(float* p, int64_t g_off, int64_t m_off, int64_t v_off, const int64_t* ranges_dev, const double* decays_dev, int n_ranges,
                          const float* state, float b1, float b2, float eps, float grad_scale, const float* scaler, void* stream);
/* Sub-pixel weights of the `deconv` layers (falnet_conv_t::weight_up2; FAL_netB.py:52-58), all layers in one launch: entry i sums the f32 OIHW
 * 3x3 master weights w into wu [cout_pad][16][cin_pad] (`dtype`; pair index 4 (2 py + px) + 2 a + b, rows / columns: py = 0 -> (W[0], W[1] + W[2]),
 * py = 1 -> (W[0] + W[1], W[2])); an entry uses (cout_pad / 32) * (cin_pad / 32) blocks from block_begin. */
typedef struct {
    const float* w; void* wu;
    int32_t cout, cin, cin_pad, cout_pad, block_begin;
    int32_t reserved;
    void* wdd;  /* NULL, or [cin_pad][4][4 cout_pad]: the layer's data-gradient weights on the low-resolution grid (falnet_conv2d variant 26):
                 * wdd[ci][2 du + dv][e 2 cout_pad + f cout_pad + co] = sum of the 3x3 taps that carry upstream pixel (2 (i + du) - 1 + e,
                 * 2 (j + dv) - 1 + f) into input position (i, j); per axis t = 2 d + parity selects taps {2}, {1, 2}, {0, 1}, {0} */
} falnet_pack_up2_t;
int falnet_pack_up2_batched(const falnet_pack_up2_t* descs_dev, int n, int total_blocks, int dtype, void* stream);
/* accumulate == 0: entries with groups == 1 OVERWRITE their gradient (plain stores), entries with groups > 1 add into it
 * (atomics: the caller zeroes those); accumulate != 0: every entry adds.
 * Limits of the three batched entry points below: at most 64 entries per launch (n > 64 is refused before anything is launched: the
 * kernels stage the block_begin column of the table in a 64-int LDS array; fal_net_amd.ops.WgradBatch cuts longer tables into several
 * launches).  The tables live in DEVICE memory, so the library cannot check their fields: a falnet_biasgrad_t entry must have gC a
 * multiple of 32 with gC <= 2048 (beyond that the kernel's channel-segment loop reaches a workgroup barrier with some threads missing
 * when gC / 8 is not a multiple of 256) and cout <= 512 (the deterministic form's workspace has 512 columns per block; its finishing
 * kernel has 512 threads); a falnet_reduce_t entry has ntaps in {1, 3, 9}, cin_total a multiple of 32, 1 <= groups <= nsplit. */
int falnet_wgrad_reduce_batched(const falnet_reduce_t* descs_dev, int n, int total_blocks, int accumulate, void* stream);
int falnet_bias_grad_batched(const falnet_biasgrad_t* descs_dev, int n, int total_blocks, int dtype, void* stream);
/* the same sums without atomics: every block stores its partial sums to ws[block][512] (ws_floats >= 512 * total_blocks, channels
 * <= 512), a second launch adds them to db in block order */
int falnet_bias_grad_batched_det(const falnet_biasgrad_t* descs_dev, int n, int total_blocks, int dtype, float* ws, int64_t ws_floats,
                                 void* stream);

/*
 * OIHW f32 master weights -> packed compute-dtype operands.
 *   fwd  : wf[co][tap][ci]  (CoutPad x taps x CinPad), channel groups padded per source:
 *          real input channels [0,c0) go to [0,c0), [c0,Cin) to [c0pad, ...)  (concat sources)
 *   dgrad: wd[ci][tap][co]  (CinPad' x taps x CoutPad) -- the same numbers, transposed
 */
int falnet_pack_weights(const float* w_oihw, int cout, int cin, int taps,
                        int c0_real, int c0_pad, int cin_pad_total, int cout_pad,
                        void* wf, void* wd, int dtype, void* stream);

/* planar NCHW f32 [B][C][H][W] -> NHWC `dtype` [B][H][W][Cpad] (zero padded).  Boundary of the
 * reference API: input image (FAL_netB.py:200), VGG input (loss_functions.py:36), MED-head grads. */
int falnet_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int Cpad,
                        int dtype, void* stream);
/* NHWC `dtype` [B][H][W][Cpad] -> planar NCHW f32 [B][C][H][W] (first C channels) */
int falnet_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int Cpad,
                        int dtype, void* stream);
/* Adjoint of the fused nearest upsample (F.interpolate backward, FAL_netB.py:58):
 * gsrc[b, sy, sx, c] = (sum over virtual pixels mapping to (sy,sx) of gup[b, vy, vx, c]) * elu'(actout) */
int falnet_upsample_bwd(const void* gup, void* gsrc, const void* actout, int B, int IH, int IW,
                        int H, int W, int C, int dtype, void* stream);
/* Weight gradient of a 3x3 pad-1 conv (stride 1 or 2) with respect to an input plane that is CONSTANT per sample -- the `flow` input of
 * conv1 (FAL_netB.py:208-209, :101): dW[co][ky][kx] += sum_b plane[b * plane_stride] * sum over the output pixels whose tap (ky,kx) is in
 * bounds of gout[b][i][j][co].  gout NHWC `dtype` [B][TH][TW][gC]; grad = &dW_oihw[0][ci][0][0] of the f32 gradient, grad_co_stride = Cin * 9;
 * ws: B * 9 * gC floats, ZERO on entry and left zero.  Adds with f32 atomics (refused in deterministic mode). */
int falnet_wgrad_const_plane(const void* gout, const void* plane, int64_t plane_stride, float* grad, int64_t grad_co_stride, float* ws,
                             int B, int TH, int TW, int gC, int cout, int IH, int IW, int stride, int dtype, void* stream);
/* 2x2/2 max pool on NHWC (torchvision VGG19 features[4,9,18]; loss_functions.py:21-29) and its adjoint */
int falnet_maxpool2_fwd(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
int falnet_maxpool2_bwd(const void* x, const void* y, const void* gy, void* gx, int B, int H, int W, int C,
                        int dtype, void* stream);
/* maxpool2_bwd_codes: the same gradient from the argmax codes a fused pool wrote (falnet_conv_t::pool_code, [B][H/2][W/2][C/2] bytes) instead of
 * the pool input: every element of gx [B][H][W][C] is written, gy where the window's code selects it and zero elsewhere.  H, W even,
 * C % 8 == 0, gy / gx 16-B aligned (-1 otherwise: there is no scalar form). */
int falnet_maxpool2_bwd_codes(const void* codes, const void* gy, void* gx, int B, int H, int W, int C, int dtype, void* stream);
/* maxpool2_bwd: x is the (ReLU) pool input; the gradient goes to the first maximum of each window
 * (aten tie rule) and is zero where that maximum is 0 (fused relu'); H, W even. */
/* gx = g * act'(y) elementwise on NHWC, act' from the activation OUTPUT y (ELU: y>0?1:y+1) */
int falnet_act_bwd(const void* g, const void* y, void* gx, int64_t n, int kind, int dtype, void* stream);

/*
 * MED head (FAL_netB.py:216-282): per-pixel softmax over the N disparity planes, expectation ->
 * disp; plane-sweep warp of the logits by d_n (W-1)/W pixels (2-tap, zero padded), second softmax,
 * blend of the equally shifted left image -> p_im0.  All planar f32.
 *   dlog0 [B][N][H][W], left [B][3][H][W], min_disp/max_disp [B]
 *   disp [B][1][H][W] (or NULL), p_im0 [B][3][H][W] (or NULL)
 *   stats [B][4][H][W]: (max0, sum0, maxW, sumW) of the two softmaxes, kept for backward (or NULL)
 */
int falnet_med_head_fwd(const float* dlog0, const float* left, const float* min_disp, const float* max_disp,
                        float* disp, float* p_im0, float* stats, int B, int N, int H, int W, void* stream);
/* grad_dlog0 [B][N][H][W] from grad_disp / grad_p_im0 (either may be NULL) */
int falnet_med_head_bwd(const float* dlog0, const float* left, const float* min_disp, const float* max_disp,
                        const float* disp, const float* p_im0, const float* stats,
                        const float* grad_disp, const float* grad_p_im0, float* grad_dlog0,
                        int B, int N, int H, int W, void* stream);
/* the same gradient written pixel-major in the conv stack's layout: `dtype` NHWC [B][H][W][cpad], channels >= N zero
 * (cpad % 8 == 0) -- feeds the 1x1 logits conv's data / weight gradient launches without a planar round trip */
int falnet_med_head_bwd_nhwc(const float* dlog0, const float* left, const float* min_disp, const float* max_disp,
                             const float* disp, const float* p_im0, const float* stats,
                             const float* grad_disp, const float* grad_p_im0, void* grad_dlog0_nhwc, int cpad, int dtype,
                             int B, int N, int H, int W, void* stream);
/* Name of the kernel the three head entry points dispatch to for a shape (tests assert that every form is covered; same predicates as
 * the launches, 16-byte aligned operands assumed).  pass: 0 = falnet_med_head_fwd, 1 = falnet_med_head_bwd, 2 = falnet_med_head_bwd_nhwc. */
int falnet_med_head_kernel_name(int pass, int dtype, int N, int W, char* buf, int len);
/* occlusion masks (FAL_netB.py:264-273,291-292), no grad: maskR = min(1, sum_n shift_{+s_n}(softmax(dlog0)_n)),
 * maskL = min(1, sum_n shift_{-s_n}(Dprob_n)).  Dprob is rebuilt from the logits and `stats`. */
int falnet_med_masks_fwd(const float* dlog0, const float* min_disp, const float* max_disp, const float* stats,
                         float* maskL, float* maskR, int B, int N, int H, int W, void* stream);
/* FAL_netA's right mask (models/FAL_netA.py:264): the same sum, but each plane is sampled with grid_sample's default
 * align_corners=False on the align_corners=True grid (:231,:241-242) -- bilinear in x AND y at
 * (x W/(W-1) + d_n - 1/2, y H/(H-1) - 1/2), zero padding.  Overwrites maskR; `stats` from falnet_med_head_fwd. */
int falnet_med_maskr_acfalse_fwd(const float* dlog0, const float* min_disp, const float* max_disp, const float* stats,
                                 float* maskR, int B, int N, int H, int W, void* stream);

/* Views and disparities along the baseline from the logits of one forward (inference only: no gradient, no statistics).  View v shifts
 * plane n by t[v] * d_n (W-1)/W pixels (2-tap, zero padded on BOTH sides), takes the softmax over the shifted logits and blends the
 * equally shifted left image; disps is sum_n d_n P_n in the view's own frame, in full-baseline pixels (not scaled by t).  t = 1 is
 * falnet_med_head_fwd's p_im0 (and the reference's commented-out `dispr`), t = 0 gives back `left` and `disp`, t < 0 renders to the other
 * side of the left camera.  All planar f32; one launch reads each logit row once for its V views.
 *   t_host: HOST array of V baseline fractions, 1 <= V <= 8, each finite with |t| <= 2 (passed to the kernel by value)
 *   views [B][V][3][H][W] (or NULL), disps [B][V][1][H][W] (or NULL); at least one of them.  `left` may be NULL when views is.
 * Returns non-zero and launches nothing on a refused argument (sizes: those falnet_med_head_fwd accepts). */
int falnet_med_sweep_fwd(const float* dlog0, const float* left, const float* min_disp, const float* max_disp,
                         const float* t_host, int V, float* views, float* disps, int B, int N, int H, int W, void* stream);

/* Free-viewpoint rendering of the logits of one forward: a homography plane sweep (csrc/med_pose.hip; inference only: no gradient, not
 * replayable -- falnet_replay_op_index: -1).  Plane n is the plane Z = fx b / s_n of the left camera, s_n = d_n (W-1)/W (the head's and the
 * sweep's table, built on the device from min_disp / max_disp).  A target camera with centre c (source-camera coordinates), rotation R
 * (X_t = R (X_s - c)) and intrinsics K_t travels as 12 doubles:
 *   A = K R^T K_t^-1   (3 x 3, row-major: target pixel -> ray direction in source pixel coordinates)     E = K c / (fx b)   (3)
 * For target pixel (x, y): q = A (x, y, 1), u0 = q_x / q_z, v0 = q_y / q_z; plane n is sampled at
 *   u_n = s_n E_x + w_n u0,  v_n = s_n E_y + w_n v0,  w_n = 1 - s_n E_z      iff q_z > 0 and w_n > 0,
 * bilinearly over four taps that read 0 outside [0, H-1] x [0, W-1] (logits and image alike); a plane that is not sampled, or whose taps all
 * fall outside, takes part in the softmax with logit 0 (not -inf), as in the head and the sweep.  With P_n the softmax of the warped logits:
 *   views [B][V][3][H][W] = sum_n P_n bilinear(left_c, u_n, v_n)
 *   disps [B][V][1][H][W] = sum_n d_n P_n                       (full-baseline pixels of the source planes, as the sweep's disps)
 *   cover [B][V][1][H][W] = sum_n P_n omega_n   in [0, 1]       (omega_n: the bilinear weights of the taps inside the image, 0 when not sampled)
 * Any of the three may be NULL, not all; `left` may be NULL when views is.  A = I, E = (t, 0, 0) is falnet_med_sweep_fwd's view t.
 *   pose_host: HOST array of V records of 12 doubles (A then E), 1 <= V <= 8, passed to the kernel by value.
 * Coordinates are formed in f64 and clamped as floating values into [-2, W+1] x [-2, H+1] before they become integers; no atomics: two
 * launches give the same bits.  Returns non-zero, launches nothing and writes nothing on a refused argument: a null required pointer, all
 * three outputs NULL, V outside 1..8, a non-finite entry of a record, a record whose third row of A is all zero, sizes other than those
 * falnet_med_head_fwd accepts (and a plane of more than 2^30 pixels: in-plane byte offsets are 32-bit). */
int falnet_med_pose_fwd(const float* dlog0, const float* left, const float* min_disp, const float* max_disp,
                        const double* pose_host, int V, float* views, float* disps, float* cover,
                        int B, int N, int H, int W, void* stream);

/* Hole filling of a premultiplied image: background-biased pull-push (csrc/inpaint.hip; inference only: no gradient, not replayable --
 * falnet_replay_op_index: -1).  Made for falnet_med_pose_fwd's outputs (values = views, a colour premultiplied by its weight; weight = cover;
 * guide = disps), but any premultiplied image will do.  Per image, all planar f32:
 *   values [I][C][H][W] premultiplied, 1 <= C <= 4; weight [I][1][H][W] in [0, 1]; guide [I][1][H][W] and guide_scale [I] (device, positive),
 *   both optional; beta in [0, 8]; floor in (0, 1] (2^-10 is the usual one); out [I][C][H][W]: the un-premultiplied, fully weighted image.
 * Level 0:  keep = weight >= floor;  w0 = keep ? weight : 0,  c0 = keep ? values : 0  (selects, not multiplies: a NaN under a dropped pixel
 *   does not leak);  g = exp(-beta guide / guide_scale), g = 1 when beta = 0 (guide is never read then);  the stored triple is
 *   (cg, wg, a) = (c0 g, w0 g, w0).
 * Pull, level l -> l + 1, sizes H_{l+1} = (H_l + 1) / 2 and the same for W, until 1 x 1 (L = falnet_inpaint_levels pulls): each coarse cell
 *   sums its existing fine cells (2 x 2, fewer at odd ends) of all C + 2 channels, then all C + 2 channels are multiplied by 1 / a_sum where
 *   a_sum > 1, so a <= 1.
 * Apex:  div(n, d) = d > 0 ? n / d : 0;  F_L = div(cg_L, wg_L),  G_L = div(wg_L, a_L).
 * Push, level l + 1 -> l.  up() is the 2x tent filter: even fine index i takes coarse taps i/2 - 1 and i/2 with weights 1/4 and 3/4, odd i
 *   takes (i-1)/2 and (i-1)/2 + 1 with 3/4 and 1/4; taps are clamped into the coarse level; x and y are separable.
 *   UG = up(G_{l+1}),  U = div(up(F_{l+1} G_{l+1}), UG);
 *   l >= 1:  F_l = a_l div(cg_l, wg_l) + (1 - a_l) U,   G_l = a_l div(wg_l, a_l) + (1 - a_l) UG;
 *   l = 0:   out = c0 + (1 - w0) U;        L = 0 (a 1 x 1 image):  out = c0 + (1 - w0) F_0.
 * The bias towards small `guide` (the background, when guide is a disparity) travels through both directions: in the pull as the factor g of
 * every sum, in the push as G, the mean g of what a cell holds, which weights the coarse taps.  Pixels with weight == 1 come back bit for bit.
 * No atomics and every sum in a fixed order: two calls give the same bits and image i of a batch equals its one-image call.
 *   falnet_inpaint_levels(H, W): L (-1 on a refused size).
 *   falnet_inpaint_workspace_bytes(C, H, W, images): the caller-provided workspace (levels 1..L of C + 2 channels; the push keeps its
 *   results in them), -1 on a refused argument; nothing is allocated inside a launch function.  The workspace belongs to one stream at a time.
 * falnet_inpaint_fwd returns non-zero, launches nothing and writes nothing on a refused argument: a null required pointer (values, weight,
 * out; the workspace where its size is not 0), guide or guide_scale null with beta > 0, out overlapping values, C outside 1..4, I, H or W below
 * 1, a plane above 2^30 pixels, beta not in [0, 8] or not finite, floor not in (0, 1], a workspace smaller than reported. */
int falnet_inpaint_levels(int H, int W);
int64_t falnet_inpaint_workspace_bytes(int C, int H, int W, int images);
int falnet_inpaint_fwd(const float* values, const float* weight, const float* guide, const float* guide_scale, float beta, float floor,
                       float* out, void* workspace, int64_t workspace_bytes, int I, int C, int H, int W, void* stream);

/* Per-pixel statistics of the head's distribution over the N planes (csrc/med_stats.hip; inference only: no gradient, not replayable --
 * falnet_replay_op_index: -1).  p_n = softmax_n dlog0, d_n = the head's plane table, a = the FIRST index of the largest stored logit (an exact
 * comparison), win = {n : |n - a| <= 1} within [0, N-1].  `which` selects the outputs by bit; they are written densely as out[B][K][H][W]
 * (K = number of set bits), planar f32, in bit order:
 *   bit 0 mean    sum p_n d_n                              (falnet_med_head_fwd's disp)
 *   bit 1 std     sqrt(sum p_n (d_n - mean)^2), pixels     (from the centred sum)
 *   bit 2 entropy -sum p_n ln p_n / ln N, in [0, 1]
 *   bit 3 arg     a, an exact small integer
 *   bit 4 conf    sum_win p_n, in (0, 1]
 *   bit 5 peak    sum_win p_n d_n / sum_win p_n, pixels
 * One launch for any subset; every logit is read once; no atomics, bit-identical from run to run.  Returns non-zero and writes nothing on a
 * refused argument: which == 0 or a bit above 5, a NULL pointer, N outside [2, 128], a non-positive size (sizes: those falnet_med_head_fwd accepts). */
#define FALNET_STAT_MEAN 1u
#define FALNET_STAT_STD 2u
#define FALNET_STAT_ENTROPY 4u
#define FALNET_STAT_ARG 8u
#define FALNET_STAT_CONF 16u
#define FALNET_STAT_PEAK 32u
int falnet_med_stats_fwd(const float* dlog0, const float* min_disp, const float* max_disp, unsigned which, float* out, int B, int N, int H, int W,
                         void* stream);

/* Ordered stream compaction (csrc/compact.hip; not replayable): record i of `src` (n records of rec_bytes bytes each) is kept when
 * score[i] >= threshold -- a NaN score is dropped -- and the kept records are written to dst in index order; count_dev[0] receives their number.
 * Per-workgroup counts, one exclusive scan, one scatter: no atomics, the result is the same bytes on every run; dst beyond the kept records is
 * not written.  rec_bytes: 4 (a row of the planar point cloud; src and dst 4-byte aligned) or 15 (packed PLY vertex records, unaligned); anything
 * else, n < 1 and a NULL pointer are refused with nothing written.  workspace: falnet_compact_workspace_bytes(n) bytes, 8-byte aligned as count_dev,
 * owned by one stream at a time. */
int64_t falnet_compact_workspace_bytes(int64_t n);
int falnet_compact_records(const void* src, int rec_bytes, const float* score, float threshold, int64_t n, void* dst, int64_t* count_dev,
                           void* workspace, void* stream);

/* ---- losses (loss_functions.py) ; all write/accumulate a scalar in `out` (f32, device) ---- */
/* out[0] (+)= scale * sum(mask * |a - b|) ; mask NULL or [B][1][H][W] broadcast over C (loss_functions.py:53) */
int falnet_l1_fwd(const float* a, const float* b, const float* mask, int B, int C, int64_t HW,
                  float scale, float* out, int accumulate, void* stream);
/* ga (+)= gscale[0] * scale * mask * sign(a - b) */
int falnet_l1_bwd(const float* a, const float* b, const float* mask, int B, int C, int64_t HW,
                  float scale, const float* gscale, float* ga, int accumulate, void* stream);
/* perceptual term: out[0] (+)= scale * sum over real channels of (a-b)^2 on NHWC `dtype` (loss_functions.py:61-65) */
int falnet_mse_fwd(const void* a, const void* b, int64_t npix, int Cpad, float scale, float* out,
                   int accumulate, int dtype, void* stream);
/* ga = gscale[0] * 2 * scale * (a - b) */
int falnet_mse_bwd(const void* a, const void* b, int64_t npix, int Cpad, float scale, const float* gscale,
                   void* ga, int dtype, void* stream);
/* edge-aware smoothness on the column window [x0, x1) (loss_functions.py:70-101; crop at
 * Train_Stage1_K.py:255): out[0] (+)= scale * sum(...). img [B][3][H][W], disp [B][1][H][W] planar f32 */
int falnet_smooth_fwd(const float* img, const float* disp, int B, int H, int W, int x0, int x1,
                      float gamma, float scale, float* out, int accumulate, void* stream);
int falnet_smooth_bwd(const float* img, const float* disp, int B, int H, int W, int x0, int x1,
                      float gamma, float scale, const float* gscale, float* gdisp, int accumulate, void* stream);
/* Loss AND gradient in one pass over the operands (a training step that knows its upstream scalars before the forward runs:
 * fal_net_amd/train.py:_stage1_fused): out[0] += the loss term exactly as the *_fwd entry point with accumulate = 1 adds it; the
 * gradient exactly as the *_bwd entry point writes it (assigned, not accumulated). */
int falnet_l1_fwd_bwd(const float* a, const float* b, int B, int C, int64_t HW, float scale, float* out, const float* gscale, float* ga,
                      void* stream);
/* falnet_l1_fwd_bwd with another gradient of the same tensor added in the same pass: ga = gscale * scale * sign(a - b) + gadd (gadd may not
 * alias ga) -- the perceptual (VGG) gradient of the synthesised view joins the L1 gradient without an extra add launch */
int falnet_l1_fwd_bwd_add(const float* a, const float* b, int B, int C, int64_t HW, float scale, float* out, const float* gscale,
                          const float* gadd, float* ga, void* stream);
int falnet_mse_fwd_bwd(const void* a, const void* b, int64_t npix, int Cpad, float scale_out, float* out, float scale_grad,
                       const float* gscale, void* ga, int dtype, void* stream);
/* Three falnet_mse_fwd_bwd in ONE launch (the perceptual term's three VGG slices, loss_functions.py:61-65): tensor k has numel[k] elements (a multiple
 * of 8, pointers 32-B aligned), out += scale_out[k] * sum (a_k - b_k)^2, ga_k = gscale[0] * 2 * scale_grad[k] * (a_k - b_k).  The pointer / scalar
 * arrays are HOST arrays of three entries (read at the call). */
int falnet_mse3_fwd_bwd(const void* const* a, const void* const* b, const int64_t* numel, const float* scale_out, float* out,
                        const float* scale_grad, const float* gscale, void* const* ga, int dtype, void* stream);
int falnet_smooth_fwd_bwd(const float* img, const float* disp, int B, int H, int W, int x0, int x1, float gamma, float scale, float* out,
                          const float* gscale, float* gdisp, void* stream);
/* Tail of a fused step (Train_Stage1_K.py:258 `loss = rec_loss + a_sm * sm_loss`): S = {rec, sm} as accumulated by the *_fwd_bwd entry
 * points above -> out = {rec + a * sm, rec, sm}; S is left {0, 0} for the next step. */
int falnet_step_scalars(float* S, float a, float* out, void* stream);
/* mixing for masked perceptual input: out = m*a + (1-m)*b (loss_functions.py:55); and grad wrt a: ga = m*g */
int falnet_mask_mix(const float* a, const float* b, const float* m, float* out, int B, int C, int64_t HW, void* stream);

/* Fused flat-buffer Adam (torch.optim.Adam semantics, Train_Stage1_K.py:180): p, g, m, v f32 [n];
 * step_size = lr / (1 - b1^t), bias2 = sqrt(1 - b2^t) computed by the caller. */
int falnet_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                     float eps, int step, float grad_scale, void* stream);

/* Same update with the hyper-state on the device: state = {lr, t} (f32).  The kernel uses t+1 and a one-thread
 * launch then advances t, so a captured hipGraph replays correctly.  n must be a multiple of 4. */
int falnet_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float* state, float b1, float b2,
                         float eps, float grad_scale, void* stream);

/* Dynamic loss scale of the f16 compute path (torch.cuda.amp.GradScaler semantics; the reference is f32-only, Train_Stage1_K.py:258-262
 * `loss.backward(); optimizer.step()`), device-resident so that no step synchronises with the host:
 *   scaler = {scale, clean steps since the last change, overflow flag, skipped steps} (f32[4], caller-initialised {S0, 0, 0, 0}).
 * falnet_grad_guard: scaler[2] = 1 when any of g[0, n) is inf / NaN (run AFTER the gradient all-reduce: every rank sees the same sum).
 * falnet_adam_step_guarded: falnet_adam_step_dev with gradients multiplied by grad_scale / scaler[0]; when scaler[2] != 0 the whole
 *   update (p, m, v, step count) is skipped.
 * falnet_loss_scale_update (after Adam): overflow -> scale = max(scale * backoff, min_scale), skipped++; else clean++ and scale =
 *   min(scale * growth, max_scale) every `interval` clean steps; clears the flag.
 * falnet_loss_seeds: seeds[i] = scaler[0] * coef[i] -- the upstream-gradient scalars (`gscale`) of the loss kernels above. */
int falnet_grad_guard(const float* g, int64_t n, float* scaler, void* stream);
int falnet_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, float* state, float b1, float b2,
                             float eps, float grad_scale, const float* scaler, void* stream);
/* falnet_adam_step_dev / _guarded (scaler NULL / not NULL) with a decay per SEGMENT of the flat buffer: seg_end_dev[s] (int64) = exclusive end
 * element of segment s, ascending, multiples of 4 (parameter slices are 16-B aligned), the last one >= n; seg_decay_dev[s] (f64) its decay;
 * 1 <= n_seg <= 1024.  Same float4 streaming pass; advances t like they do. */
int falnet_adam_step_wd(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end_dev, const double* seg_decay_dev, int n_seg,
                        float* state, float b1, float b2, float eps, float grad_scale, const float* scaler, void* stream);
int falnet_loss_scale_update(float* scaler, float growth, float backoff, int interval, float min_scale, float max_scale, void* stream);
int falnet_loss_seeds(const float* scaler, const float* coef, float* seeds, int n, void* stream);

/* Stage-2 occlusion mask (Train_Stage2_K.py:296-302): out = a * b, forced to 1 in the column window [x0, x1); planar f32
 * [B][1][H][W], no gradient */
int falnet_occlusion_mask(const float* a, const float* b, float* out, int B, int H, int W, int x0, int x1, void* stream);
/* mirror-loss weight (Train_Stage2_K.py:319-324): out = (1 - occ) / rowmax[b] inside [x0, x1), 0 outside; with it the mirror
 * loss is falnet_l1_fwd(disp, teacher_disp, mask = out, scale = 1 / (B H (x1 - x0))) */
int falnet_mirror_weight(const float* occ, const float* rowmax, float* out, int B, int H, int W, int x0, int x1, void* stream);
/* horizontal flip of planar f32 [n_rows][W] (Train_Stage2_K.py:248-253 flip grid) */
int falnet_hflip(const float* src, float* dst, int64_t n_rows, int W, void* stream);
/* per-sample max of planar f32 [B][n] -> out[B]  (F.max_pool2d(kernel=(H,W)), Train_Stage2_K.py:319) */
int falnet_rowmax(const float* src, float* out, int B, int64_t n, void* stream);

/* Small f32 matrix product C (+)= A B with element strides (A[m * sam + k * sak], B[k * sbk + n * sbn], C row-major M x N):
 * the composed logits conv Wc = W1x1 . W3x3 (FAL_netB.py:127,190; once per weight update) and the split of its gradient,
 * dW3x3 = W1x1^T dWc, dW1x1 = dWc W3x3^T.  M * N * K <= 2^32. */
int falnet_gemm_f32_small(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C,
                          int M, int N, int K, int accumulate, void* stream);
/* Resampling of planar f32 maps [planes][H][W] -> [planes][OH][OW] times `scale` (Test_KITTI.py:287-300 ms_pp): bilinear != 0 ->
 * F.interpolate(mode='bilinear', align_corners=True), else mode='nearest' */
int falnet_resize_planar(const float* src, float* dst, int64_t planes, int H, int W, int OH, int OW, int bilinear, float scale,
                         void* stream);

/* Per-sample scalars of one step in one launch (Train_Stage1_K.py:237, FAL_netB.py:208-209): max_out = max_disp, min_out = min_disp
 * (or max_disp * mul / div when min_disp is NULL), flow[b * flow_stride] = max_disp / 100 in `dtype` (the constant input plane). */
int falnet_disp_prologue(const float* max_disp, const float* min_disp, float mul, float div, float* min_out, float* max_out,
                         void* flow, int flow_stride, int B, int dtype, void* stream);

/* ---- training-data augmentation (data_transforms.py:46-157, Train_Stage1_K.py:116-128) ---- */
/* One pass of Pillow's 8-bit bicubic resampling (Image.resize(size, BICUBIC), data_transforms.py:68) over an interleaved uint8
 * image [H][W][C]: along x (horizontal != 0: dst [H][out_size][C]) or along y (dst [out_size][W][C]).  bounds [out_size][2] =
 * (first source index, tap count), kk [out_size][ksize] = 22-bit fixed-point coefficients (host side:
 * fal_net_amd.data_transforms.resample_coeffs, the precompute_coeffs of Pillow's Resample.c).  Bit-exact with Pillow. */
int falnet_resample_u8(const uint8_t* src, uint8_t* dst, int H, int W, int C, int out_size, int horizontal,
                       const int32_t* bounds, const int32_t* kk, int ksize, void* stream);
/* crop [y1,y1+th) x [x1,x1+tw) of a uint8 [H][W][3] image, optional np.fliplr, RandomGamma / RandomBrightness /
 * RandomCBrightness with the given factors (<= 0: not applied; float64 arithmetic as numpy), ArrayToTensor, Normalize(0,255),
 * Normalize(mean,1) -> planar f32 [3][th][tw] */
int falnet_augment_normalize(const uint8_t* src, int H, int W, int x1, int y1, int th, int tw, int flip, double gamma,
                             double bright, double cb0, double cb1, double cb2, float mean0, float mean1, float mean2,
                             float* dst, void* stream);

/* The whole chain above for a BATCH in one launch (csrc/augment_batch.hip): per sample, both views -- bicubic resize of the uint8
 * [H][W][3] frame to rw x rh restricted to the crop window [y1,y1+th) x [x1,x1+tw) (Pillow's two-pass order and rounding, so bit-exact
 * with falnet_resample_u8 x2 + crop), optional mirror, the colour chain and both Normalize steps of falnet_augment_normalize -> planar f32
 * out0 / out1 [B][3][th][tw].  The resampling coefficients are computed on the device in f64, in the order of
 * fal_net_amd.data_transforms.resample_coeffs; there are no per-sample host arrays.
 * One record per sample: src[j] is the ADDRESS of the frame that feeds output position j (after the flip-swap of the views), cb[j] the
 * per-channel brightness factors of position j; gamma / bright / cb[j][0] <= 0: transform not applied.
 * Supported scale factors, per axis: 1 / FALNET_AUG_MAX_SCALE <= resized / source <= FALNET_AUG_MAX_SCALE, i.e. [0.5, 2.0] (at most 9
 * taps; the reference draws from [0.75, 1.5]: at most 7).  table_dev is the record table in device memory (read by the kernel),
 * table_host the same B records in host memory (checked before the launch): a size outside that range, a crop outside the resized image,
 * a null operand or a source address that is not device memory is refused (falnet_last_error); there is no fallback. */
#define FALNET_AUG_MAX_SCALE 2
typedef struct {
    uint64_t src[2];
    int32_t H, W, rw, rh, x1, y1, flip, reserved;
    double gamma, bright, cb[2][3];
} falnet_aug_t;
int falnet_augment_batch(const falnet_aug_t* table_dev, const falnet_aug_t* table_host, int B, int th, int tw, float mean0, float mean1,
                         float mean2, float* out0, float* out1, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Host launch path in C (csrc/replay.cpp).  A command = one call of a launch entry point of this header (every function that ends in
 * `void* stream`), an event record or a stream wait.  `op`: index from falnet_replay_op_index("falnet_conv2d") ..., or FALNET_CMD_RECORD /
 * FALNET_CMD_WAIT; `stream` / `event`: indices into the tables passed to falnet_replay; iarg: the pointer / integer arguments in
 * declaration order (nint of them), farg: the float / double ones (nflt), the trailing stream argument is supplied by the replay.
 * falnet_replay issues commands 0..n-1 in order and stops at the first failure (its index in *failed_at, -1 when all were issued); the
 * launches are ordinary launches -- same kernels, same streams, same dependencies as the eager sequence they were recorded from. */
#define FALNET_CMD_RECORD (-1)
#define FALNET_CMD_WAIT (-2)
typedef struct {
    int32_t op, stream, event, nint, nflt, reserved;
    uint64_t iarg[18];
    double farg[8];
} falnet_cmd_t;
#define FALNET_CMD_MAX_INT 18
#define FALNET_CMD_MAX_FLT 8
int falnet_replay_op_index(const char* name);
int falnet_replay_op_args(int op, int* nint, int* nflt);
int falnet_replay(const falnet_cmd_t* cmds, int n, void* const* streams, int nstreams, void* const* events, int nevents, int* failed_at);
/* p[0..n) = value (hipMemsetAsync / hipMemsetD32Async) and a device-to-device copy: the two aten launches of a static step, replayable */
int falnet_fill_f32(float* p, int64_t n, float value, void* stream);
int falnet_copy_bytes(void* dst, const void* src, int64_t nbytes, void* stream);
/* One wave that does nothing for `microseconds` (s_memrealtime, the 100 MHz constant clock) on `stream`: the probe of the plan's stream self-test
 * (fal_net_amd/plan.py: stream_selftest) -- two of them on two streams take ONE period when the streams sit on different hardware queues and TWO
 * when HIP has mapped both onto the same queue.  Not part of any step. */
int falnet_spin(int microseconds, void* stream);
/* The matrix-pipe rate the board SUSTAINS: 2 048 workgroups x 4 waves, each issuing iters x 16 register-resident v_mfma_f32_16x16x32 on the
 * caller's operands `ab` (64 x 8 x 64 x 8 16-bit values = 512 KiB; random data for the ceiling under real switching activity); FLOPs of one launch =
 * 2048 * 4 * iters * 16 * 16384.  bench.py's `roofline.sustained_mfma` (measurement only: no step launches it); `out` is never written on finite data. */
int falnet_mfma_probe(const void* ab, float* out, int iters, int dtype, void* stream);

/* ---- test-time outputs (csrc/dump.hip; Test_KITTI.py:211-253,303-317, myUtils.py:339-373) ----------------------------------------------
 * Inputs are planar f32 (B, C, H, W) as the model returns them; `mean_*` is the RGB mean the loader subtracted (0.411, 0.432, 0.45).  Byte outputs
 * are written as whole 32-bit words: the output pointer is 4-byte aligned and its ALLOCATION is rounded up to a multiple of 4 bytes (the pad
 * bytes are written 0).  The f32 arithmetic is the host's, operation by operation (correctly rounded division, no fused multiply-add), so the
 * 8-bit outputs equal numpy's byte for byte.  None of these is replayable (falnet_replay_op_index: -1).
 *
 * Exact q-th percentile (0 <= q <= 100) of each of the B samples of x (n_per_sample contiguous floats each), numpy's default 'linear' definition:
 * position q/100 (n - 1), the two order statistics on either side found exactly (radix select on a monotone integer image of the floats, integer
 * histograms: bit-identical from run to run), one interpolation in double.  NaN input is out of contract (a NaN sorts by its bit pattern); -0.0
 * sorts below +0.0.  workspace: falnet_percentile_workspace_bytes(B) bytes, cleared by the call itself; after the call the words [4] and [5] of each
 * sample's region (regions are workspace_bytes(B) / B bytes apart) hold the two order statistics as f32. */
int64_t falnet_percentile_workspace_bytes(int B);
int falnet_percentile_f32(const float* x, int64_t n_per_sample, int B, double q, float* out, void* workspace, void* stream);
/* Test_KITTI.py:213-216 without the host: v = 256 clip(d / (p95[b] + 1e-6), 0, 1) in f32, k = min(rint(v), 255) (round half to even),
 * out[b][y][x] = lut[k]; lut: 256 RGBA entries (fal_net_amd/plasma_lut.txt), out: (B, H, W, 4) u8; p95: B floats on the device */
int falnet_disp_to_plasma_u8(const float* disp, const float* p95, const void* lut_rgba, void* out_rgba, int B, int H, int W, void* stream);
/* Test_KITTI.py:229-241: planar (B, 3, H, W) -> interleaved (B, H, W, 3) u8, rint(255 (x + mean)) SATURATED to [0, 255] -- the one deliberate
 * difference: the reference's astype(uint8) wraps an out-of-range value around */
int falnet_image_to_u8(const float* x, float mean_r, float mean_g, float mean_b, void* out, int B, int H, int W, void* stream);
/* Test_KITTI.py:248-253: rint(clip(255 |x|, 0, 255)) of n floats -> n bytes in the same order */
int falnet_feature_to_u8(const float* x, void* out, int64_t n, void* stream);
/* local_normalization, Test_KITTI.py:303-317, win = 3 only: img = x + mean, mu = avg_pool2d(img, 3, 1, 1), sigma = avg_pool2d((img - mu)^2, 3, 1, 1)^(1/2)
 * (zero padding, divisor 9 at the borders too), out = (img - mu) / (sigma + 1e-7).  mu_out / sigma_out: NULL, or (B, 3, H, W) f32 that receive mu and
 * sigma (the quotient is ill-conditioned where sigma ~ 0; tests compare its two parts) */
int falnet_local_norm(const float* x, float mean_r, float mean_g, float mean_b, float* out, float* mu_out, float* sigma_out, int win, int B, int H, int W,
                      void* stream);
/* get_point_cloud, myUtils.py:339-373: z = focal baseline / (disp + 1e-4); u = j + 0.5, v = i + 0.5 (affine_grid with align_corners=False);
 * x = (u - W/2) / focal z and y = (v - H/2) / focal z from the UNCAPPED z, then z clamped to [0, 200]; colour = (img + mean) * rgb_scale (255 for a
 * model input; mean 0 and scale 1 for an image that is already 0..255, which is how the reference calls it).  out_planar: NULL or (B, 6, H W) f32, rows
 * x, z, -y, r, g, b; out_packed: NULL or (B, H W) binary-PLY vertex records of 15 bytes (x, z, -y as little-endian f32; r, g, b as u8, truncated
 * like the reference's int() and saturated).  At least one of the two. */
int falnet_point_cloud(const float* img, float mean_r, float mean_g, float mean_b, float rgb_scale, const float* disp, double focal, double baseline,
                       float* out_planar, void* out_packed, int B, int H, int W, void* stream);

/* ---- evaluation metrics (csrc/metrics.hip; myUtils.py:123-172,196-334, loss_functions.py:124-173) ---------------------------------------
 * The numbers an evaluation loop produces per frame, computed from the planar f32 maps where they lie and written into one ROW of a caller-owned,
 * device-resident table of doubles (FALNET_MET_ROW doubles per frame; a call writes only the columns of its own group).  The host reads the table
 * once after the last frame.  workspace: falnet_metrics_workspace_bytes() bytes, 8-byte aligned, owned by ONE stream at a time (calls on a stream
 * may share it: they are ordered).  Every reduction is deterministic: a fixed grid writes per-workgroup partial sums, a finalising kernel adds them
 * in index order; no floating-point atomics.  Two calls on the same inputs give bit-identical rows.  None of these is replayable. */
#define FALNET_DEPTH_KITTI2015 0 /* disps_to_depths_kitti2015: gt is a disparity, both depths fb / (d + (1 - [d > 0])), masked by gt > 0, whole frame */
#define FALNET_DEPTH_EIGEN 1     /* disps_to_depths_kitti: rows H-219:H-4, columns 44:1180, gt is a depth, masked by gt > 0 */
#define FALNET_DEPTH_MAKE3D 2    /* disps_to_depths_make + compute_make_errors: gt is a depth, masked by 0 < gt < max_d, always median-scaled, log10 term */
#define FALNET_MET_ROW 24
#define FALNET_MET_ABS_REL 0 /* depth group: the seven metrics in the order of kitti_error_names / make_error_names ... */
#define FALNET_MET_SQ_REL 1
#define FALNET_MET_RMS 2
#define FALNET_MET_LOG 3 /* log_rms; make3d: mean |log10 gt - log10 pred| */
#define FALNET_MET_A1 4
#define FALNET_MET_A2 5
#define FALNET_MET_A3 6
#define FALNET_MET_N 7    /* ... the number of pixels that count, the three threshold counts as integers ... */
#define FALNET_MET_N_A1 8
#define FALNET_MET_N_A2 9
#define FALNET_MET_N_A3 10
#define FALNET_MET_SCALE 11 /* ... and the median scale factor with the two medians it is made of (1, 0, 0 without median scaling) */
#define FALNET_MET_MEDIAN_GT 12
#define FALNET_MET_MEDIAN_PRED 13
#define FALNET_MET_EPE 14 /* end-point group: the mean and the number of pixels it is over */
#define FALNET_MET_EPE_N 15
#define FALNET_MET_RMSE 16 /* view group: get_rmse, get_mea, get_psnr and the three sums and the count behind them */
#define FALNET_MET_MEA 17
#define FALNET_MET_PSNR 18
#define FALNET_MET_VIEW_SUM_SQ 19
#define FALNET_MET_VIEW_SUM_ABS 20
#define FALNET_MET_VIEW_SUM_RSQ 21
#define FALNET_MET_VIEW_N 22
#define FALNET_MET_SSIM 23 /* structural similarity of the view (falnet_ssim_metric, csrc/ssim.hip): a group of its own, NaN until written */
int64_t falnet_metrics_workspace_bytes(void);
/* np.median(gt[mask]) / np.median(pred[mask]) of the depths of one frame (H x W f32 maps; `mode` and `fb` = focal * baseline as below), exact:
 * a radix select over the f64 depths with a 64-bit key, the number of selected pixels and the ranks found on the device; an even count takes the
 * mean of the two middle order statistics, in the type the host's array has (f32 for the ground truth of eigen / make3d).  scale_out: 4 doubles on
 * the device -- {factor, median gt, median pred, n} -- that falnet_depth_errors takes as `scale` without a host read (NaN when nothing is selected). */
int falnet_depth_median_scale(const float* pred_disp, const float* gt, int H, int W, int mode, double fb, double max_d, double* scale_out,
                              void* workspace, void* stream);
/* compute_kitti_errors / compute_make_errors of one frame: disparity -> depth per `mode`, optional scale (NULL: none; make3d requires it), both depths
 * clamped to [min_d, max_d], then abs_rel, sq_rel, rms, log term and the three `max(gt / pred, pred / gt) < 1.25^k` rates, in f64 per pixel in the
 * host's order.  fb: focal * 0.54 (kitti2015), focal * baseline (eigen), 721 * 0.22 (make3d), formed by the caller.  eigen needs H >= 219, W >= 1180.
 * min_d and max_d must be f32 values (the host clamps an f32 ground truth in f32). */
int falnet_depth_errors(const float* pred_disp, const float* gt, int H, int W, int mode, double fb, const double* scale, double min_d, double max_d,
                        double* row, void* workspace, void* stream);
/* realEPE: pred (B, 1, h, w) sampled bilinearly (align_corners=True, the arithmetic of falnet_resize_planar; equal sizes: the identity) at the size of
 * target (B, 1, H, W); mean of |target - up| over target != 0 (sparse) or over every pixel, accumulated in f64 */
int falnet_epe(const float* pred, int h, int w, const float* target, int B, int H, int W, int sparse, double* row, void* workspace, void* stream);
/* get_rmse / get_mea / get_psnr of a synthesised view against the real one, both (B, 3, H, W) normalised by the RGB mean: out = clamp(255 (x + mean), 0,
 * 255), lab = 255 (y + mean) in f32; sums of (out - lab)^2, |out - lab| and (round(out) - lab)^2 in f64 */
int falnet_view_errors(const float* out, const float* label, float mean_r, float mean_g, float mean_b, int B, int H, int W, double* row, void* workspace,
                       void* stream);

/* ---- structural similarity (csrc/ssim.hip; Wang et al. 2004) ------------------------------------------------------------------------------
 * For a plane pair x, y and a window w of radius R (the outer product of 1-D weights of sum 1), at every VALID window centre (no padding:
 * (H - 2R) x (W - 2R) of them): mx = sum w x, my = sum w y, vx = sum w x^2 - mx^2, vy likewise, cxy = sum w x y - mx my,
 * S = (2 mx my + C1)(2 cxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)).  One workgroup per tile of one plane; per-workgroup partial sums in the
 * caller's workspace (falnet_ssim_workspace_bytes(B, C, H, W, radius) bytes, 8-byte aligned, owned by one stream at a time; 0 for a radius that is
 * not built), added by a finalising kernel in a fixed order: no floating-point atomics, two calls give the same bits.  The workspace's LAST 8 bytes
 * receive the plain sum over the windows as a double (of S for the metric, of (1 - S) / 2 for the loss).  H < 2R + 1 or W < 2R + 1 is an argument
 * error.  None of these is replayable. */
int64_t falnet_ssim_workspace_bytes(int B, int C, int H, int W, int radius);
/* The metric: R = 5, Gaussian weights of sigma 1.5, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, on get_psnr's operands x = round(clamp((out + mean) * 255,
 * 0, 255)), y = (label + mean) * 255 formed in f32 without a fused multiply-add; window sums and everything after them in f64.
 * row[FALNET_MET_SSIM] = the mean of S over the B * 3 * (H - 10) * (W - 10) windows; no other column is touched.  out, label: (B, 3, H, W). */
int falnet_ssim_metric(const float* out, const float* label, float mean_r, float mean_g, float mean_b, int B, int H, int W, double* row, void* workspace,
                       void* stream);
/* The loss: the 3 x 3 box (radius 1, the only one built: any other radius is an argument error), C1 = 0.01^2, C2 = 0.03^2, x = synth + mean_c,
 * y = label + mean_c (C <= 3 channels), all f32:  out[0] (+)= scale * sum over the windows of (1 - S) / 2  (scale = 1 / (B C (H - 2)(W - 2)): the mean). */
int falnet_ssim_loss_fwd(const float* synth, const float* label, float mean_r, float mean_g, float mean_b, int B, int C, int H, int W, int radius,
                         float scale, float* out, int accumulate, void* workspace, void* stream);
/* ga (+)= gscale[0] * scale * d sum((1 - S) / 2) / d synth (gscale NULL: 1); every element of ga is written, the border pixels that fewer windows
 * contain included.  Needs no workspace. */
int falnet_ssim_loss_bwd(const float* synth, const float* label, float mean_r, float mean_g, float mean_b, int B, int C, int H, int W, int radius,
                         float scale, const float* gscale, float* ga, int accumulate, void* stream);
/* Both in one launch: out[0] += scale_out * sum (as falnet_ssim_loss_fwd with accumulate = 1); ga = (add_grad ? ga : 0) + gscale[0] * scale_grad * d sum /
 * d synth (as falnet_ssim_loss_bwd) -- add_grad = 1 joins the gradient another loss kernel has already written for the same tensor. */
int falnet_ssim_loss_fwd_bwd(const float* synth, const float* label, float mean_r, float mean_g, float mean_b, int B, int C, int H, int W, int radius,
                             float scale_out, float* out, float scale_grad, const float* gscale, float* ga, int add_grad, void* workspace, void* stream);

/* ---- Velodyne ground truth (csrc/velo.hip; the original Eigen split, Datasets/Kitti_eigen_test_original.py) -----------------------------------
 * Monodepth's generate_depth_map of one raw KITTI scan on the device.  points: n_points x 4 f32 (x, y, z, reflectance) as the .bin file holds them,
 * on the device; the fourth value is ignored and taken as 1.  P: 12 doubles on the HOST, the row-major 3 x 4 velodyne-to-image matrix, passed on to
 * the kernel by value.  Per point with x >= 0: s_i = ((P[i][0] x + P[i][1] y) + P[i][2] z) + P[i][3] in f64 with no fused multiply-add,
 * u = rint(s_0 / s_2) - 1, v = rint(s_1 / s_2) - 1 (half to even), depth = (float)s_2 (vel_depth: x); it lands on (v, u) when 0 <= u < W and
 * 0 <= v < H as doubles.  depth_out (H x W f32, device, every pixel written): the minimum depth over the points on the pixel through an integer
 * atomicMin on the monotone image of the f32 -- bit-identical for any order of the points and from run to run, no floating-point atomics; 0 where
 * no point lands and where the minimum is negative.  n_points = 0 gives an all-zero map.  H W < 2^31; every entry of P finite.  Not replayable. */
int falnet_velo_project(const float* points, int n_points, const double* P, int H, int W, int vel_depth, float* depth_out, void* stream);

/* ---- Pseudo-LiDAR (csrc/lidar.hip; fal_net_amd/pseudo_lidar.py) --------------------------------------------------------------------------------
 * The inverse of falnet_velo_project: an (H, W) f32 depth or disparity map on the device back-projected into Velodyne-format records, x forward,
 * y left, z up, intensity as four f32 -- the 16-byte point of a KITTI .bin file.  Q: 12 doubles on the HOST, the row-major 3 x 4 back-projection
 * matrix [M^-1 | M^-1 P[:,3]] of a velodyne-to-image matrix P with M = P[:, :3], passed on to the kernels by value.  Per pixel (v, u), all arithmetic
 * f64 in the stated order with no fused multiply-add unless marked f32:
 *   1. fb > 0: the map is a disparity, valid only if disp > 0, d = (float)(fb / (double)disp); fb == 0: the map is the depth d (the projection's
 *      third homogeneous coordinate, what falnet_velo_project writes);
 *   2. keep when d > min_depth && d <= max_depth (f32 compares: NaN and infinity fail);
 *   3. score (H x W f32, may be NULL): keep when score >= threshold (a NaN score is dropped);
 *   4. r_i = (Q[i][0] (u + 1) + Q[i][1] (v + 1)) + Q[i][2], X_i = d r_i - Q[i][3], (x, y, z) = (float)X_i; keep when x > 0 && z <= max_height
 *      (max_height may be +infinity);
 *   5. the record is x, y, z, intensity: intensity_map's value at the pixel (H x W f32), or the constant `intensity` when the map is NULL.
 * beams == 0 (dense): the kept records in row-major pixel order.  1 <= beams <= 128, 1 <= az_bins <= 4096 (beam mode): elev_edges_dev / az_edges_dev
 * are non-decreasing f64 tables ON THE DEVICE of beams + 1 tangents of the elevation edges and az_bins + 1 tangents of the azimuth edges; from the
 * f32 record widened back to f64, rho = sqrt(x x + y y), e = z / rho, a = y / x, beam = #{k : e >= te[k]} - 1, col = #{j : a >= ta[j]} - 1
 * (searchsorted(side='right') - 1; a NaN counts nothing); a point whose beam or col is outside its range is dropped.  Each bin keeps the point of the
 * smallest 64-bit key (bits(d) << 32) | (v W + u) -- nearest depth first, then the lowest pixel index -- through an integer atomicMin on a u64: no
 * floating-point atomics.  The winners are written in bin order, beam major.  Either mode is bit-identical from run to run and to the host
 * restatement (tests/_lidar_ref.py): both sides do only correctly rounded + - * / sqrt and comparisons against the same table values.
 * out_points: up to `capacity` records, 16-byte aligned (one record is one 16-byte store); count_dev: one int64 on the device, the TRUE number of kept
 * records -- where it exceeds capacity only the first `capacity` records are written and the call still returns 0; bytes beyond the written records
 * are not touched.  workspace: falnet_lidar_workspace_bytes(H, W, beams, az_bins) bytes, 8-byte aligned as count_dev and the tables (beam mode fills
 * its key table itself).  Refused with nothing written: a NULL map, Q, count_dev or workspace, NULL tables in beam mode, a NULL output with
 * capacity > 0, H W < 1 or >= 2^31, beams or az_bins out of range (az_bins is checked in dense mode too), a max_depth that is not finite, a negative
 * or non-finite fb, a NaN min_depth / max_height / threshold, a non-finite entry of Q, capacity < 0, a misaligned pointer.
 * falnet_lidar_workspace_bytes is 0 for a refused shape.  Not replayable. */
int64_t falnet_lidar_workspace_bytes(int H, int W, int beams, int az_bins);
int falnet_velo_unproject(const float* map, double fb, const float* score, float threshold, const float* intensity_map, float intensity, const double* Q,
                          float min_depth, float max_depth, float max_height, int H, int W, int beams, int az_bins, const double* elev_edges_dev,
                          const double* az_edges_dev, float* out_points, int64_t capacity, int64_t* count_dev, void* workspace, void* stream);

/* ---- Triangle mesh of the predicted depth (csrc/mesh.hip; fal_net_amd/mesh.py) ------------------------------------------------------------------
 * One sample's pixel grid triangulated and cut where depth jumps, as binary-PLY records (the numpy restatement is tests/_mesh_ref.py).
 * img (3 x H x W planar f32), means, rgb_scale, disp (H x W f32), focal, baseline: as falnet_point_cloud with B = 1 -- vertex g = i W + j IS that
 * cloud's vertex (csrc/pc_vertex.h): z = fb / (disp + 1e-4f), x and -y from the uncapped z, z capped to [0, 200], colour (img + mean) rgb_scale
 * truncated and saturated to a byte.
 *   valid vertex   min_depth < z && z <= max_depth on the capped f32 z, and with score (H x W f32, may be NULL) score >= threshold; every comparison
 *                  with a NaN is false.  0 <= min_depth < max_depth < 200, so a valid vertex is never a capped one.
 *   quad (i, j)    0 <= i < H - 1, 0 <= j < W - 1, corners a = (i, j), b = (i, j + 1), c = (i + 1, j), d = (i + 1, j + 1).  Two or more invalid corners:
 *                  no triangle.  One: the diagonal that avoids it (a or d invalid: b-c; b or c invalid: a-d).  None: a-d iff |za - zd| <= |zb - zc|
 *                  (f32 subtractions; a tie goes to a-d), else b-c.
 *   triangles      diagonal a-d: T0 = (a, c, d), T1 = (a, d, b); diagonal b-c: T0 = (a, c, b), T1 = (b, c, d).  With PLY axes x right, y forward, z up
 *                  (the record's x, z, -y) every (v1 - v0) x (v2 - v0) points towards the camera.
 *   keep rule      a triangle is kept iff its three vertices are valid and each edge (p, q) has max(zp, zq) <= min(zp, zq) * ratio: one correctly
 *                  rounded f32 multiply, ratio = (float)(1.0 + max_jump) formed in double and rounded once.  max_jump >= 0; infinity keeps every
 *                  valid triangle.
 *   vertices_out   the vertices named by a kept triangle, in pixel order: 15-byte records x y z f32, r g b u8 (fal_net_amd/dumps.py: PLY_VERTEX) or,
 *                  with_normals != 0, 27-byte records x y z nx ny nz f32, r g b u8.  Room for H W records.
 *   faces_out      the kept triangles in quad order, T0 before T1: 13-byte records, the byte 3 and three little-endian int32 indices into
 *                  vertices_out (a vertex's index is its rank among the used pixels).  Room for 2 (H - 1) (W - 1) records.
 *   normal         of a used vertex: the sum, over the kept triangles that contain it, of the un-normalised (V1 - V0) x (V2 - V0) in the triangle's
 *                  stored vertex order, taken over the quads (i - 1, j - 1), (i - 1, j), (i, j - 1), (i, j) in that order, T0 before T1; f64 from the f32
 *                  record coordinates, each component two products and a subtraction, no fused multiply-add; len = sqrt((nx nx + ny ny) + nz nz);
 *                  each of nx / len, ny / len, nz / len is divided in f64 and rounded to f32; (0, 0, 0) when len is zero or not finite.  A gather: no
 *                  scatter, no atomic.
 * counts_dev: two int64 on the device, the number of vertex and of face records.  Bytes beyond the records are not touched; positions are decided by
 * indices alone (csrc/ordered.h), so two calls give the same bytes.  workspace: falnet_mesh_workspace_bytes(H, W) bytes, 8-byte aligned as counts_dev;
 * img, disp, score and the two outputs 4-byte aligned.  H < 2 or W < 2 is legal: counts (0, 0), nothing else written.  Refused with nothing launched:
 * a NULL img, disp, output, counts_dev or workspace, H W < 1 or >= 2^28, focal <= 0, min_depth / max_depth outside the stated order (a NaN included),
 * a negative or NaN max_jump, a misaligned pointer.  falnet_mesh_workspace_bytes is 0 for a refused shape.  One sample per call.  Not replayable. */
int64_t falnet_mesh_workspace_bytes(int H, int W);
int falnet_mesh_build(const float* img, float mean_r, float mean_g, float mean_b, float rgb_scale, const float* disp, double focal, double baseline,
                      const float* score, float threshold, float min_depth, float max_depth, double max_jump, int H, int W, int with_normals,
                      void* vertices_out, void* faces_out, int64_t* counts_dev, void* workspace, void* stream);

/* ---- Connected components of a depth or disparity map (csrc/components.hip; fal_net_amd/components.py) ------------------------------------------------
 * map: B maps of H x W f32, one after the other; pixel g = i W + j of a map has the value v_g.  The map is taken as given, depth or disparity: the
 * edge test is a ratio and means the same on either (the numpy restatement is tests/_components_ref.py).
 *   valid pixel   lo < v_g && v_g <= hi, and with score (B x H x W f32, may be NULL) also score_g >= threshold; every comparison with a NaN is false.
 *                 0 <= lo < hi; hi may be +infinity; a NaN bound is refused.
 *   edge          two 4-neighbours p, q (right, down) are joined iff both are valid and max(v_p, v_q) <= min(v_p, v_q) * ratio: one correctly rounded
 *                 f32 multiply, the keep rule of falnet_mesh_build, whose ratio = (float)(1.0 + max_jump) the caller forms in double and rounds once.
 *                 ratio >= 1; +infinity joins all valid neighbours; a NaN is refused.  A tie joins.
 *   component     a connected set of that graph.
 *   label         (int32, B x H x W, may be NULL: not wanted) label_g = the smallest pixel index of g's component, -1 for an invalid pixel.  Indices
 *                 are per image: the labels of image b do not carry b H W.
 *   size          (int32, B x H x W) size_g = the number of pixels of g's component, 0 for an invalid pixel.
 *   info          (int64, 3 B + 1 words) per image the number of components (pixels with label_g == g), the number of valid pixels and the largest
 *                 component's size; then one status word, 0 when every loop of the kernels ran to its end.  Every data-dependent loop is cut after
 *                 H W iterations, which a correct kernel never reaches, and then sets a bit there (1: tile pass, 2: border merge, 4: flatten) --
 *                 the outputs of such a call mean nothing.
 * Both outputs are written in full, the -1 / 0 of the invalid pixels included, and nothing beyond them.  The result is a function of the input alone:
 * not of the launch geometry, the order in which workgroups arrive or falnet_set_deterministic; two calls give the same bits (integer atomics only:
 * min, add, max).  workspace: falnet_components_workspace_bytes(B, H, W) bytes (0 for a refused shape), 8-byte aligned as info; map, score and the two
 * outputs 4-byte aligned.  H = 1 or W = 1 is legal.  Refused with nothing launched: a NULL map, size, info or workspace, B < 1, H W < 1, H W >= 2^30,
 * B H W >= 2^31, lo / hi outside the stated order (a NaN included), ratio < 1 or NaN, a misaligned pointer.  Four launches for a batch of up to 65535
 * maps, the image index in the block index.  Not replayable. */
int64_t falnet_components_workspace_bytes(int B, int H, int W);
int falnet_components(const float* map, const float* score, float threshold, float lo, float hi, float ratio, int B, int H, int W, int32_t* label,
                      int32_t* size, int64_t* info, void* workspace, void* stream);

/* ---- stable segmented argsort (csrc/sort.hip; fal_net_amd/sparsification.py: argsort_u32) ---------------------------------------------------
 * keys: `segments` independent arrays of n u32 keys each, keys[s * n + i], 1 <= segments <= 8, n <= 2^24, on the device, never written.
 * perm[s * n + r] = the index i of the element of segment s that has rank r in ascending key order; equal keys stay in ascending index order
 * (np.argsort(kind="stable")).  Four least-significant-digit passes of 8 bits, three launches each, every segment in the same launches; no output
 * position depends on an atomic: two calls write the same bytes.  workspace: falnet_sort_u32_workspace_bytes(n, segments) bytes (0 for a refused
 * shape and for n = 0), 8-byte aligned as perm.  n = 0 returns 0 and writes nothing.  Refused before any launch: n < 0 or n > 2^24, segments
 * outside 1 .. 8, a NULL pointer, a perm or workspace that is not 8-byte aligned.  Not replayable. */
int64_t falnet_sort_u32_workspace_bytes(int64_t n, int segments);
int falnet_sort_u32(const uint32_t* keys, int64_t n, int segments, uint32_t* perm, void* workspace, void* stream);

/* ---- sparsification curves (csrc/sparsify.hip; fal_net_amd/sparsification.py) -----------------------------------------------------------------
 * pred_disp, gt, H, W, mode, fb, scale (may be NULL), min_d, max_d: exactly the arguments of falnet_depth_errors; the pixels that count, their
 * number n and their depths g, p (scaled, then clamped) are that function's.  The counted pixels are numbered 0 .. n - 1 in row-major order of the
 * region.  Per pixel in f64: e_abs = |g - p| / g, e_sq = (g - p)^2, t = max(g / p, p / g).  An f32 x has the key k(x) = 0xFFFFFFFF for a NaN,
 * bits ^ 0xFFFFFFFF with the sign bit set, bits | 0x80000000 otherwise; an ordering is the stable ascending sort of ~k(x): the largest x first,
 * NaN before everything, ties in pixel-number order.  There are scores.n + 3 orderings: x = map[s] (sign +1: larger is more uncertain) or -map[s]
 * (sign -1: larger is more confident) at the pixel's place in the H x W map, then the oracles x = (float)e_abs, (float)e_sq, (float)t.
 * Cut j of `steps` = S (2 .. 100) removes the first r_j = (j n) / S pixels of an ordering and keeps n_j = n - r_j; of the kept pixels
 * abs_rel_j = sum e_abs / n_j, rms_j = sqrt(sum e_sq / n_j), d1_j = (n_j - #{t < 1.25}) / n_j.
 * row: 1 + (3 scores.n + 3) S doubles -- n; per score its abs_rel, rms and d1 curves; the oracle abs_rel, rms and d1 curves (each from the
 * ordering of its own metric); n = 0 gives NaN curves.  Sums have a fixed partition and order: two calls give the same bits.
 * workspace: falnet_sparsify_workspace_bytes(H, W, scores.n) bytes (0 for a refused shape), 8-byte aligned as row and scale.  Refused with nothing
 * written: what falnet_depth_errors refuses, H W > 2^24, steps or scores.n out of range, a sign that is not +1 or -1, a NULL map.  Not replayable. */
typedef struct {
    const float* map[4]; /* H x W f32 on the device */
    int sign[4];         /* +1 or -1 */
    int n;               /* 0 .. 4 */
} falnet_scores_t;
int64_t falnet_sparsify_workspace_bytes(int H, int W, int n_scores);
int falnet_sparsify(const float* pred_disp, const float* gt, int H, int W, int mode, double fb, const double* scale, double min_d, double max_d,
                    falnet_scores_t scores, int steps, double* row, void* workspace, void* stream);

/* ---- cloud metrics: nearest neighbour, Chamfer distance and F-score (csrc/nearest.hip; fal_net_amd/cloud_metrics.py) ---------------------------
 * query: nq records, ref: nr records on the device; a record is 4 consecutive f32 x, y, z, . -- the 16-byte point of falnet_velo_unproject and of a
 * KITTI .bin file; the fourth value is ignored.  0 <= nq, nr < 2^31.  For a query q and a reference r (the numpy restatement is
 * tests/_cloud_ref.py):
 *   dx = qx - rx, dy = qy - ry, dz = qz - rz;   d2(q, r) = (dx dx + dy dy) + dz dz
 * every operation rounded to f32 in this order, no fused multiply-add.  A pair whose d2 is NaN -- a non-finite coordinate, inf - inf -- does not take
 * part.  d2[q] (f32) is the minimum over the pairs that take part, idx[q] (int32) the smallest r that attains it; a query with no pair taking part
 * (nr = 0 included) gets d2 = +inf, idx = -1.  nq = 0 issues no launch.  d2 is >= +0 or NaN, so its bits are monotone as an unsigned integer, and the
 * 64-bit key (bits(d2) << 32) | r decides value and tie together: the result does not depend on how the references are divided among workgroups,
 * and is bit-identical to the host restatement and from run to run.
 * splits: into how many ranges of whole tiles the references are divided over the grid's second dimension; 0: falnet_nearest_splits(nq, nr), the
 * library's choice (1 for an empty set, 0 for a refused shape); at most 1024.  One split stores the result plainly; S > 1 takes one integer atomicMin
 * per query and split on a u64 key in `workspace` -- falnet_nearest_workspace_bytes(nq, nr, splits) bytes, 8-byte aligned, 0 bytes (and may be NULL)
 * for one split; the library fills it on the stream, and a finishing launch unpacks it.  No floating-point atomics.  query and ref 16-byte aligned,
 * d2 and idx 4-byte aligned.  Refused with nothing launched: a NULL pointer, nq or nr outside [0, 2^31), splits outside [0, 1024], a misaligned
 * pointer.  Not replayable. */
int falnet_nearest_splits(int64_t nq, int64_t nr);
int64_t falnet_nearest_workspace_bytes(int64_t nq, int64_t nr, int splits);
int falnet_nearest(const float* query, int64_t nq, const float* ref, int64_t nr, int splits, float* d2, int32_t* idx, void* workspace, void* stream);

/* The sums of one frame's two d2 arrays -- prediction -> ground truth (n_pred entries) and ground truth -> prediction (n_gt entries), both on the
 * device -- into one row of FALNET_CLOUD_ROW doubles of a device-resident table.  tau2: K <= FALNET_CLOUD_MAX_THRESHOLDS doubles on the HOST,
 * tau2[k] = tau_k tau_k, each >= 0.  Per direction, over the FINITE entries only (a non-finite one is left out of everything):
 *   n = their number;  sum sqrt((double)d2);  sum (double)d2;  per k < K the count of (double)d2 <= tau2[k]   (the counts of k >= K are 0)
 * The sums are f64 over a fixed grid in a fixed order (a thread's stride, the shuffles of a wave, the waves, the workgroups): two calls give the same
 * bits; the counts are exact.  Means and ratios (accuracy, completeness, Chamfer distance, precision, recall, F-score) are the host's to form after
 * reading the table.  workspace: falnet_cloud_errors_workspace_bytes() bytes, 8-byte aligned as row; the d2 arrays 4-byte aligned (NULL with 0
 * entries is legal).  Two launches.  Not replayable. */
#define FALNET_CLOUD_MAX_THRESHOLDS 8
#define FALNET_CLOUD_N_PRED 0      /* finite entries of the prediction -> ground truth array */
#define FALNET_CLOUD_SUM_PRED 1    /* sum of their sqrt: metres */
#define FALNET_CLOUD_SUMSQ_PRED 2  /* sum of them: square metres */
#define FALNET_CLOUD_N_GT 3        /* the same three of the ground truth -> prediction array */
#define FALNET_CLOUD_SUM_GT 4
#define FALNET_CLOUD_SUMSQ_GT 5
#define FALNET_CLOUD_HIT_PRED 6    /* 8 columns: prediction entries within tau_k (precision's numerator) */
#define FALNET_CLOUD_HIT_GT 14     /* 8 columns: ground-truth entries within tau_k (recall's numerator) */
#define FALNET_CLOUD_ROW 22
int64_t falnet_cloud_errors_workspace_bytes(void);
int falnet_cloud_errors(const float* d2_pred, int64_t n_pred, const float* d2_gt, int64_t n_gt, const double* tau2, int K, double* row,
                        void* workspace, void* stream);

/* ---- the ground plane of a scan: consensus fit, moments, heights, removal (csrc/ground.hip; fal_net_amd/ground.py) -----------------------------
 * points: n records on the device; a record is 4 consecutive f32 x, y, z, . -- the 16-byte point of falnet_velo_unproject (x forward, y left, z up);
 * the fourth value is ignored.  A plane is held in height form z = p x + q y + r, and every residual is the vertical one (the numpy
 * restatement is tests/_ground_ref.py):
 *   e = z - ((p x + q y) + r)
 * every operation rounded to f32 in this order, no fused multiply-add.  A point is an inlier of a plane iff |e| <= tol in f32; a NaN anywhere makes
 * the comparison false, so a non-finite point never takes part.  The band is vertical on purpose: no square root is taken anywhere a result decides
 * an integer; for the tilts admitted below it differs from the perpendicular band by less than 3.5 %.
 *
 * falnet_ground_hypotheses: triples is (H, 3) int32 on the device, indices into points.  Plane h is formed in f64 in this order, without FMA:
 *   u = P1 - P0, v = P2 - P0;  nx = uy vz - uz vy, ny = uz vx - ux vz, nz = ux vy - uy vx;  p = -(nx / nz), q = -(ny / nz), r = z0 - (p x0 + q y0)
 * It is valid iff p, q, r are finite and (p p + q q) <= tan2_max (a repeated index or a collinear triple gives nz = 0 and is invalid; so is an index
 * outside [0, n), whose point is not read).  planes[h] = (f32 p, f32 q, f32 r, 1.0f), or four +0 when invalid.  f64 + - x / are IEEE on both sides:
 * the host reproduces the planes bit for bit.  3 <= n < 2^31, 1 <= H <= FALNET_GROUND_MAX_HYPOTHESES.
 *
 * falnet_ground_consensus: counts[h] (u32) = the number of inliers of plane h, 0 for an invalid one.  best: FALNET_GROUND_BEST_WORDS 32-bit words,
 * 8-byte aligned: the maximum of the 64-bit key (count << 32) | (0xffffffff - h) -- the largest count, ties to the smallest index -- as low and high
 * word; the status (1: a plane; 0: no hypothesis has 3 inliers, "no plane"); the winning index (-1 without a plane); the bits of its f32 p, q, r
 * (+0 without a plane); the largest count.  Counts are integers, so the result does not depend on how the points are divided among workgroups.
 * splits: into how many ranges of whole tiles the points are divided over the grid's second dimension; 0: falnet_ground_splits(n, H), the library's
 * choice (0 for a refused shape); at most 1024.  One split stores the counts plainly; S > 1 takes one integer atomicAdd per hypothesis and workgroup
 * on the u32 counters of `workspace` -- falnet_ground_consensus_workspace_bytes(n, H, splits) bytes, 8-byte aligned, 0 bytes (and may be NULL) for
 * one split; the library zeroes it on the stream.  No floating-point atomics.  Not replayable. */
#define FALNET_GROUND_MAX_HYPOTHESES 4096
#define FALNET_GROUND_BEST_WORDS 8
#define FALNET_GROUND_BEST_KEY 0     /* two words: low, high */
#define FALNET_GROUND_BEST_STATUS 2
#define FALNET_GROUND_BEST_INDEX 3
#define FALNET_GROUND_BEST_PLANE 4   /* three words: the bits of p, q, r */
#define FALNET_GROUND_BEST_COUNT 7
int falnet_ground_hypotheses(const float* points, int64_t n, const int32_t* triples, int64_t H, double tan2_max, float* planes, void* stream);
int falnet_ground_splits(int64_t n, int64_t H);
int64_t falnet_ground_consensus_workspace_bytes(int64_t n, int64_t H, int splits);
int falnet_ground_consensus(const float* points, int64_t n, const float* planes, int64_t H, float tol, int splits, uint32_t* counts, uint32_t* best,
                            void* workspace, void* stream);

/* The moments of the inliers of one plane into one row of FALNET_GROUND_ROW doubles of a device-resident table: n, sum x, y, z, xx, xy, yy, xz, yz,
 * zz in f64, products formed in f64 from the f32 coordinates, then the plane: index, count, p, q, r (the f32 values widened) and status.  The plane is
 * the `best` record of falnet_ground_consensus in device memory -- no host round trip; status 0 sums nothing -- or, with best NULL, the caller's p, q,
 * r, index and count (status 1).  The sums run over a fixed grid in a fixed order (a thread's stride, the shuffles of a wave, the waves, the
 * workgroups): two calls give the same bits, n is exact.  workspace: falnet_ground_moments_workspace_bytes() bytes, 8-byte aligned as row.
 * 3 <= n < 2^31.  Two launches.  Not replayable. */
#define FALNET_GROUND_N 0
#define FALNET_GROUND_SX 1
#define FALNET_GROUND_SY 2
#define FALNET_GROUND_SZ 3
#define FALNET_GROUND_SXX 4
#define FALNET_GROUND_SXY 5
#define FALNET_GROUND_SYY 6
#define FALNET_GROUND_SXZ 7
#define FALNET_GROUND_SYZ 8
#define FALNET_GROUND_SZZ 9
#define FALNET_GROUND_INDEX 10   /* the winning hypothesis, -1 without one */
#define FALNET_GROUND_COUNT 11   /* its inlier count */
#define FALNET_GROUND_P 12       /* the plane whose inliers were summed */
#define FALNET_GROUND_Q 13
#define FALNET_GROUND_R 14
#define FALNET_GROUND_STATUS 15  /* 1: a plane; 0: no plane, every sum is 0 */
#define FALNET_GROUND_ROW 16
int64_t falnet_ground_moments_workspace_bytes(void);
int falnet_ground_moments(const float* points, int64_t n, const uint32_t* best, float p, float q, float r, int32_t index, uint32_t count, float tol,
                          double* row, void* workspace, void* stream);

/* heights[i] = (z - ((p x + q y) + r)) cz in the f32 chain above; cz = f32(1 / sqrt(1 + p p + q q)) of the refined plane is the host's to pass.
 * falnet_ground_split keeps the records with lo < h <= hi (inside != 0) or every other record (inside == 0; a NaN height is outside every range), in
 * point order -- the ordered compaction of csrc/ordered.h: count, one scan, scatter -- into out_points, at most `capacity` records; *count_dev (int64
 * on the device) is the number kept, also when it exceeds the capacity, exactly as falnet_velo_unproject reports it.  workspace:
 * falnet_ground_split_workspace_bytes(n) bytes, 8-byte aligned.  0 <= n < 2^31; n == 0 launches nothing and writes nothing.  Not replayable. */
int falnet_ground_heights(const float* points, int64_t n, float p, float q, float r, float cz, float* heights, void* stream);
int64_t falnet_ground_split_workspace_bytes(int64_t n);
int falnet_ground_split(const float* points, int64_t n, float p, float q, float r, float cz, float lo, float hi, int inside, float* out_points,
                        int64_t capacity, int64_t* count_dev, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
