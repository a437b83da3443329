// Weight-gradient dispatch, shared by wgrad.hip (the chooser and the kernel table) and the files that hold the streaming kernels
// (wgrad_rows.hip, wgrad_wave.hip): the kernel ids, the chooser's result, the canonical-tap test and the launchers' prototypes.
// (Not part of common.h: that file is hashed into the autotune cache header, and nothing here bears on a conv choice.)
#pragma once
#include "common.h"

// the kernels behind falnet_wgrad (the values are the public FALNET_WGK_* ids: falnet_wgrad_kernel_name returns them)
enum WgradKernel {
    WGK_BAD = -1,
    WGK_TAP = FALNET_WGK_TAP,
    WGK_PATCH = FALNET_WGK_PATCH,
    WGK_S2 = FALNET_WGK_S2,
    WGK_C3 = FALNET_WGK_C3,
    WGK_C3WAVE = FALNET_WGK_C3WAVE,
    WGK_ROWS = FALNET_WGK_ROWS,
    WGK_ROWS_S2 = FALNET_WGK_ROWS_S2,
    WGK_WAVE = FALNET_WGK_WAVE,
};

// choose_wgrad_kernel's result: the kernel and the template arguments of the instantiation its launcher runs (and its symbol names)
struct WgradChoice {
    WgradKernel kernel = WGK_BAD;
    int ciw = 1, cow = 1;  // patch / s2: 32-channel input / output blocks per workgroup (patch: 1x1, 1x2, 2x1; s2: cow 1 | 2)
    int nco = 1;           // wave: 32-channel output blocks (gC / 32)
    bool s2 = false;       // wave: the stride-2 form
    int up2 = 0;           // rows: falnet_wgrad_t::up2 (0 high-resolution form, 1 one parity class per split, 2 all four per step)
};

// the 3x3 taps in row-major order, (dy, dx) = (t / 3 - 1, t % 3 - 1): what every halo / streaming kernel assumes
static inline bool falnet_wgrad_canonical_taps9(const falnet_wgrad_t& p) {
    if (p.ntaps != 9) return false;
    for (int t = 0; t < 9; ++t)
        if (p.tap_dy[t] != t / 3 - 1 || p.tap_dx[t] != t % 3 - 1) return false;
    return true;
}

bool falnet_wgrad_rows_applicable(const falnet_wgrad_t& p);     // wgrad_rows.hip: row-streaming kernel (variant 7)
int falnet_wgrad_rows_launch(const falnet_wgrad_t& p, const WgradChoice& c, hipStream_t st);
bool falnet_wgrad_rows_s2_applicable(const falnet_wgrad_t& p);  // wgrad_rows.hip: its stride-2 form (variant 8)
int falnet_wgrad_rows_s2_launch(const falnet_wgrad_t& p, const WgradChoice& c, hipStream_t st);
bool falnet_wgrad_wave_applicable(const falnet_wgrad_t& p);     // wgrad_wave.hip: wave-streaming kernel for 32-channel inputs (variant 9)
int falnet_wgrad_wave_launch(const falnet_wgrad_t& p, const WgradChoice& c, hipStream_t st);
bool falnet_wgrad_c3wave_applicable(const falnet_wgrad_t& p);   // wgrad_wave.hip: the first layer's gradient in the wave-streaming form (variant 6)
int falnet_wgrad_c3wave_launch(const falnet_wgrad_t& p, const WgradChoice& c, hipStream_t st);
