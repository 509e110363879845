// DPP all-reductions over the 16 lanes of a DPP row (lanes sharing lane >> 4), shared by the fused token-pair kernels
// (contrastive_fused.hip, search_fp8.hip).
#pragma once
#include "common.h"

template <int CTRL>
DEVINL float dpp_mov_f(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
DEVINL int dpp_mov_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true); }
// xor 1, xor 2 as quad permutes; once quads are uniform the half-row / row mirrors exchange the remaining halves
DEVINL float row16_max(float x) {
    x = fmaxf(x, dpp_mov_f<0xB1>(x));
    x = fmaxf(x, dpp_mov_f<0x4E>(x));
    x = fmaxf(x, dpp_mov_f<0x141>(x));
    x = fmaxf(x, dpp_mov_f<0x140>(x));
    return x;
}
DEVINL int row16_min(int x) {
    x = min(x, dpp_mov_i<0xB1>(x));
    x = min(x, dpp_mov_i<0x4E>(x));
    x = min(x, dpp_mov_i<0x141>(x));
    x = min(x, dpp_mov_i<0x140>(x));
    return x;
}
DEVINL float row16_sum(float x) {
    x += dpp_mov_f<0xB1>(x);
    x += dpp_mov_f<0x4E>(x);
    x += dpp_mov_f<0x141>(x);
    x += dpp_mov_f<0x140>(x);
    return x;
}
