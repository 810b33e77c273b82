// One bf16 K or V row of D elements -> D e4m3 bytes plus one fp32 scale: the row function of the FP8 cache format, shared by every kernel that
// writes it (kv_quantize_fp8.hip: the host-driven quantiser; layer_kv_mirror_fp8.hip: the mirror writer inside the paged layer call), so that a
// row has ONE set of bits whoever quantised it.
//   scale = amax / 448 (IEEE fp32 division; 1.0f for an all-zero row),  q = e4m3_rne(clamp(x / scale, -448, 448))
// A row that holds a NaN, a +inf or a -inf gets a NaN scale and an e4m3 NaN code (0x7F or 0xFF) in every byte.
// A row is D / 8 CONSECUTIVE lanes of one wave, lane `sub` of them holding elements [8 sub, 8 sub + 8): one 16-byte load per lane, the row's
// absmax by xor-shuffles inside the row's lanes, eight divisions, four v_cvt_pk_fp8_f32 (the instruction does not saturate: 465 and beyond
// would become NaN, hence the clamp), one 8-byte store per lane and one scale store per row.  All D / 8 lanes of a row call it together.
#pragma once
#include "nsa_common.hpp"

namespace nsa {

template <int D>
__device__ __forceinline__ void kv_quantize_fp8_row(const __bf16 *x_row, unsigned char *q_row, float *scale_slot, int sub) {
    constexpr int LPR = D / 8;  // lanes per row
    const u32x4 raw = *(const u32x4 *)(x_row + 8 * sub);
    float x[8];
    // the row's absmax as the largest |x| bit pattern: the unsigned order of the patterns is the order of the values, with +inf (0x7f800000) and
    // every NaN above all finite ones, so a non-finite element survives the reduction whatever fmaxf does with a NaN
    uint32_t amax_bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = raw[i] << 16, hi = raw[i] & 0xffff0000u;
        x[2 * i] = __uint_as_float(lo);
        x[2 * i + 1] = __uint_as_float(hi);
        amax_bits = max(amax_bits, max(lo & 0x7fffffffu, hi & 0x7fffffffu));
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) amax_bits = max(amax_bits, (uint32_t)__shfl_xor((int)amax_bits, o, 64));
    // the row holds an inf or a NaN: NaN scale, NaN bytes.  Branch-free -- such a row runs the divisions like any other (its scale is inf or NaN
    // here) and gets the seven NaN bits ORed into every byte: 0x7F or 0xFF, both NaN in e4m3
    const uint32_t nan_bytes = amax_bits >= 0x7f800000u ? 0x7f7f7f7fu : 0u;
    const float amax = __uint_as_float(amax_bits);
    const float scale = amax_bits == 0 ? 1.0f : amax / 448.0f;
    u32x2 out;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = fminf(fmaxf(x[4 * i + k] / scale, -448.0f), 448.0f);
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
        out[i] = (uint32_t)w | nan_bytes;
    }
    *(u32x2 *)(q_row + 8 * sub) = out;
    if (sub == 0) *scale_slot = nan_bytes ? __uint_as_float(0x7fc00000u) : scale;
}

}  // namespace nsa
