// nsa_band_attn_fwd_ragged_fp8 / nsa_band_attn_fwd_paged_fp8: the MFMA band forward (band_attn_mfma.hip has the mapping) over e4m3 K/V with
// one fp32 scale per key row -- band_attn_fwd_fp8.hpp has the body, the staging and the LDS map.  bf16 queries, Dk = Dv in {64, 128}, the
// three forms the ragged call plans (band_plan): split NT = 1 with the selection kernel's combine pass behind it, unsplit NT = 1, unsplit
// NT = 3 (D = 64) / 2 (D = 128).  A translation unit of its own: the bf16 kernels' modules keep their instantiations, and with them their code.
#include "attn_mfma_tiles.hpp"
#include "band_attn_fwd_fp8.hpp"

namespace nsa {

template <int D, int NT, bool SPLIT, bool PAGED>
__global__ __launch_bounds__(256, 2) void band_attn_fwd_fp8_kernel(BandAttnParams P, BandFp8Scales Z, BandPageTable PT) {
    band_attn_body_fp8<D, NT, SPLIT, PAGED>(P, Z, blockIdx.x, &PT);
}

template <int D, bool PAGED>
static int launch_band_fp8_t(const BandAttnParams &P0, const BandFp8Scales &Z, const BandPageTable &pt, hipStream_t st) {
    constexpr int NTW = D == 64 ? 3 : 2;
    BandAttnParams P = P0;
    BandLaunch L;
    // (the caller has checked the workspace: a plan that splits has its records, there is no second form to fall to)
    if (int rc = band_launch_plan(P, true, "band_attn_fp8", &L)) return rc;
    // two stages of (V tile + scales) per wave: 18 / 34 KiB a workgroup where the bf16 kernels ask 32 / 64 KiB
    const size_t lds = 4 * (size_t)band_fp8_wave_lds(D);
    if (L.split) {
        hipLaunchKernelGGL((band_attn_fwd_fp8_kernel<D, 1, true, PAGED>), dim3(L.grid), dim3(256), lds, st, P, Z, pt);
        NSA_LAUNCH_CHECK("band_attn_fwd_fp8(split)");
        const SelAttnParams C = band_combine_params(P);
        hipLaunchKernelGGL((sel_attn_combine_kernel<__bf16, D>), dim3((unsigned)((C.R * C.h + 3) / 4)), dim3(256), 0, st, C);
        NSA_LAUNCH_CHECK("band_attn_combine");
        return NSA_OK;
    }
    if (L.nt != NTW) hipLaunchKernelGGL((band_attn_fwd_fp8_kernel<D, 1, false, PAGED>), dim3(L.grid), dim3(256), lds, st, P, Z, pt);
    else hipLaunchKernelGGL((band_attn_fwd_fp8_kernel<D, NTW, false, PAGED>), dim3(L.grid), dim3(256), lds, st, P, Z, pt);
    NSA_LAUNCH_CHECK("band_attn_fwd_fp8");
    return NSA_OK;
}

int launch_band_attn_fwd_fp8(const BandAttnParams &P, const BandFp8Scales &Z, hipStream_t st, const BandPageTable *pt) {
    NSA_CHECK_ARG(P.t_pos && Z.k_scale && Z.v_scale, "band_attn_fp8: per-sequence positions and both scales");
    NSA_CHECK_ARG(P.Dk == P.Dv && (P.Dk == 64 || P.Dk == 128), "band_attn_fp8: Dk = Dv in {64, 128}");
    if (pt) return P.Dk == 64 ? launch_band_fp8_t<64, true>(P, Z, *pt, st) : launch_band_fp8_t<128, true>(P, Z, *pt, st);
    const BandPageTable none{};
    return P.Dk == 64 ? launch_band_fp8_t<64, false>(P, Z, none, st) : launch_band_fp8_t<128, false>(P, Z, none, st);
}

}  // namespace nsa
