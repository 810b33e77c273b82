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

// The sliding and the compressed branch of a ragged layer decode over e4m3 K/V in ONE launch (nsa_layer_decode_ragged_fp8): two argument
// blocks with one position array, both in the split NT = 1 ragged form with a common nsplit and no combine pass -- every (token group,
// split) wave leaves its (m, l, o) record where the bf16 dual launch leaves it (an empty-interval record for a sequence that is not live),
// and decode_finish_kernel merges them.  Workgroups [0, grid0) take block A, the rest block B.
// ONE body.  The bf16 dual kernel inlines its body once per block; here the workgroup's block is chosen first -- blockIdx.x is uniform, so
// the choice is a scalar select per member, the arguments stay in scalar registers -- and the body stands once: half the code in a launch
// whose two halves run side by side on a CU, and the registers of one instantiation.
template <int D>
__global__ __launch_bounds__(256, 2) void band_attn_fwd_dual_fp8_kernel(BandAttnParams PA, BandFp8Scales ZA, BandAttnParams PB, BandFp8Scales ZB,
                                                                        unsigned grid0) {
    const bool a = blockIdx.x < grid0;
    const BandAttnParams P = a ? PA : PB;
    const BandFp8Scales Z = a ? ZA : ZB;
    band_attn_body_fp8<D, 1, true, false>(P, Z, a ? blockIdx.x : blockIdx.x - grid0, nullptr);
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

// the FP8 counterpart of launch_band_attn_fwd_dual: (P0, Z0) the sliding, (P1, Z1) the compressed branch.  The plan is band_dual_plan's, so
// the grids, the split count and the record offsets are the bf16 launch's.  Order: workgroups are handed out by index, so the block whose
// waves walk MORE key rows goes first and the short ones fill the tail.  Both blocks share nsplit, so rows per wave compare as rows per
// branch: the window's min(w, tokens) against the compressed rows, both of the largest sequence the host bound allows (the host never
// reads the positions) -- sliding first up to about 16 w tokens of context, compressed first beyond.
int launch_band_attn_fwd_dual_fp8(const BandAttnParams &A0, const BandFp8Scales &Z0, const BandAttnParams &A1, const BandFp8Scales &Z1, hipStream_t st) {
    const char *who = "band dual launch (fp8)";
    BandAttnParams P[2] = {A0, A1};
    int64_t waves[2];
    NSA_CHECK_ARG(P[0].t_pos && P[0].t_pos == P[1].t_pos && P[0].t_max == P[1].t_max, "%s: one position array for both branches", who);
    NSA_CHECK_ARG(Z0.k_scale && Z0.v_scale && Z1.k_scale && Z1.v_scale, "%s: both scales of both branches", who);
    // (D = 128 has no instantiation: its only caller pairs the branches where the finish kernel takes their records, Dv = 64)
    NSA_CHECK_ARG(P[0].Dk == 64 && P[0].Dv == 64 && P[1].Dv == 64, "%s: Dk = Dv = 64 only", who);
    NSA_CHECK_ARG(band_dual_plan(&P[0], &P[1], NSA_DT_BF16, waves) && P[0].nsplit == P[1].nsplit,
                  "%s: both branches in split form with deferred combine and a common split count, one supported shape", who);
    const unsigned grid[2] = {(unsigned)((waves[0] + 3) / 4), (unsigned)((waves[1] + 3) / 4)};
    const bool cmp_first = P[1].S_kv > std::min(P[0].w, P[0].S_kv);
    const int a = cmp_first ? 1 : 0;
    const BandFp8Scales *Z[2] = {&Z0, &Z1};
    hipLaunchKernelGGL(band_attn_fwd_dual_fp8_kernel<64>, dim3(grid[0] + grid[1]), dim3(256), 4 * (size_t)band_fp8_wave_lds(64), st, P[a], *Z[a], P[a ^ 1],
                       *Z[a ^ 1], grid[a]);
    NSA_LAUNCH_CHECK("band_attn_fwd_dual_fp8");
    return NSA_OK;
}

}  // namespace nsa
