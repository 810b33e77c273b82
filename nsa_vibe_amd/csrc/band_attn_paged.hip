// nsa_band_attn_fwd_paged: the MFMA band forward (band_attn_mfma.hip has the mapping, band_attn_fwd_body.hpp the body) in its PAGED form --
// the ragged form over pools of pages, the block table in an argument block of its own.  LDS-DMA staging only, in the three forms the
// ragged call runs: split NT = 1, unsplit NT = 1, unsplit NT = 3 (D = 64) / 2 (D = 128).  The dual kernel and the band work carried by the
// decode-step kernels have no paged form.  band_attn_mfma.hip plans the launch (band_plan) and launches the combine pass of the split form.
#include "attn_mfma_tiles.hpp"
#include "band_attn_fwd_body.hpp"

namespace nsa {

template <typename T, int D, int NT, bool SPLIT>
__global__ __launch_bounds__(256, 2) void band_attn_fwd_paged_kernel(BandAttnParams P, BandPageTable PT) {
    band_attn_body<T, D, NT, SPLIT, 1, true, true>(P, blockIdx.x, 4, nullptr, false, &PT);
}

template <typename T, int D>
static void launch_paged_t(const BandAttnParams &P, const BandPageTable &pt, int nt, bool split, unsigned grid, size_t lds, hipStream_t st) {
    constexpr int NTW = D == 64 ? 3 : 2;
    if (split) hipLaunchKernelGGL((band_attn_fwd_paged_kernel<T, D, 1, true>), dim3(grid), dim3(256), lds, st, P, pt);
    else if (nt != NTW) hipLaunchKernelGGL((band_attn_fwd_paged_kernel<T, D, 1, false>), dim3(grid), dim3(256), lds, st, P, pt);
    else hipLaunchKernelGGL((band_attn_fwd_paged_kernel<T, D, NTW, false>), dim3(grid), dim3(256), lds, st, P, pt);
}

void launch_band_attn_paged_kernel(const BandAttnParams &P, const BandPageTable &pt, int dtype, int nt, bool split, unsigned grid, size_t lds, hipStream_t st) {
    with_elt<false>(dtype, [&](auto t) {
        if (P.Dk == 64) launch_paged_t<decltype(t), 64>(P, pt, nt, split, grid, lds, st);
        else launch_paged_t<decltype(t), 128>(P, pt, nt, split, grid, lds, st);
    });
}

}  // namespace nsa
