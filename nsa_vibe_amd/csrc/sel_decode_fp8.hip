// The FP8 K/V instantiations of the one-launch decode step (decode_step_kernel<..., FP8 = true>, sel_decode_step.hpp; the gather is
// decode_attend_chunks_fp8, sel_attn_decode_fp8.hpp): what nsa_sel_decode_ragged_fp8 and nsa_sel_decode_paged_fp8 launch.  bf16 queries,
// the rows form over per-sequence positions, unsplit forms 0 and 1 (D = 128: form 0 on eight waves), group size 6 or any h <= 16, ragged or
// paged caches: 20 kernels.  A translation unit of its own, as band_attn_paged.hip is: the module of sel_decode_fused.hip stays what it was.
#include "sel_decode_step.hpp"

namespace nsa {

template <int NW, int HC, int CPW, int D>
static DecStepKernel fp8_kernel(bool paged) {
    if (paged) return decode_step_kernel<__bf16, NW, false, HC, CPW, D, true, true, false, true>;
    return decode_step_kernel<__bf16, NW, false, HC, CPW, D, true, false, false, true>;
}
template <int NW, int CPW, int D>
static DecStepKernel fp8_kernel(int hc, bool paged) {
    return hc == 6 ? fp8_kernel<NW, 6, CPW, D>(paged) : fp8_kernel<NW, 0, CPW, D>(paged);
}

DecStepKernel dstep_kernel_fp8(int nw, int hc, int cpw, int D, bool paged) {
    if (nw != 16 && nw != 8) return nullptr;
    if (D == 128) return nw == 8 && cpw == 2 ? fp8_kernel<8, 2, 128>(hc, paged) : nullptr;
    if (D != 64) return nullptr;
    if (nw == 16) return cpw == 2 ? fp8_kernel<16, 2, 64>(hc, paged) : fp8_kernel<16, 4, 64>(hc, paged);
    return cpw == 2 ? fp8_kernel<8, 2, 64>(hc, paged) : fp8_kernel<8, 4, 64>(hc, paged);
}

}  // namespace nsa
