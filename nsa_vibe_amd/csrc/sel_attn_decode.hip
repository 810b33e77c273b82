// Decode form of the selection attention as its own launch (one 1024-thread workgroup per query row): see sel_attn_decode.hpp.
// Used by the decode routes that do not run the fused scorer+selector+attention kernel (contexts beyond its LDS budget, other
// score geometries, the plain nsa_sel_attn_fwd call with S = 1).
#include "sel_attn_decode.hpp"
#include "nsa_host.hpp"

namespace nsa {

template <typename T, int NW, int D = 64>
__global__ __launch_bounds__(NW * 64, D == 64 ? 4 : 2) void sel_attn_decode_wg_kernel(DecAttnArgs A, const int32_t *__restrict__ ranges) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dlds[];
    const int64_t row = blockIdx.x;
    const int lane = lane_id();
    int rs = 0, re = 0;
    if (threadIdx.x < 64 && lane < A.n) {
        rs = ranges[(row * A.n + lane) * 2];
        re = ranges[(row * A.n + lane) * 2 + 1];
    }
    decode_attend_row<T, NW, D>(A, row, rs, re, dlds);
}

// 16 waves per row while every row can have a CU to itself (all 16 chunks of a selector row in flight at once); beyond that 8 waves
// and 64 KiB of V tiles, so that two rows share a CU and one row's merge / set-up overlaps the other's gather.  The fused decode step
// (sel_decode_fused.hip) follows the same rule: a row's chunks go to the same waves on both routes, and the outputs agree bit for bit.
int dec_att_waves(int64_t rows, int D) {
    if (D == 128) return 8;  // sixteen 16 KiB V tiles do not fit a CU's LDS (sel_attn_decode.hpp)
    const int mode = tuning(TUNE_DECODE_WAVES);
    if (mode == 8 || mode == 16) return mode;
    return rows <= 256 ? 16 : 8;
}

bool sel_attn_decode_wg_shape_ok(int dtype, int h, int Dk, int Dv, int n) {
    if (tuning(TUNE_DECODE_WG) == 0) return false;
    return attn_mfma_shape_ok(dtype, h, Dk, Dv) && n >= 1 && n <= 64;
}

bool sel_attn_decode_wg_supported(const AttnCall &c) {
    return sel_attn_decode_wg_shape_ok(c.dtype, c.h, c.Dk, c.Dv, c.n) && c.vss == c.Dv && qkv_aligned(c);
}

int launch_sel_attn_decode_wg(const SelAttnParams &P, int dtype, hipStream_t st) {
    NSA_CHECK_ARG(P.R >= 1 && P.R < ((int64_t)1 << 31), "sel_attn_decode: bad row count");
    DecAttnArgs A{P.Q, P.K, P.V, P.O, P.G, P.h, P.S_kv, P.n, P.ksb, P.ksg, P.kss, P.vsb, P.vsg, P.vss, P.scale * LOG2E};
    const int nw = dec_att_waves(P.R, P.Dk);
    void (*k)(DecAttnArgs, const int32_t *) = nullptr;
    with_elt<false>(dtype, [&](auto t) {
        using T = decltype(t);
        k = P.Dk == 128 ? sel_attn_decode_wg_kernel<T, 8, 128> : nw == 16 ? sel_attn_decode_wg_kernel<T, 16> : sel_attn_decode_wg_kernel<T, 8>;
    });
    static void *raised[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // raise the dynamic-LDS limit once per kernel (the runtime call costs about a millisecond)
    bool done = false;
    for (void *r : raised) done |= (r == (void *)k);
    if (!done) {
        NSA_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        for (void *&r : raised)
            if (!r) {
                r = (void *)k;
                break;
            }
    }
    hipLaunchKernelGGL(k, dim3((unsigned)P.R), dim3(nw * 64), dec_att_lds(nw, P.Dk), st, A, P.ranges);
    NSA_LAUNCH_CHECK("sel_attn_decode_wg");
    return NSA_OK;
}

}  // namespace nsa
