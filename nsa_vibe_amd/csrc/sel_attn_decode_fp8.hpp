// FP8 form of decode_attend_chunks (sel_attn_decode.hpp): the gathered K/V blocks of the selected branch held as OCP e4m3 with one fp32
// scale per (plane, token row) -- half the gather traffic of the bf16 caches.  Q, the partial records, the merge and O are those of the bf16
// form; the arithmetic stays on the bf16 16x16x32 MFMAs (e4m3 is a subset of bf16: the conversion is exact, Q and P keep bf16 precision):
//     x[key] = (K8[key] . q) c2 k_scale[key]          (the scale multiplies the fp32 logit behind the MFMA)
//     P[key] = bf16(exp2(x[key] - m) v_scale[key])    (the scale multiplies the probability before it is rounded to the MFMA operand)
//     l      = sum exp2(x[key] - m)                   (unscaled)
// Same waves per row, chunk-to-wave rule, k-slot of every (key, d) and merge order as the bf16 form: with all scales 1.0f O has the bits of
// the bf16 form on the dequantised caches (tests/test_hip_decode_fp8.py).
// Staging of a 64-key chunk, all of it issued at once (one memory round trip):
//   K   64 rows of D bytes straight to registers in A-fragment shape: lane (rho, q) takes the 8 bytes d = 32 s + 8 q .. + 7 of row 16 u + rho
//       (4 KS global_load_dwordx2, the (u, s, rho, q) -> (key, d) map of the bf16 form at half the width); they stay packed (2 registers per
//       fragment, also for the prefetched next chunk) and are converted right before their MFMA: v_cvt_pk_f32_fp8 + one v_perm_b32 per pair
//       (the upper halves of the two exact floats).
//   scales   the chunk's 64 k_scale and 64 v_scale by two 4-byte LDS-DMA loads (lane i: row min(i, len - 1), so a scale behind the chunk's
//       last key is never read) into 512 bytes behind the V image; read back as four 16-byte reads each in the accumulator's layout
//       (lane (rho, q): keys 16 u + 4 q .. + 3).  (Loaded to registers they would cost 32 VGPRs per chunk in flight.)
//   V   LDS-DMA into the wave's tile at D bytes per row: 4 KiB at D = 64, 8 KiB at D = 128 -- half the tile, the rest stays unused here (the
//       partial record still needs 64 D + 128 bytes).  16-byte column c of row r sits at column c ^ swz8(r), swz8(r) = (r >> 2) & 3 at 64-byte
//       rows, (r >> 1) & 7 at 128-byte rows: the rows of a 256-byte bank window then hold different columns.  The intent is that the rows a
//       transposing read touches per 16-byte column spread over the banks; bank conflicts of these reads have NOT been counted.
//   V^T  ONE ds_read_b64_tr_b8 per (d tile, 32-key half): within a 16-lane group, source lane L supplies 8 bytes of "row" L >> 1, half
//       L & 1, and lane i receives byte i of rows 0 .. 7.  Every lane addresses its row freely, so row j of group q is key 4 q + j (j < 4) or
//       16 + 4 q + j - 4: the eight bytes a lane receives are exactly the k-slots of the bf16 form's paired reads -- no lane movement.
#pragma once
#include "sel_attn_decode.hpp"

namespace nsa {

constexpr int dec_fp8_v_bytes(int D) { return 64 * D; }  // V image of a chunk; the scales sit behind it: k_scale [64] f32 | v_scale [64] f32

// eight e4m3 bytes -> the bf16 fragment of the same eight values, in order (exact)
__device__ __forceinline__ bf16x8 fp8x8_to_bf16(u32x2 raw) {
    u32x4 r;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[w], true);
        r[2 * w] = __builtin_amdgcn_perm(__float_as_uint(lo[1]), __float_as_uint(lo[0]), 0x07060302u);
        r[2 * w + 1] = __builtin_amdgcn_perm(__float_as_uint(hi[1]), __float_as_uint(hi[0]), 0x07060302u);
    }
    return __builtin_bit_cast(bf16x8, r);
}

// a * b as ONE v_mul_f32 (IEEE, what the compiler's own fmul is): the rescale of the O accumulators, kept out of the packed fp32 forms
__device__ __forceinline__ float mul_f32(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// vt, qf_in, kv_row, NC: as decode_attend_chunks.  A.K / A.V: e4m3 bytes, rows D bytes apart (ksb / ksg / vsb / vsg in elements = bytes);
// A.k_scale / A.v_scale: fp32, one per row, rows of a plane contiguous (kzb / kzg / vzb / vzg in elements).  CH::PAGED: the scale pools are
// addressed like K / V -- the plane of the chunk's checked page, row tok0 & 1023.
template <int NW, typename CH, int D = 64>
__device__ __forceinline__ void decode_attend_chunks_fp8(const DecAttnArgs &A, int64_t row, const CH &ch, const int NC, unsigned char *vt, const bf16x8 *qf_in,
                                                         const int64_t kv_row) {
    using T = __bf16;
    using M = MfmaT<T>;
    using x8 = typename M::x8;
    constexpr int KS = D / 32, MT = D / 16;
    constexpr int TILE = dec_att_tile(D);             // the wave's LDS: what the bf16 form and the partial records use
    constexpr int VLD = dec_fp8_v_bytes(D) / 1024;    // LDS-DMA pieces of a V chunk (1 KiB each)
    constexpr int PC = D / 16, VRPI = 64 / PC;        // 16-byte columns of a row; rows of a piece
    constexpr int LOG2D = D == 64 ? 6 : 7;
    static_assert(D == 64 || (D == 128 && NW == 8), "D = 128: eight waves per row");
    constexpr bool PF = NW < 16;  // K rows of the wave's next chunk fetched behind the current one
    constexpr bool PG = CH::PAGED;
    auto swz8 = [](int r) { return D == 64 ? (r >> 2) & 3 : (r >> 1) & 7; };
    int lane = lane_id();
    // (opaque from here: the lane-derived offsets of this phase are formed here, not hoisted above the selector where they would be spilled)
    asm volatile("" : "+v"(lane));
    const int wave = uniform((int)(threadIdx.x >> 6));
    const int rho = lane & 15, q = lane >> 4;
    const int h = A.h;
    const int g = (int)(kv_row % A.G);
    const int64_t b = kv_row / A.G;
    unsigned char *vl = vt + wave * TILE;
    const float *ksl = (const float *)(vl + dec_fp8_v_bytes(D)), *vsl = ksl + 64;

    x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = qf_in[s];

    // (PG: b = 0 -- the planes of pool page 0; a chunk's bases follow from its page)
    const unsigned char *Kb = (const unsigned char *)A.K + b * A.ksb + (int64_t)g * A.ksg;
    const uint64_t va = (uint64_t)((const unsigned char *)A.V + b * A.vsb + (int64_t)g * A.vsg);
    const uint64_t kza = (uint64_t)(A.k_scale + b * A.kzb + (int64_t)g * A.kzg), vza = (uint64_t)(A.v_scale + b * A.vzb + (int64_t)g * A.vzg);
    const int plane_rows = PG ? DEC_PAGE_TOKENS : A.S_kv;
    // a descriptor over `bytes` bytes at a wave-uniform address (the halves through uint32_t: sel_attn_decode.hpp)
    auto rsrc = [](uint64_t a, int bytes) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
        return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | (uint64_t)lo), (short)0, __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
    };
    [[maybe_unused]] const auto vrs0 = rsrc(va, plane_rows * D), kzrs0 = rsrc(kza, plane_rows * 4), vzrs0 = rsrc(vza, plane_rows * 4);

    const int ld_row = lane / PC, ld_piece = lane % PC;
    constexpr int NSW = D == 64 ? 1 : 2;  // D = 128: the swizzle of LDS row VRPI i + ld_row alternates with the parity of i
    uint32_t vsw[NSW];
#pragma unroll
    for (int j = 0; j < NSW; ++j) vsw[j] = (uint32_t)((ld_piece ^ swz8(VRPI * j + ld_row)) << 4);
    uint32_t vrd0[MT];
    {
        const int jj = rho >> 1, r = 4 * q + (jj & 3) + 16 * (jj >> 2);  // the key (inside a 32-key half) of this lane's source row
#pragma unroll
        for (int m = 0; m < MT; ++m) vrd0[m] = r * D + ((m ^ swz8(r)) << 4) + 8 * (rho & 1);
    }

    // the scales, then V, by LDS-DMA (loads complete in order: the scales land first, the logits need them first)
    auto issue_v = [&](int tok0, int len, [[maybe_unused]] int page) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(3))) void lds_void;
        auto vrs = vrs0, kzrs = kzrs0, vzrs = vzrs0;
        int r0 = tok0;
        if constexpr (PG) {
            vrs = rsrc(va + (uint64_t)page * (uint64_t)A.vsb, DEC_PAGE_TOKENS * D);
            kzrs = rsrc(kza + (uint64_t)page * (uint64_t)A.kzb * 4, DEC_PAGE_TOKENS * 4);
            vzrs = rsrc(vza + (uint64_t)page * (uint64_t)A.vzb * 4, DEC_PAGE_TOKENS * 4);
            r0 = tok0 & (DEC_PAGE_TOKENS - 1);
        }
        const int zs = uniform(r0 * 4), zo = min(lane, len - 1) * 4;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(kzrs, (lds_void *)(vl + dec_fp8_v_bytes(D)), 4, zo, zs, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(vzrs, (lds_void *)(vl + dec_fp8_v_bytes(D) + 256), 4, zo, zs, 0, 0);
        const int vs = uniform(r0 * D);
#pragma unroll
        for (int i = 0; i < VLD; ++i) {
            const int rc = min(VRPI * i + ld_row, len - 1);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (lds_void *)(vl + i * 1024), 16, rc * D + vsw[i % NSW], vs, 0, 0);
        }
#else
        (void)tok0, (void)len;
#endif
    };
    auto load_k = [&](int tok0, int len, u32x2 (&k)[4][KS], [[maybe_unused]] int page) {
        const unsigned char *kp = Kb;
        if constexpr (PG) {
            kp = Kb + (int64_t)page * A.ksb;
            tok0 &= DEC_PAGE_TOKENS - 1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kr = tok0 + min(16 * u + rho, len - 1);
#pragma unroll
            for (int s = 0; s < KS; ++s) k[u][s] = *(const u32x2 *)(kp + (int64_t)kr * D + 32 * s + 8 * q);
        }
    };

    f32x4 o[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) o[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float mrun = -INFINITY, lrun = 0.f;

    int cur = dec_first_chunk<NW>(wave, NC), tok0 = 0, len = 0;
    [[maybe_unused]] int pg = 0, npg = 0;
    u32x2 kfr[4][KS];
    if (cur < NC) {
        ch.get(cur, tok0, len);
        if constexpr (PG) pg = ch.page(tok0);
        load_k(tok0, len, kfr, pg);
        issue_v(tok0, len, pg);
    }
    while (cur < NC) {
        const int nxt = dec_next_chunk<NW>(cur, wave, NC);
        const bool hn = nxt < NC;
        int ntok0 = 0, nlen = 0;
        [[maybe_unused]] u32x2 kn[4][KS];
        if (hn) {
            ch.get(nxt, ntok0, nlen);
            if constexpr (PG) npg = ch.page(ntok0);
            if constexpr (PF) load_k(ntok0, nlen, kn, npg);
        }
        f32x4 sacc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sacc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) sacc[u] = M::mma(fp8x8_to_bf16(kfr[u][s]), qf[s], sacc[u]);
        }
        // the scales have landed (the V pieces behind them and the 4 KS prefetched K loads may stay out)
        if (PF && hn) wait_vmcnt<4 * KS + VLD>();
        else wait_vmcnt<VLD>();
        f32x4 kz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) kz[u] = *(const f32x4 *)(ksl + 16 * u + 4 * q);
        float x[16];
        float vmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = (16 * u + 4 * q + j < len) ? (sacc[u][j] * A.c2) * kz[u][j] : -INFINITY;
                x[4 * u + j] = v;
                vmax = fmaxf(vmax, v);
            }
        vmax = xor32_max(xor16_max(vmax));
        const float mnew = fmaxf(mrun, vmax);
        const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
        mrun = mnew;
        float psum = 0.f;
        x8 pf[2];
        f32x4 vz[4];  // (read here, once the K scales are dead: 16 registers less at the loop's widest point)
#pragma unroll
        for (int u = 0; u < 4; ++u) vz[u] = *(const f32x4 *)(vsl + 16 * u + 4 * q);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float pe = __builtin_amdgcn_exp2f(x[i] - mnew);
            psum += pe;
            // a key behind the chunk's end has pe = 0 and an unread scale slot: its P is zero whatever that slot holds
            pf[i >> 3][i & 7] = Elt<T>::from_f((16 * (i >> 2) + 4 * q + (i & 3) < len) ? pe * vz[i >> 2][i & 3] : 0.f);
        }
        lrun = lrun * alpha + psum;
        if (PF && hn) wait_vmcnt<4 * KS>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[m][j] = mul_f32(o[m][j], alpha);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                typedef __attribute__((ext_vector_type(2))) int i32x2;
                const i32x2 raw = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2 *)(vl + vrd0[m] + hf * 32 * D));
                o[m] = M::mma(fp8x8_to_bf16(__builtin_bit_cast(u32x2, raw)), pf[hf], o[m]);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every LDS read of this chunk done before the next chunk's DMA overwrites the tile
        __builtin_amdgcn_sched_barrier(0);
        if (hn) {
            if constexpr (PF) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int s = 0; s < KS; ++s) kfr[u][s] = kn[u][s];
            } else {
                load_k(ntok0, nlen, kfr, npg);
            }
            issue_v(ntok0, nlen, npg);
        }
        cur = nxt;
        tok0 = ntok0;
        len = nlen;
        pg = npg;
    }
    // ---- partial record and merge: those of decode_attend_chunks, value for value and in its order (a copy, so that the bf16 kernels' code
    // does not change with this form)
    const float ltot = xor32_add(xor16_add(lrun));
    float *pm = (float *)vl, *pl = pm + 16, *po = pm + 32;
    if (q == 0) {
        pm[rho] = mrun;
        pl[rho] = ltot;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) *(f32x4 *)(po + rho * D + 16 * m + 4 * q) = o[m];
    __syncthreads();
    for (int tid = threadIdx.x; tid < h * D; tid += NW * 64) {
        const int hh = tid >> LOG2D, d = tid & (D - 1);
        float mm = -INFINITY;
#pragma unroll
        for (int w = 0; w < NW; ++w) mm = fmaxf(mm, ((const float *)(vt + w * TILE))[hh]);
        float acc = 0.f, l = 0.f;
        if (mm > -INFINITY) {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const float *pw = (const float *)(vt + w * TILE);
                const float wgt = __builtin_amdgcn_exp2f(pw[hh] - mm);
                l = fmaf(pw[16 + hh], wgt, l);
                acc = fmaf(pw[32 + hh * D + d], wgt, acc);
            }
        }
        ((T *)A.O)[(row * h + hh) * D + d] = Elt<T>::from_f(l > 0.f ? acc / l : 0.f);
    }
}

}  // namespace nsa
