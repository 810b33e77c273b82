// FP8 form of band_attn_body (band_attn_fwd_body.hpp): the K/V of the sliding and the compressed branch held as OCP e4m3 with one fp32
// scale per (plane, key row) -- half the K/V bytes of the bf16 caches.  A copy beside the bf16 body, as decode_attend_chunks_fp8 stands beside
// decode_attend_chunks: that body is inlined into every decode-step kernel and keeps its code.  Ragged positions always (P.t_pos), bf16 Q / O,
// the stand-alone launch only (no merge through LDS, no gates).  The wave's tokens, slots, 32-key tile partition, split shares, masks, the
// one RESCALE_THR decision per tile, the partial record and the epilogue are the bf16 body's; the arithmetic stays on the bf16 16x16x32 MFMAs
// (e4m3 -> bf16 is exact).  The scales enter where unit scales leave the bf16 body's bits:
//     interior tile   x[key] = fma(K8[key] . q, c2 k_scale[key], -m)          (c2 * 1.0f is c2)
//     slow path       x[key] = (K8[key] . q) (c2 k_scale[key]), -inf outside the slot's [lo, hi)
//     P[key] = bf16(exp2(x[key]) v_scale[key]) inside the slot's interval, +0 outside it -- a select: a scale slot behind a sequence's keys
//              may hold inf;   l = sum exp2(x[key]), unscaled
// Staging of a 32-key tile.  Every address is a lane's own 64-bit one, so a tile that straddles two pages is not a case of its own:
//   K       straight to registers in A-fragment shape: lane (rho, q) takes the 8 bytes d = 32 s + 8 q .. + 7 of row 16 u + rho (2 KS
//           global_load_dwordx2); they stay packed (2 registers per fragment) and are converted right before the tile's first MFMA.  K is wave
//           private in this kernel, so nothing is shared through LDS.  Issued behind the previous tile's QK MFMAs, into the registers those
//           have just read.
//   scales  ONE 4-byte LDS-DMA load: lane i < 32 fetches k_scale of row i, lane 32 + i v_scale of row i, 256 bytes behind the V image; read
//           back as two 16-byte reads each in the accumulator's layout (keys 16 u + 4 q .. + 3).
//   V       LDS-DMA at D bytes per row (2 / 4 loads of 1 KiB) under the swz8 XOR swizzle of sel_attn_decode_fp8.hpp; V^T by ONE
//           ds_read_b64_tr_b8 per d tile with that file's lane -> row map: a lane receives the k-slots of the bf16 form's paired tr_b16 reads.
//   Rows behind the wave's last key (kend - 1) re-read that row and its scales: nothing beyond it is read, in K, V or the scales.
// LDS: a wave needs 32 D + 256 bytes per tile instead of 2 * 64 D.  The space is spent on a SECOND stage (2 * (32 D + 256) = 4.5 / 8.5 KiB per
// wave against 8 / 16 KiB): the DMA of tile i + 1 is issued before tile i is consumed and lands while its MFMAs run; the bf16 body has to wait
// for its fragment reads before it may refill its one stage.
// PAGED: the row and both scales of a key come from the plane of the same checked page id, row r & (page_rows - 1); the verdict over the
// sequence's needed table entries is the bf16 body's, taken once per wave before the first pool read.
#pragma once
#include "attn_mfma_tiles.hpp"
#include "sel_attn_decode_fp8.hpp"

namespace nsa {

constexpr int band_fp8_stage_bytes(int D) { return 32 * D + 256; }  // V image | k_scale [32] f32 | v_scale [32] f32
constexpr int band_fp8_wave_lds(int D) { return 2 * band_fp8_stage_bytes(D); }

// a wave-uniform address pinned in scalar registers (a lane's choice between two of them is then one select per half)
__device__ __forceinline__ uint64_t uniform_u64(uint64_t a) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return ((uint64_t)hi << 32) | lo;
}

template <int D, int NT, bool SPLIT, bool PAGED>
__device__ __forceinline__ void band_attn_body_fp8(const BandAttnParams &P, const BandFp8Scales &Z, const unsigned bid,
                                                   [[maybe_unused]] const BandPageTable *pt) {
    using T = __bf16;
    using M = MfmaT<T>;
    using x8 = typename M::x8;
    using x4 = typename M::x4;
    constexpr int KS = D / 32, MT = D / 16;
    constexpr int STAGE = band_fp8_stage_bytes(D);
    [[maybe_unused]] constexpr int VLD = 32 * D / 1024;  // LDS-DMA loads of a V tile (1 KiB each)
    constexpr int PC = D / 16, VRPI = 64 / PC;  // 16-byte columns of a row; rows of one load
    auto swz8 = [](int r) { return D == 64 ? (r >> 2) & 3 : (r >> 1) & 7; };
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const int wave = uniform((int)(threadIdx.x >> 6));
    const int tpw = P.tpw, h = P.h;
    const int ngrp = (P.S + tpw - 1) / tpw;
    const int nbg = P.B * P.G;
    int bg, grp, sp = 0;
    if (SPLIT) {
        const int64_t wid = (int64_t)bid * 4 + wave;
        const int64_t gi = wid / P.nsplit;
        sp = (int)(wid - gi * P.nsplit);
        bg = (int)(gi / ngrp);
        grp = (int)(gi - (int64_t)bg * ngrp);
        if (bg >= nbg) return;
    } else {
        const int W = (ngrp + 3) >> 2;
        int tc;
        wg_pair(bid, P.map_mode, W, bg, tc);
        grp = 4 * tc + wave;
        if (grp >= ngrp || bg >= nbg) return;
    }
    const int b = bg / P.G, g = bg - b * P.G;
    const int tw0 = grp * tpw, ntok = min(tpw, P.S - tw0);
    unsigned char *vl0 = smem + (size_t)wave * band_fp8_wave_lds(D);

    // ---- key interval of the wave and of every slot; PAGED: the verdict over the sequence's needed table entries (band_attn_fwd_body.hpp)
    BandPos bp = band_pos(P, b);
    [[maybe_unused]] int ent = 0, pg_j0 = 0, pg_jhi = -1;
    if constexpr (PAGED) {
        if (bp.live) {
            const int e = bp.t0 + P.S - P.a;
            const int hi_b = e < 0 ? 0 : e / P.dd + P.c;
            const int lo_b = max(0, band_hi(bp.t0, P.a, P.dd, P.c, P.S_kv, 0) - P.w);
            if (hi_b > lo_b) {
                pg_j0 = uniform(lo_b >> pt->shift), pg_jhi = uniform((hi_b - 1) >> pt->shift);
                const int32_t *row = pt->table + (int64_t)b * pt->stride;
                bool bad = false;
                for (int j = pg_j0; j <= pg_jhi; j += 64) {
                    const int v = j + lane <= pg_jhi ? row[j + lane] : 0;
                    bad |= __any((unsigned)v >= (unsigned)pt->n_pages) != 0;
                    if (j == pg_j0) ent = v;
                }
                if (bad) bp.live = false;
            }
        }
    }
    const int hi_min = band_row_hi(P, bp, tw0);
    const int hi_max = band_row_hi(P, bp, tw0 + ntok - 1);
    const int klo = max(0, hi_min - P.w), lo_max = max(0, hi_max - P.w);
    const int rho = lane & 15, q = lane >> 4;
    int hi_s[NT], lo_s[NT];
    int64_t orow[NT];
    x8 qf[NT][KS];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int slot = 16 * n + rho, tok = slot / h, head = slot - tok * h;
        const bool used = tok < ntok;
        const int t = tw0 + tok;
        hi_s[n] = used ? band_row_hi(P, bp, t) : 0;
        lo_s[n] = max(0, hi_s[n] - P.w);
        orow[n] = used ? ((((int64_t)b * P.S + t) * P.G + g) * h + head) : -1;
        load_col_frags<D>((const T *)P.Q + orow[n] * D, used, q, qf[n]);
    }
    const int kend = min(P.S_kv, hi_max);  // no row from kend on is read: the rows behind a sequence's keys were never written

    // ---- sources.  The planes of a tile's (at most two) pages as wave-uniform 64-bit bases: index 0 the page of the tile's first row, 1 that of
    // its clamped last row; the ragged form has one plane for the whole walk
    // (eight scalars, not arrays: a lane's choice between two of them must stay a select of values)
    uint64_t kb0, kb1, vb0, vb1, kz0, kz1, vz0, vz1;
    auto plane = [&](const void *base, int64_t page, int64_t ps, int64_t gs, int esz) {
        return uniform_u64((uint64_t)((const unsigned char *)base + (page * ps + (int64_t)g * gs) * esz));
    };
    kb0 = kb1 = plane(P.K, PAGED ? 0 : b, P.ksb, P.ksg, 1);
    vb0 = vb1 = plane(P.V, PAGED ? 0 : b, P.vsb, P.vsg, 1);
    kz0 = kz1 = plane(Z.k_scale, PAGED ? 0 : b, Z.kzb, Z.kzg, 4);
    vz0 = vz1 = plane(Z.v_scale, PAGED ? 0 : b, Z.vzb, Z.vzg, 4);
    [[maybe_unused]] auto page_of = [&](int j) {
        if (j - pg_j0 >= 64) {
            pg_j0 = j;
            ent = j + lane <= pg_jhi ? pt->table[(int64_t)b * pt->stride + j + lane] : 0;
        }
        return __builtin_amdgcn_readlane(ent, uniform(j - pg_j0));
    };
    int shift = 31;  // (ragged: every row is "page" 0 of the plane of (b, g))
    [[maybe_unused]] int pg_cur = -1;
    if constexpr (PAGED) shift = pt->shift;
    const int pmask = (int)((1u << shift) - 1u);

    const int ld_row = lane / PC, ld_piece = lane % PC;
    constexpr int NSW = D == 64 ? 1 : 2;  // D = 128: the swizzle of LDS row VRPI i + ld_row alternates with the parity of i
    uint32_t vsw[NSW];
#pragma unroll
    for (int j = 0; j < NSW; ++j) vsw[j] = (uint32_t)((ld_piece ^ swz8(VRPI * j + ld_row)) << 4);
    uint32_t vrd0[MT];
    {
        const int jj = rho >> 1, r = 4 * q + (jj & 3) + 16 * (jj >> 2);  // the key of this lane's source row of the transposing read
#pragma unroll
        for (int m = 0; m < MT; ++m) vrd0[m] = r * D + ((m ^ swz8(r)) << 4) + 8 * (rho & 1);
    }
    // the planes of the tile at tok0 (PAGED: of the page of its first row and of its clamped last row; both are checked entries)
    auto tile_planes = [&](int tok0) {
        if constexpr (PAGED) {
            const int j0 = uniform(tok0 >> shift), j1 = uniform((tok0 + min(31, kend - 1 - tok0)) >> shift);
            if (j0 != pg_cur) {
                const int pg = page_of(j0);
                kb0 = plane(P.K, pg, P.ksb, P.ksg, 1), vb0 = plane(P.V, pg, P.vsb, P.vsg, 1);
                kz0 = plane(Z.k_scale, pg, Z.kzb, Z.kzg, 4), vz0 = plane(Z.v_scale, pg, Z.vzb, Z.vzg, 4);
                pg_cur = j0;
            }
            const int pg = page_of(j1);
            kb1 = plane(P.K, pg, P.ksb, P.ksg, 1), vb1 = plane(P.V, pg, P.vsb, P.vsg, 1);
            kz1 = plane(Z.k_scale, pg, Z.kzb, Z.kzg, 4), vz1 = plane(Z.v_scale, pg, Z.vzb, Z.vzg, 4);
        }
    };
    // row `r` of the tile (clamped to the wave's last key) -> (second page?, byte-free row index inside its plane)
    auto plane_row = [&](int tok0, int r, bool &second) {
        const int abs_row = tok0 + min(r, kend - 1 - tok0);
        second = (abs_row >> shift) != (tok0 >> shift);
        return (uint32_t)(abs_row & pmask);
    };
    // the scales, then V, of the tile at tok0 into the stage at vl by LDS-DMA (loads complete in order; completion is a vmcnt event)
    auto issue_v = [&](int tok0, unsigned char *vl) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(3))) void lds_void;
        typedef const __attribute__((address_space(1))) void gbl_void;
        bool sec;
        const uint32_t zr = plane_row(tok0, lane & 31, sec);
        const uint64_t zk = sec ? kz1 : kz0, zv = sec ? vz1 : vz0, zb = lane < 32 ? zk : zv;
        __builtin_amdgcn_global_load_lds((gbl_void *)(zb + zr * 4u), (lds_void *)(vl + 32 * D), 4, 0, 0);
#pragma unroll
        for (int i = 0; i < VLD; ++i) {
            const uint32_t vr = plane_row(tok0, VRPI * i + ld_row, sec);
            __builtin_amdgcn_global_load_lds((gbl_void *)((sec ? vb1 : vb0) + (vr * (uint32_t)D + vsw[i % NSW])), (lds_void *)(vl + i * 1024), 16, 0, 0);
        }
#else
        (void)tok0, (void)vl;
#endif
    };
    auto load_k = [&](int tok0, u32x2 (&k)[2][KS]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bool sec;
            const uint32_t kr = plane_row(tok0, 16 * u + rho, sec);
            const unsigned char *kp = (const unsigned char *)((sec ? kb1 : kb0) + (kr * (uint32_t)D + 8 * q));
#pragma unroll
            for (int s = 0; s < KS; ++s) k[u][s] = *(const u32x2 *)(kp + 32 * s);
        }
    };

    f32x4 o[NT][MT];
    float mrun[NT], lrun[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int m = 0; m < MT; ++m) o[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
        mrun[n] = orow[n] >= 0 ? -INFINITY : INFINITY;  // unused slots: their (zero) scores never trigger the max-raising path
        lrun[n] = 0.f;
    }
    const float c2 = P.scale * LOG2E;

    const int ntile_all = hi_max > klo ? (hi_max - klo + 31) >> 5 : 0;
    int tile = 0, tile_end = ntile_all;
    if (SPLIT) {
        tile = (int)(((int64_t)ntile_all * sp) / P.nsplit);
        tile_end = (int)(((int64_t)ntile_all * (sp + 1)) / P.nsplit);
    }
    u32x2 k8[2][KS];
    int st = 0;  // the stage of the tile being consumed
    if (tile < tile_end) {
        tile_planes(klo + 32 * tile);
        issue_v(klo + 32 * tile, vl0);
        load_k(klo + 32 * tile, k8);
    }

    for (; tile < tile_end; ++tile, st ^= 1) {
        const int tok0 = klo + 32 * tile;
        const unsigned char *vl = vl0 + uniform(st * STAGE);
        const bool more = tile + 1 < tile_end;
        wait_vmcnt<0>();  // this tile's scales and V have landed (its K registers with them)
        // tile i + 1 on its way into the other stage: its last reader, tile i - 1, drained lgkmcnt at the foot of its iteration
        if (more) {
            tile_planes(tok0 + 32);
            issue_v(tok0 + 32, vl0 + uniform((st ^ 1) * STAGE));
        }
        const bool interior = tok0 >= lo_max && tok0 + 32 <= hi_min;  // every key valid for every used slot
        f32x4 sacc[NT][2];
#pragma unroll
        for (int n = 0; n < NT; ++n) sacc[n][0] = sacc[n][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // one K fragment converted at a time and used by all NT column tiles (every accumulator still sums its k-steps in order)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const x8 kf = fp8x8_to_bf16(k8[u][s]);
#pragma unroll
                for (int n = 0; n < NT; ++n) sacc[n][u] = M::mma(kf, qf[n][s], sacc[n][u]);
            }
        if (more) load_k(tok0 + 32, k8);  // into the registers the MFMAs above have read
        // key of sacc[n][u][j] = tok0 + 16u + 4q + j; its logit scale c2 k_scale[key]
        f32x4 kc[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 kz = *(const f32x4 *)(vl + 32 * D + 4 * (16 * u + 4 * q));
#pragma unroll
            for (int j = 0; j < 4; ++j) kc[u][j] = c2 * kz[j];
        }
        float x[NT][8];
        float tmax = -INFINITY;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) x[n][4 * u + j] = fmaf(sacc[n][u][j], kc[u][j], -mrun[n]);
            tmax = fmaxf(tmax, fmaxf(fmaxf(fmaxf(x[n][0], x[n][1]), fmaxf(x[n][2], x[n][3])),
                                     fmaxf(fmaxf(x[n][4], x[n][5]), fmaxf(x[n][6], x[n][7]))));
        }
        if (!interior || __any(!(tmax <= RESCALE_THR))) {
            asm volatile("; slow path: masks and/or raise the running max" ::: "memory");
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                float vmax = -INFINITY;
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int key = tok0 + 16 * u + 4 * q + j;
                        const float v = (key >= lo_s[n] && key < hi_s[n]) ? sacc[n][u][j] * kc[u][j] : -INFINITY;
                        x[n][4 * u + j] = v;
                        vmax = fmaxf(vmax, v);
                    }
                vmax = fmaxf(vmax, __shfl_xor(vmax, 16, 64));
                vmax = fmaxf(vmax, __shfl_xor(vmax, 32, 64));
                const float mnew = fmaxf(mrun[n], vmax);
                const float msub = (mnew == -INFINITY) ? 0.f : mnew;
                const float alpha = (mnew == mrun[n]) ? 1.f : __builtin_amdgcn_exp2f(mrun[n] - msub);
                mrun[n] = mnew;
                lrun[n] *= alpha;
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[n][m][j] = mul_f32(o[n][m][j], alpha);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[n][j] -= msub;
            }
        }
        f32x4 vz[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) vz[u] = *(const f32x4 *)(vl + 32 * D + 128 + 4 * (16 * u + 4 * q));
        typedef __attribute__((ext_vector_type(2))) int i32x2;
        i32x2 v8[MT];  // V^T fragments, packed: converted one at a time below
#pragma unroll
        for (int m = 0; m < MT; ++m) v8[m] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2 *)(vl + vrd0[m]));
        // P = bf16(pe v_scale) inside the slot's interval and +0 outside it, by a select: there pe is 0 and the scale slot may hold anything.
        // edge (a tile on a window edge or the diagonal): per key; else every key is valid for every used slot, and the select is per slot
        x8 pf[NT];
        auto probs = [&](auto edge) {
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                float psum = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float pe = __builtin_amdgcn_exp2f(x[n][j]);
                    psum += pe;
                    const int key = tok0 + 16 * (j >> 2) + 4 * q + (j & 3);
                    const bool in = decltype(edge)::value ? (key >= lo_s[n] && key < hi_s[n]) : orow[n] >= 0;
                    pf[n][j] = Elt<T>::from_f(in ? pe * vz[j >> 2][j & 3] : 0.f);
                }
                lrun[n] += psum;
            }
        };
        if (interior) probs(std::false_type{});
        else probs(std::true_type{});
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const x8 va = fp8x8_to_bf16(__builtin_bit_cast(u32x2, v8[m]));
#pragma unroll
            for (int n = 0; n < NT; ++n) o[n][m] = M::mma(va, pf[n], o[n][m]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every LDS read of this stage done before the DMA of tile i + 2 refills it
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue: the bf16 body's record / output row, value for value
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        float ltot = lrun[n] + __shfl_xor(lrun[n], 16, 64);
        ltot += __shfl_xor(ltot, 32, 64);
        if (orow[n] < 0) continue;
        if (SPLIT) {
            const int64_t row = orow[n] / h;
            const int head = (int)(orow[n] - row * h);
            float *pr = P.part + ((row * P.nsplit + sp) * (int64_t)h + head) * (D + PART_PAD);
            if (q == 0) {
                pr[0] = mrun[n];
                pr[1] = ltot;
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) *(f32x4 *)(pr + PART_PAD + 16 * m + 4 * q) = o[n][m];
        } else {
            const float inv = ltot > 0.f ? 1.f / ltot : 0.f;
            T *Or = (T *)P.O + orow[n] * D;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                x4 ov;
#pragma unroll
                for (int j = 0; j < 4; ++j) ov[j] = Elt<T>::from_f(o[n][m][j] * inv);
                *(x4 *)(Or + 16 * m + 4 * q) = ov;
            }
            if (P.lse && q == 0) P.lse[orow[n]] = ltot > 0.f ? (mrun[n] + __builtin_amdgcn_logf(ltot)) * LN2 : -INFINITY;
        }
    }
}

}  // namespace nsa
