// MFMA band attention forward for gfx950 (bf16 / f16, Dk = Dv in {64, 128}, h <= 16): the sliding-window and the compressed
// branch of NSA (reference: sliding_window_attention, nsa/core/attention_kernels.py:146-178; compressed branch with the
// num_cmp(t) emission schedule, :106-143).  Query row t attends the contiguous key interval [lo(t), hi(t)) defined in
// sel_attn_params.hpp (BandAttnParams); rows with an empty interval give zeros.
//
// Mapping: one wave64 = TPW consecutive tokens of one (b,g) with all their h heads: NT*16 (token, head) "slots" are the
// columns of NT 16x16x32 MFMA tiles (h = 6, NT = 3: 8 tokens x 6 heads = 48 slots, every column used).  A K/V tile of 32
// keys is brought into wave-private LDS once (LDS-DMA) and its fragments are reused by all NT column tiles, so the band
// around TPW tokens costs (w + TPW) key rows per wave instead of w per token.  The product is computed transposed like
// the selection kernel (S^T = K.Q^T, O^T += V^T.P^T): softmax statistics are per lane (= per slot) and the S^T
// accumulators feed the PV MFMA without any lane movement.  Tiles that lie inside every slot's interval take the
// mask-free path with deferred max; only the tiles on the window edge / causal diagonal apply per-slot masks.
// A 256-thread workgroup = 4 consecutive token groups; all LDS is wave private (no workgroup barrier).
#include <stdlib.h>

#include "attn_mfma_tiles.hpp"
#include "band_attn_fwd_body.hpp"

namespace nsa {

template <typename T, int D, int NT, bool SPLIT, int STAGE, bool RAGGED = false>
__global__ __launch_bounds__(256, 2) void band_attn_fwd_kernel(BandAttnParams P) {
    band_attn_body<T, D, NT, SPLIT, STAGE, RAGGED>(P, blockIdx.x);
}

// decode: the sliding and the compressed branch of one step in ONE launch (two argument blocks, split-KV form)
// RAGGED: both blocks carry the same position array (the layer's ragged call); a sequence that is not live leaves the empty-interval
// records (m = -inf, l = 0, o = 0) the finish kernel turns into zero rows, as a row too short for a compressed token does today
template <typename T, int D, bool RAGGED = false>
__global__ __launch_bounds__(256, 2) void band_attn_fwd_dual_kernel(BandAttnParams P0, BandAttnParams P1, unsigned grid0) {
    if (blockIdx.x < grid0) band_attn_body<T, D, 1, true, 1, RAGGED>(P0, blockIdx.x);
    else band_attn_body<T, D, 1, true, 1, RAGGED>(P1, blockIdx.x - grid0);
}

// ------------------------------------------------------------------------------------------------------------------------
// Backward, dQ: the same 48-slot query-major walk as the forward.  P is recomputed from the forward's log-sum-exp, so there is
// no running max: per key tile  S^T = K.Q^T,  dP^T = V.dO^T,  dS^T = P^T o (dP^T - delta) * scale  (delta per slot = per lane
// column),  dQ^T[d, slot] += K^T[d x keys] . dS^T  -- dS^T goes from the accumulators straight into the B operand, K^T comes
// from a second LDS image of the K tile (transposing reads), V is staged in the row layout.  dK / dV of the band are taken
// by the key-block-major selection backward kernel (the band written as one range per row).
// ------------------------------------------------------------------------------------------------------------------------
struct BandBwdExtra {
    const void *dO;      // [B,S,G,h,D]
    const float *lse;    // [B,S,G,h]  natural-log log-sum-exp of the forward (-inf: empty row)
    const float *delta;  // [B,S,G,h]  rowsum(dO * O)
    void *dQ;            // [B,S,G,h,D]
};

// D = 128 (NT = 1): K is staged ONCE, in the chunk-swizzled image of the transposing reads; its b128 row-fragment reads are bank-conflict
// free too (see sel_attn_bwd_mfma.hip, BGeo), so a wave needs 2 x 8 KiB of LDS instead of 3 x 8 KiB and two workgroups fit a CU
template <int D>
constexpr int band_dq_wave_lds() {
    return (D == 64 ? 3 : 2) * Geo<D>::TILE_BYTES;
}

template <typename T, int D, int NT>
__global__ __launch_bounds__(256, 2) void band_attn_bwd_dq_kernel(BandAttnParams P, BandBwdExtra E) {
    using M = MfmaT<T>;
    using G_ = Geo<D>;
    using x8 = typename M::x8;
    using x4 = typename M::x4;
    constexpr int KS = G_::KSTEPS, MT = G_::MT;
    constexpr bool ONE_K = D == 128;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const int wave = uniform((int)(threadIdx.x >> 6));
    const int tpw = P.tpw, h = P.h;
    const int ngrp = (P.S + tpw - 1) / tpw;
    const int nbg = P.B * P.G;
    const int W = (ngrp + 3) >> 2;
    int bg, tc;
    wg_pair(blockIdx.x, P.map_mode, W, bg, tc);
    const int grp = 4 * tc + wave;
    if (grp >= ngrp || bg >= nbg) return;
    const int b = bg / P.G, g = bg - b * P.G;
    const int tw0 = grp * tpw, ntok = min(tpw, P.S - tw0);
    unsigned char *kl = smem + (size_t)wave * band_dq_wave_lds<D>();  // K rows | K transposable | V rows (ONE_K: K transposable | V rows)
    unsigned char *ktl = ONE_K ? kl : kl + G_::TILE_BYTES, *vl = ktl + G_::TILE_BYTES;

    const int hi_min = band_hi(P.t0, P.a, P.dd, P.c, P.S_kv, tw0);
    const int hi_max = band_hi(P.t0, P.a, P.dd, P.c, P.S_kv, tw0 + ntok - 1);
    const int klo = max(0, hi_min - P.w), lo_max = max(0, hi_max - P.w);
    const int rho = lane & 15, q = lane >> 4;
    int hi_s[NT], lo_s[NT];
    int64_t orow[NT];
    float lse2[NT], dlt[NT];
    x8 qf[NT][KS], dof[NT][KS];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int slot = 16 * n + rho, tok = slot / h, head = slot - tok * h;
        const bool used = tok < ntok;
        const int t = tw0 + tok;
        hi_s[n] = used ? band_hi(P.t0, P.a, P.dd, P.c, P.S_kv, t) : 0;
        lo_s[n] = max(0, hi_s[n] - P.w);
        orow[n] = used ? ((((int64_t)b * P.S + t) * P.G + g) * h + head) : -1;
        const float l = used ? E.lse[orow[n]] : -INFINITY;
        lse2[n] = l > -INFINITY ? l * LOG2E : INFINITY;  // empty / unused slot: exp2(s - inf) = 0
        dlt[n] = used ? E.delta[orow[n]] : 0.f;
        load_col_frags<D>((const T *)P.Q + orow[n] * D, used, q, qf[n]);
        load_col_frags<D>((const T *)E.dO + orow[n] * D, used, q, dof[n]);
    }

    [[maybe_unused]] const KvSrc<D> kv = kv_src<T, D>(P, b, g, lane);  // (the host pass sees no use: the DMA builtin is device only)
    // V is read as row fragments (A operand of dP^T), K as transposed ones and as row fragments: from its own row image, or (ONE_K) from the transposable one
    uint32_t krd0[KS], vrd0[KS], trd0[MT];
    frag_read_offsets<D>(rho, q, vrd0, trd0);
#pragma unroll
    for (int s = 0; s < KS; ++s) krd0[s] = ONE_K ? rho * G_::ROWB + G_::tr_piece(rho, 4 * s + q) : vrd0[s];
    // one 32-key tile -> three wave-private images (rows past the end of K/V re-read the last row; they are masked)
    auto issue_dma = [&](int tok0) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(3))) void lds_void;
        const int ks = uniform(tok0 * kv.krowb), vs = uniform(tok0 * kv.vrowb);
        const int last = P.S_kv - 1 - tok0;
#pragma unroll
        for (int i = 0; i < G_::NLD; ++i) {
            const int r = i * G_::RPI + kv.ld_row;
            const int rc = min(r, last);
            const uint32_t pk = G_::row_piece(r, kv.ld_piece), pt = G_::tr_piece(r, kv.ld_piece);
            if constexpr (!ONE_K) __builtin_amdgcn_raw_ptr_buffer_load_lds(kv.krs, (lds_void *)(kl + i * 1024), 16, rc * kv.krowb + pk, ks, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(kv.krs, (lds_void *)(ktl + i * 1024), 16, rc * kv.krowb + pt, ks, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(kv.vrs, (lds_void *)(vl + i * 1024), 16, rc * kv.vrowb + pk, vs, 0, 0);
        }
#else
        (void)tok0;
#endif
    };

    f32x4 dq[NT][MT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int m = 0; m < MT; ++m) dq[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float c2 = P.scale * LOG2E;
    const int ntile = hi_max > klo ? (hi_max - klo + 31) >> 5 : 0;
    if (ntile > 0) issue_dma(klo);
    for (int tile = 0; tile < ntile; ++tile) {
        const int tok0 = klo + 32 * tile;
        x8 kfr[2][KS], vfr[2][KS], ka[MT];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int s = 0; s < KS; ++s) {  // (K and V interleaved: the order the loop's schedule was measured with)
                kfr[u][s] = *(const x8 *)(kl + krd0[s] + u * 16 * G_::ROWB);
                vfr[u][s] = *(const x8 *)(vl + vrd0[s] + u * 16 * G_::ROWB);
            }
        read_tr_frags<T, D>(ktl, trd0, ka);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (tile + 1 < ntile) issue_dma(tok0 + 32);
        const bool interior = tok0 >= lo_max && tok0 + 32 <= hi_min;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            f32x4 sacc[2], dpacc[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                sacc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
                dpacc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    sacc[u] = M::mma(kfr[u][s], qf[n][s], sacc[u]);
                    dpacc[u] = M::mma(vfr[u][s], dof[n][s], dpacc[u]);
                }
            }
            x8 dsf;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float p = __builtin_amdgcn_exp2f(fmaf(sacc[u][j], c2, -lse2[n]));
                    if (!interior) {  // wave uniform: only the window-edge / diagonal tiles pay for the masks
                        const int key = tok0 + 16 * u + 4 * q + j;
                        p = (key >= lo_s[n] && key < hi_s[n]) ? p : 0.f;
                    }
                    dsf[4 * u + j] = Elt<T>::from_f(p * (dpacc[u][j] - dlt[n]) * P.scale);
                }
#pragma unroll
            for (int m = 0; m < MT; ++m) dq[n][m] = M::mma(ka[m], dsf, dq[n][m]);
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        if (orow[n] < 0) continue;
        T *dst = (T *)E.dQ + orow[n] * D;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            x4 ov;
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = Elt<T>::from_f(dq[n][m][j]);
            *(x4 *)(dst + 16 * m + 4 * q) = ov;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------
// NT = 3 column tiles per wave (48 / h tokens) once there are enough tokens to fill the chip, NT = 1 (16 / h tokens)
// below that; with very few token groups (decode) the key interval is also split over several waves.
// (D = 128: 2 column tiles, the accumulators are twice as wide)
static void band_plan(int B, int S, int G, int h, int D, int *nt, int *tpw, int *nsplit) {
    const int ntw = D == 64 ? 3 : 2;
    const int tpw3 = 16 * ntw / h, tpw1 = 16 / h;
    const int64_t grp3 = (int64_t)B * G * ((S + tpw3 - 1) / tpw3);
    if (grp3 >= 2048) {
        *nt = ntw, *tpw = tpw3, *nsplit = 1;
        return;
    }
    *nt = 1, *tpw = tpw1;
    const int64_t grp1 = (int64_t)B * G * ((S + tpw1 - 1) / tpw1);
    int ns = 1;
    if (grp1 < 1024) {
        ns = (int)((2048 + grp1 - 1) / grp1);
        if (ns > 16) ns = 16;
    }
    *nsplit = ns;
}

size_t band_attn_workspace(int B, int S, int G, int h, int Dk, int Dv, int dtype, int *nsplit_out) {
    int nt = 1, tpw = 1, ns = 1;
    if (attn_mfma_shape_ok(dtype, h, Dk, Dv)) band_plan(B, S, G, h, Dk, &nt, &tpw, &ns);
    if (nsplit_out) *nsplit_out = ns;
    return ns > 1 ? (size_t)B * S * G * ns * h * (Dv + PART_PAD) * sizeof(float) : 0;
}

template <typename T, int D>
static int launch_band_t(const BandAttnParams &P0, hipStream_t st, const BandPageTable *pt) {
    constexpr int dtype = std::is_same<T, __bf16>::value ? NSA_DT_BF16 : NSA_DT_F16;
    BandAttnParams P = P0;
    int nt = 1, ns = 1;
    band_plan(P.B, P.S, P.G, P.h, D, &nt, &P.tpw, &ns);
    const bool split = ns > 1 && P.part != nullptr && P.nsplit == ns;
    if (!split) P.nsplit = 1;
    const int64_t nbg = (int64_t)P.B * P.G;
    const int ngrp = (P.S + P.tpw - 1) / P.tpw;
    const size_t lds = 4 * (size_t)(2 * Geo<D>::TILE_BYTES);
    const bool ragged = P.t_pos != nullptr;  // per-sequence positions: the RAGGED instantiations (LDS-DMA staging only)
    if (split) {
        const int64_t waves = nbg * ngrp * P.nsplit;
        // pt: the paged form -- the same plan and geometry, the PAGED kernels of band_attn_paged.hip (a translation unit of their own)
        if (pt) launch_band_attn_paged_kernel(P, *pt, dtype, 1, true, (unsigned)((waves + 3) / 4), lds, st);
        else if (ragged) hipLaunchKernelGGL((band_attn_fwd_kernel<T, D, 1, true, 1, true>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, st, P);
        else hipLaunchKernelGGL((band_attn_fwd_kernel<T, D, 1, true, 1>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, st, P);
        NSA_LAUNCH_CHECK("band_attn_fwd(split)");
        if (P.defer_combine) return NSA_OK;
        SelAttnParams C{};
        C.O = P.O;
        C.lse = P.lse;
        C.R = nbg * P.S;
        C.h = P.h;
        C.part = P.part;
        C.nsplit = P.nsplit;
        hipLaunchKernelGGL((sel_attn_combine_kernel<T, D>), dim3((unsigned)((C.R * C.h + 3) / 4)), dim3(256), 0, st, C);
        NSA_LAUNCH_CHECK("band_attn_combine");
        return NSA_OK;
    }
    const int64_t W = (ngrp + 3) / 4;
    P.map_mode = (nbg % 8 == 0) ? 2 : 1;
    NSA_CHECK_ARG(nbg * W < ((int64_t)1 << 31), "band_attn: too many workgroups for one launch");
    const unsigned grid = (unsigned)(nbg * W);
    const int stage = tuning(TUNE_BAND_STAGE);  // A/B switch: 0 = register staging, 1 = LDS-DMA  // measured: LDS-DMA 750 vs register staging 650 TFLOP/s (compressed branch, 64k)
    constexpr int NTW = D == 64 ? 3 : 2;
    if (pt) launch_band_attn_paged_kernel(P, *pt, dtype, nt, false, grid, lds, st);
    else if (ragged && nt != NTW) hipLaunchKernelGGL((band_attn_fwd_kernel<T, D, 1, false, 1, true>), dim3(grid), dim3(256), lds, st, P);
    else if (ragged) hipLaunchKernelGGL((band_attn_fwd_kernel<T, D, NTW, false, 1, true>), dim3(grid), dim3(256), lds, st, P);
    else if (nt != NTW) hipLaunchKernelGGL((band_attn_fwd_kernel<T, D, 1, false, 1>), dim3(grid), dim3(256), lds, st, P);
    else if (D == 128 || stage != 0) hipLaunchKernelGGL((band_attn_fwd_kernel<T, D, NTW, false, 1>), dim3(grid), dim3(256), lds, st, P);
    else if constexpr (D == 64) hipLaunchKernelGGL((band_attn_fwd_kernel<T, D, NTW, false, 0>), dim3(grid), dim3(256), lds, st, P);  // (register staging: D = 64 only)
    NSA_LAUNCH_CHECK("band_attn_fwd");
    return NSA_OK;
}

int launch_band_attn_fwd_mfma(const BandAttnParams &P, int dtype, hipStream_t st, const BandPageTable *pt) {
    NSA_CHECK_ARG(!pt || P.t_pos, "band_attn: the paged form takes per-sequence positions");
    return with_elt<false>(dtype, [&](auto t) { return P.Dk == 64 ? launch_band_t<decltype(t), 64>(P, st, pt) : launch_band_t<decltype(t), 128>(P, st, pt); });
}

// Both branches of a decode step in one launch.  Requires both to be in split form with deferred combine (the caller combines).
bool band_dual_plan(BandAttnParams *P0, BandAttnParams *P1, int dtype, int64_t waves[2]) {
    BandAttnParams *P[2] = {P0, P1};
    for (int i = 0; i < 2; ++i) {
        int nt = 1, ns = 1;
        band_plan(P[i]->B, P[i]->S, P[i]->G, P[i]->h, P[i]->Dk, &nt, &P[i]->tpw, &ns);
        if (!(nt == 1 && ns > 1 && P[i]->part && P[i]->nsplit == ns && P[i]->defer_combine)) return false;
        waves[i] = (int64_t)P[i]->B * P[i]->G * ((P[i]->S + P[i]->tpw - 1) / P[i]->tpw) * ns;
    }
    return P0->Dk == P1->Dk && attn_mfma_shape_ok(dtype, P0->h, P0->Dk, P0->Dv);
}

int launch_band_attn_fwd_dual(const BandAttnParams &A0, const BandAttnParams &A1, int dtype, hipStream_t st) {
    BandAttnParams P[2] = {A0, A1};
    int64_t waves[2];
    NSA_CHECK_ARG(band_dual_plan(&P[0], &P[1], dtype, waves), "band dual launch: both branches in split form with deferred combine, one supported shape");
    const unsigned grid[2] = {(unsigned)((waves[0] + 3) / 4), (unsigned)((waves[1] + 3) / 4)};
    const bool d64 = P[0].Dk == 64;
    const size_t lds = 4 * (size_t)(2 * (d64 ? Geo<64>::TILE_BYTES : Geo<128>::TILE_BYTES));
    const dim3 g2(grid[0] + grid[1]);
    const bool ragged = P[0].t_pos != nullptr;  // per-sequence positions: the RAGGED instantiation
    NSA_CHECK_ARG(P[0].t_pos == P[1].t_pos && (!ragged || P[0].t_max == P[1].t_max), "band dual launch: one position array for both branches");
    with_elt<false>(dtype, [&](auto t) {
        if (ragged && d64) hipLaunchKernelGGL((band_attn_fwd_dual_kernel<decltype(t), 64, true>), g2, dim3(256), lds, st, P[0], P[1], grid[0]);
        else if (ragged) hipLaunchKernelGGL((band_attn_fwd_dual_kernel<decltype(t), 128, true>), g2, dim3(256), lds, st, P[0], P[1], grid[0]);
        else if (d64) hipLaunchKernelGGL((band_attn_fwd_dual_kernel<decltype(t), 64>), g2, dim3(256), lds, st, P[0], P[1], grid[0]);
        else hipLaunchKernelGGL((band_attn_fwd_dual_kernel<decltype(t), 128>), g2, dim3(256), lds, st, P[0], P[1], grid[0]);
    });
    NSA_LAUNCH_CHECK("band_attn_fwd_dual");
    return NSA_OK;
}

// dQ of the band (bf16/f16, Dk = Dv = 64 or 128).  delta = rowsum(dO * O) [B,S,G,h] fp32 comes from the caller.
template <typename T, int D>
static int launch_band_dq_t(BandAttnParams P, const BandBwdExtra &E, hipStream_t st) {
    // 48 slots per wave when there are enough token groups, else 16.  D = 128: always 16 -- at 32 (NT = 2, the forward's form) the dQ
    // accumulators, Q / dO fragments and K / V tile fragments need more than 256 registers (the compiler spilled 308 B per lane)
    constexpr int NTW = D == 64 ? 3 : 1;
    const int tpw3 = 16 * NTW / P.h, tpw1 = 16 / P.h;
    const int64_t nbg = (int64_t)P.B * P.G;
    const bool big = nbg * ((P.S + tpw3 - 1) / tpw3) >= 2048;
    P.tpw = big ? tpw3 : tpw1;
    const int ngrp = (P.S + P.tpw - 1) / P.tpw;
    const int64_t W = (ngrp + 3) / 4;
    P.map_mode = (nbg % 8 == 0) ? 2 : 1;
    NSA_CHECK_ARG(nbg * W < ((int64_t)1 << 31), "band_attn_bwd: too many workgroups for one launch");
    const size_t lds = 4 * (size_t)band_dq_wave_lds<D>();  // 48 KiB (D = 64), 64 KiB (D = 128)
    if (big) hipLaunchKernelGGL((band_attn_bwd_dq_kernel<T, D, NTW>), dim3((unsigned)(nbg * W)), dim3(256), lds, st, P, E);
    else hipLaunchKernelGGL((band_attn_bwd_dq_kernel<T, D, 1>), dim3((unsigned)(nbg * W)), dim3(256), lds, st, P, E);
    NSA_LAUNCH_CHECK("band_attn_bwd_dq");
    return NSA_OK;
}

int launch_band_attn_bwd_dq(const BandAttnParams &P, const void *dO, const float *lse, const float *delta, void *dQ, int dtype,
                            hipStream_t st) {
    BandBwdExtra E{dO, lse, delta, dQ};
    return with_elt<false>(dtype, [&](auto t) { return P.Dk == 64 ? launch_band_dq_t<decltype(t), 64>(P, E, st) : launch_band_dq_t<decltype(t), 128>(P, E, st); });
}

}  // namespace nsa
