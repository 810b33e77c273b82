// MFMA backward of the selection attention for gfx950 (bf16 / f16, Dk = Dv = D in {64, 128}, h <= 16).
//
// Reference: autograd of the masked SDPA (nsa/core/attention_kernels.py:705-772); the structure of the reference's
// analytic backward (nsa/kernels/triton_sel_kernel/__init__.py:163-231: recompute P, dS = P*(dP - delta), dQ/dK/dV)
// without its first-key quirk (:217-219).  P is recomputed from the forward's log-sum-exp.
//
// Three kernels, no atomics, bitwise reproducible:
//   1. delta[row,h] = sum_dv dO*O.
//   2. dQ, query-major (one wave per query row, or per 16/h consecutive rows that share their tiles: the forward's mappings): per 32-key tile
//        S^T = K.Q^T, dP^T = V.dO^T, dS^T = exp2(S^T c - lse) * (dP^T - delta) * scale, dQ^T += K^T.dS^T
//      (K is staged once in LDS, as a transposable image: transposing reads give the dQ^T A-operand, row reads the S^T A-operand.)
//   3. dK, dV, KEY-BLOCK-major: one workgroup owns 64 keys of one (b,g) and keeps their dK/dV (64xD fp32 each) in MFMA
//      accumulators while it sweeps every query row that selected the block.  The rows are found by scanning the range
//      lists (lane = row) and compacted in ascending t, so the summation order is fixed.  Rows are processed two at a
//      time in round 1 (2 x 6 heads = 12 of the 16 MFMA rows); round 2 lays the (row, head) slots end to end, every tile full:
//      S = Q.K^T, dP = dO.V^T (16x16x32), then dV += P^T.dO and
//      dK += dS^T.Q as 16x16x16 MFMAs whose A operand is taken straight from the S/dP accumulators (their row index,
//      the (query,head) slot, is the contraction index) and whose B operand is read transposed from LDS.
#include "attn_mfma_tiles.hpp"
#include "attn_rows_schedule.hpp"

namespace nsa {

// Tile geometry: the forward's Geo<D> (attn_mfma_tiles.hpp), a row image and a transposable image.
// Head dimension D = Dk = Dv in {64, 128}: rows of D bf16/f16 elements = D / 8 pieces of 16 B = D / 16 chunks of 32 B.
//   D = 64:  128-B rows, piece XOR r & 7,  chunk XOR (r >> 1) & 3.
//   D = 128: 256-B rows, piece XOR r & 15, chunk XOR r & 7 (the forward's Geo<128> swizzles).
// Bank check (MI355X LDS: 64 banks of 4 B, ds_read_b128 served in the four 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...,
// ds_read_b64_tr_b16 in two 32-lane groups), done exhaustively over every lane group, fragment index and 16-row half, for both D:
// the row reads of the row image (row rho, piece 4s + q), the row reads of the transposable image (same pieces) and the transposing
// reads (row 4q + rho / 4, chunk m, 8 B at 8 (rho & 3)) each touch every bank once per group -- no conflicts.

// ------------------------------------------------------------------------------------------ 1. delta
// Dv / 8 lanes per (row, head), 16 bytes per lane -- a wave reads 512 / Dv whole rows of O and of dO per instruction (one thread
// per row made every lane walk its own 128-byte row: 0.9 TB/s)
template <typename T, int D>
__global__ __launch_bounds__(256) void bwd_delta_kernel(const T *__restrict__ O, const T *__restrict__ dO, float *__restrict__ delta,
                                                         int64_t n_rows, int Dv) {
    constexpr int LPR = D / 8;  // lanes per (row, head)
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPR;  // (row, head)
    const int sub = threadIdx.x % LPR;
    float acc = 0.f;
    if (i < n_rows) {
        const u32x4 a = *(const u32x4 *)(O + i * Dv + 8 * sub), b = *(const u32x4 *)(dO + i * Dv + 8 * sub);
        const T *pa = (const T *)&a, *pb = (const T *)&b;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = fmaf(Elt<T>::to_f(pa[k]), Elt<T>::to_f(pb[k]), acc);
    }
#pragma unroll
    for (int m = 1; m < LPR; m <<= 1) acc += __shfl_xor(acc, m, 64);
    if (i < n_rows && sub == 0) delta[i] = acc;
}

// ------------------------------------------------------------------------------------------ 2. dQ (query-major)
// What a wave of either dQ kernel holds for its 16 MFMA columns (one (query row, head) slot each) and what it does per 32-key tile.
// Wave-private LDS: K in a transposable image, V in a row image.  ONE K image (round 4): the chunk-swizzled image of the transposing reads
// also serves the b128 row-fragment reads without bank conflicts (see bwd_dkdv_kernel), so K is fetched once per tile: 8 LDS-DMA
// instructions per 32 keys at D = 64.
template <typename T, int D>
struct DqWave {
    using M = MfmaT<T>;
    using Gm = Geo<D>;
    using x8 = typename M::x8;
    using x4 = typename M::x4;
    static constexpr int BROWB = Gm::ROWB, KS = Gm::KSTEPS, MT = Gm::MT, NLD = Gm::NLD, RPI = Gm::RPI;
    unsigned char *k_tr, *v_row;        // K, transposable image (row fragments are read from it too); V, row image
    KvSrc<D> kv;
    uint32_t kd_tr[NLD], vd_row[NLD];   // per-lane source offsets of the LDS-DMA loads of a full tile
    uint32_t rd_krow[KS], rd_row[KS], rd_tr[MT];
    x8 qf[KS], dof[KS];                 // B operands held for every tile: Q^T and dO^T fragments (slot = column)
    float lse2 = 0.f, dlt = 0.f;        // the slot's lse (log2 domain) and delta: set by the kernel
    float c2, scale;
    f32x4 dq[MT];
    x8 kfr[2][KS], vfr[2][KS];          // fragments of the current tile
    x4 ktr[2][MT];

    // orow = row * h + head of the lane's slot (used: the slot holds one)
    __device__ __forceinline__ DqWave(const SelAttnBwdParams &P, unsigned char *lds, int b, int g, int lane, int64_t orow, bool used)
        : k_tr(lds), v_row(lds + Gm::TILE_BYTES) {
        const int rho = lane & 15, q = lane >> 4;
        load_col_frags<D>((const T *)P.Q + orow * D, used, q, qf);
        load_col_frags<D>((const T *)P.dO + orow * D, used, q, dof);
        c2 = P.scale * LOG2E;
        scale = P.scale;
        kv = kv_src<T, D>(P, b, g, lane);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int r = RPI * i + kv.ld_row;
            kd_tr[i] = kv.ld_row * kv.krowb + Gm::tr_piece(r, kv.ld_piece);
            vd_row[i] = kv.ld_row * kv.vrowb + Gm::row_piece(r, kv.ld_piece);
        }
        frag_read_offsets<D>(rho, q, rd_row, rd_tr);
#pragma unroll
        for (int s = 0; s < KS; ++s) rd_krow[s] = Gm::tr_img(rho, 4 * s + q);
#pragma unroll
        for (int m = 0; m < MT; ++m) dq[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // the 32 keys from tok0 -> LDS by LDS-DMA.  !whole: the rows past `last` re-read row `last` (the caller masks their dS to zero)
    __device__ __forceinline__ void fetch(int tok0, bool whole, int last) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(3))) void lds_void;
        const int ks = uniform(tok0 * kv.krowb), vs = uniform(tok0 * kv.vrowb);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int rowshift = whole ? 0 : (min(RPI * i + kv.ld_row, last) - kv.ld_row);
            const int kso = whole ? ks + i * kv.kstep : ks, vso = whole ? vs + i * kv.vstep : vs;
            const uint32_t kadd = whole ? 0u : (uint32_t)(rowshift * kv.krowb), vadd = whole ? 0u : (uint32_t)(rowshift * kv.vrowb);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(kv.krs, (lds_void *)(k_tr + i * 1024), 16, kd_tr[i] + kadd, kso, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(kv.vrs, (lds_void *)(v_row + i * 1024), 16, vd_row[i] + vadd, vso, 0, 0);
        }
#else
        (void)tok0, (void)whole, (void)last;
#endif
    }
    // A tile step in three parts; the kernel's own LDS reads and tile bookkeeping go between them.  (1) the tile has landed: its fragments
    __device__ __forceinline__ void read_frags() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        read_row_frags<D>(k_tr, rd_krow, kfr);
        read_row_frags<D>(v_row, rd_row, vfr);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int m = 0; m < MT; ++m) ktr[u][m] = M::tr(k_tr + rd_tr[m] + u * 16 * BROWB);
    }
    // (2) the fragments are in registers: the images are refilled with the next tile (more: there is one) under the products of this one
    __device__ __forceinline__ void refill(bool more, int tok0, bool whole, int last) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (more) fetch(tok0, whole, last);
    }
    // (3) the products.  The slot takes key 16u + 4q + j of the tile if bit 16u + j of km is set; !mixed (wave uniform): no slot of the wave
    // is covered in part, every slot is all-on or all-off -- one predicate per lane
    __device__ __forceinline__ void accumulate(bool mixed, bool on, unsigned km) {
        f32x4 sacc[2], pacc[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            sacc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
            pacc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                sacc[u] = M::mma(kfr[u][s], qf[s], sacc[u]);
                pacc[u] = M::mma(vfr[u][s], dof[s], pacc[u]);
            }
        }
        x8 dsf;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float p = __builtin_amdgcn_exp2f(fmaf(sacc[u][j], c2, -lse2));
                if (!mixed) p = on ? p : 0.f;
                else if (!((km >> (16 * u + j)) & 1u)) p = 0.f;
                dsf[4 * u + j] = Elt<T>::from_f(p * (pacc[u][j] - dlt) * scale);
            }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            x8 a;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = ktr[0][m][j];
                a[4 + j] = ktr[1][m][j];
            }
            dq[m] = M::mma(a, dsf, dq[m]);
        }
    }
    __device__ __forceinline__ void store(T *dQr, int q) const {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            x4 ov;
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = Elt<T>::from_f(dq[m][j]);
            *(x4 *)(dQr + 16 * m + 4 * q) = ov;
        }
    }
};

// One query row per wave: the row's ranges as sorted disjoint segments, each walked in 32-key tiles
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void bwd_dq_kernel(SelAttnBwdParams P, const float *__restrict__ delta, int map_mode) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const int wave = uniform((int)(threadIdx.x >> 6));
    int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (map_mode != 0) {  // same (b,g)-major / XCD-aware order as the forward kernel
        const int W = (P.S + 3) >> 2;
        int bg, tc;
        wg_pair(blockIdx.x, map_mode, W, bg, tc);
        const int t = 4 * tc + wave;
        if (t >= P.S) return;
        row = ((int64_t)(bg / P.G) * P.S + t) * P.G + (bg % P.G);
    }
    if (row >= P.R) return;
    unsigned char *lds = smem + (size_t)wave * Geo<D>::WAVE_LDS;
    int *seg = (int *)(lds + 2 * Geo<D>::TILE_BYTES);

    const int h = P.h;
    const int g = (int)(row % P.G);
    const int b = (int)(row / ((int64_t)P.G * P.S));
    int nseg;
    const int L = normalise_ranges(P.ranges + row * (int64_t)P.n * 2, P.n, P.S_kv, seg, &nseg);
    const int rho = lane & 15, q = lane >> 4;  // head = column

    DqWave<T, D> w(P, lds, b, g, lane, row * h + rho, rho < h);
    w.lse2 = (rho < h && L > 0) ? P.lse[row * h + rho] * LOG2E : 0.f;
    w.dlt = (rho < h) ? delta[row * h + rho] : 0.f;

    int it_seg = -1, it_start = 0, it_len = 0, it_pos = 0;
    auto next_tile = [&](int &tok0, int &nvalid) -> bool {
        while (true) {
            if (it_pos < it_len) {
                tok0 = it_start + it_pos;
                nvalid = min(32, it_len - it_pos);
                it_pos += 32;
                return true;
            }
            if (++it_seg >= nseg) return false;
            it_start = uniform(seg[2 * it_seg]);
            it_len = uniform(seg[2 * it_seg + 3]) - uniform(seg[2 * it_seg + 1]);
            it_pos = 0;
        }
    };
    // tail tiles: rows past the segment re-read its last row, their keys are masked
    int tok0 = 0, nvalid = 0;
    bool have = next_tile(tok0, nvalid);
    if (have) w.fetch(tok0, nvalid == 32, nvalid - 1);
    while (have) {
        const int cur_nvalid = nvalid;
        w.read_frags();
        have = next_tile(tok0, nvalid);
        w.refill(have, tok0, nvalid == 32, nvalid - 1);
        w.accumulate(cur_nvalid != 32, true, bit_span(0, cur_nvalid - 1) >> (4 * q));
    }
    if (rho < h) w.store((T *)P.dQ + (row * (int64_t)h + rho) * D, q);
}

// Several rows per wave, the query-tile form (see sel_attn_rows_mfma.hip): one wave owns TPW = 16/h consecutive rows of one (b,g) (h = 6:
// two rows = 12 of the 16 MFMA columns) and walks the UNION of their selected 32-key tiles, so the two LDS images of a tile are built once
// for the rows that share it.  Tile schedule and ownership are those of attn_rows_schedule.hpp; a slot whose row did not select a key
// gets p = 0.
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void bwd_dq_rows_kernel(SelAttnBwdParams P, const float *__restrict__ delta, int map_mode, int tpw, int NW,
                                                          int wave_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = lane_id();
    const int wave = uniform((int)(threadIdx.x >> 6));
    const int h = P.h, n = P.n;
    const int ngrp = (P.S + tpw - 1) / tpw;
    const int nbg = (int)(P.R / P.S);
    const int W4 = (ngrp + 3) >> 2;
    int bg, tc;
    wg_pair(blockIdx.x, map_mode, W4, bg, tc);
    const int grp = 4 * tc + wave;
    if (grp >= ngrp || bg >= nbg) return;
    const int b = bg / P.G, g = bg - b * P.G;
    const int tw0 = grp * tpw, ntok = min(tpw, P.S - tw0);

    unsigned char *lds = smem + (size_t)wave * wave_lds;
    RowsSched sch(lds + 2 * Geo<D>::TILE_BYTES, tpw, n, NW, ntok);
    for (int i = lane; i < 2 * tpw * NW + 16; i += 64) sch.fullw[i] = 0u;
    for (int r = 0; r < ntok; ++r) {
        const int64_t row = ((int64_t)b * P.S + tw0 + r) * P.G + g;
        if (lane < n) {
            const int32_t *in = P.ranges + (row * n + lane) * 2;
            const int s = min(max(in[0], 0), P.S_kv);
            const int e = min(max(in[1], s), P.S_kv);
            sch.rg[2 * (r * n + lane)] = s;
            sch.rg[2 * (r * n + lane) + 1] = e;
        }
    }
    sch.build(lane);

    const int rho = lane & 15, q = lane >> 4;
    const int tok = rho / h, head = rho - tok * h;
    const bool used = tok < ntok;
    const int64_t orow = used ? ((((int64_t)b * P.S + tw0 + tok) * P.G + g) * h + head) : -1;  // row * h + head

    DqWave<T, D> w(P, lds, b, g, lane, orow, used);
    bool live = false;  // rows without any selected key have lse = -inf: every p is 0
    if (used) {
        const float l = P.lse[orow];
        live = l > -INFINITY;
        w.lse2 = live ? l * LOG2E : 0.f;
        w.dlt = delta[orow];
    }

    // a tile reaching past the end of K/V is never `full`: its clamped rows are masked
    int cur = sch.next_tile();
    if (cur >= 0) w.fetch(32 * cur, 32 * cur + 32 <= P.S_kv, P.S_kv - 1 - 32 * cur);
    const unsigned rowbit = live ? (1u << tok) : 0u;
    while (cur >= 0) {
        const int nxt = sch.next_tile();
        const int tok0 = 32 * cur;
        w.read_frags();
        sch.refresh(cur, lane);
        w.refill(nxt >= 0, 32 * nxt, 32 * nxt + 32 <= P.S_kv, P.S_kv - 1 - 32 * nxt);
        unsigned fullm, touchm;
        sch.owners(cur, fullm, touchm);
        const unsigned partm = touchm & ~fullm;
        if (partm) sch.rebuild_kmask(partm, tok0, lane);  // partially covered by some row: that row's 32-key mask from its ranges
        const bool on = (fullm & rowbit) != 0u;
        unsigned km = on ? 0xffffffffu : 0u;
        if (partm) {
            if (partm & rowbit) km = sch.kmask[tok];
            km >>= 4 * q;  // bit 16u + j = key 16u + 4q + j of the tile
        }
        w.accumulate(partm != 0u, on, km);
        cur = nxt;
    }
    if (used) w.store((T *)P.dQ + orow * D, q);
}

// ------------------------------------------------------------------------------------------ 3. dK / dV (key-block-major)
// column tiles (of 16 (query,head) slots) staged per round.  D = 128 stages 4 (two 16 KiB images, plus 32 KiB of K / V block images:
// 71 KiB per workgroup, two per CU); at 8 the kernel either spills (Q / dO of a round in registers: 2 x 8 x 16 B per thread beside
// 64 dK / dV accumulator registers) or needs 104 KiB of LDS (one workgroup per CU)
template <int D>
constexpr int kb_nct() {
    return D == 64 ? 8 : 4;
}
#ifdef NSA_DBG_WGTIME
__device__ unsigned long long g_dbg[4 * 65536];
#endif

template <typename T, int D>
__global__ __launch_bounds__(256, 2) void bwd_dkdv_kernel(SelAttnBwdParams P, const float *__restrict__ delta, float *__restrict__ part,
                                                        const unsigned long long *__restrict__ hitmap, const unsigned long long *__restrict__ fullmap,
                                                        int *__restrict__ flags, int rows_per_split, int nkb, int nbg, int nsplit) {
    using M = MfmaT<T>;
    using Gm = Geo<D>;
    using x8 = typename M::x8;
    using x4 = typename M::x4;
    constexpr int BROWB = Gm::ROWB, PIECES = Gm::PIECES, KS = Gm::KSTEPS, MT = Gm::MT;
    // Workgroup -> (key block j, bg, row split z).  Workgroups go round-robin over the 8 XCDs by linear id; all key blocks
    // of one (bg, z) pair are put on ONE XCD (its 512 Q/dO rows stay in that L2), and the pairs are dealt evenly over the
    // XCDs (every pair carries about the same number of hits, while key block 0 alone is hit by every row: a j-major
    // order leaves one XCD with several times the work of the others).
    int j, bg, zsp;
    {
        const int w = blockIdx.x, xcd = w & 7, slot = w >> 3;
        const int pair = (slot / nkb) * 8 + xcd;
        j = slot % nkb;
        if (pair >= nbg * nsplit) return;
        zsp = pair / nbg;
        bg = pair - zsp * nbg;
    }
    constexpr int KB_NCT = kb_nct<D>();
    // D = 128 fits 256 registers without scratch only by giving up the register prefetch of the next round's Q / dO rows (they are
    // loaded at the top of their own round) and by reading the K / V fragments from LDS (KV_LDS below)
    constexpr bool PREFETCH = D == 64;
    constexpr int SLOTS = 16 * KB_NCT;        // (query,head) slots per round
    constexpr int IMG = SLOTS * BROWB;        // bytes of one staged image
    constexpr int NLD = SLOTS * PIECES / 256; // 16-byte pieces per thread and image
    // ONE image per staged operand (round 4): the chunk-swizzled image the transposing reads need serves the b128 row-fragment reads too, free
    // of bank conflicts (every 16-lane service group of ds_read_b128 touches 64 distinct banks: checked exhaustively) -- rounds 1-3 staged
    // Q and dO twice (row image + transposable image: 64 KiB of LDS writes per round instead of 32)
    // D = 64: the K/V block images alias the staging images (only read before the loop: their fragments stay in registers).
    // D = 128: the fragments are read from LDS inside the loop (32 registers fewer), the images get LDS of their own
    constexpr bool KV_LDS = D == 128;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * IMG + (KV_LDS ? 2 * 64 * BROWB : 0)];
    __shared__ __attribute__((aligned(16))) float s_lse2[SLOTS], s_delta[SLOTS];
    __shared__ __attribute__((aligned(16))) unsigned long long s_mask[SLOTS];
    __shared__ int s_tilefull[KB_NCT];  // every used slot of the tile covers all 64 keys of the block: the mask test is skipped
    __shared__ int s_t[512];
    __shared__ unsigned long long s_m[512];
    unsigned char *k_img = KV_LDS ? lds + 2 * IMG : lds, *v_img = k_img + 64 * BROWB;
    unsigned char *q_img = lds, *do_img = lds + IMG;

#ifdef NSA_DBG_WGTIME
    const unsigned long long dbg_t0 = wall_clock64();
#endif
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int rho = lane & 15, q = lane >> 4;
    const int b = bg / P.G, g = bg % P.G;
    const int h = P.h;
    const int key0 = 64 * j;
    const T *Kb = (const T *)P.K + (int64_t)b * P.ksb + (int64_t)g * P.ksg;
    const T *Vb = (const T *)P.V + (int64_t)b * P.vsb + (int64_t)g * P.vsg;
    const float c2 = P.scale * LOG2E;

    // ---- K_j, V_j -> LDS (row images); rows past S_kv re-read the last row (never covered by a mask)
#pragma unroll
    for (int i = 0; i < 64 * PIECES / 256; ++i) {
        const int p = tid + 256 * i, r = p / PIECES, pc = p % PIECES;
        const int64_t kr = min(key0 + r, P.S_kv - 1);
        *(u32x4 *)(k_img + Gm::row_img(r, pc)) = *(const u32x4 *)(Kb + kr * P.kss + pc * 8);
        *(u32x4 *)(v_img + Gm::row_img(r, pc)) = *(const u32x4 *)(Vb + kr * P.vss + pc * 8);
    }
    __syncthreads();
    // B operands of S = Q.K^T and dP = dO.V^T for this wave's 16 keys: loop invariant
    x8 kB[KV_LDS ? 1 : KS], vB[KV_LDS ? 1 : KS];
    uint32_t kvrd[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        kvrd[s] = Gm::row_img(16 * wave + rho, 4 * s + q);
        if constexpr (!KV_LDS) {
            kB[s] = *(const x8 *)(k_img + kvrd[s]);
            vB[s] = *(const x8 *)(v_img + kvrd[s]);
        }
    }
    __syncthreads();
    f32x4 dK[MT], dV[MT];
#pragma unroll
    for (int n = 0; n < MT; ++n) {
        dK[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        dV[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    uint32_t rd_row[KS], rd_tr[MT];
#pragma unroll
    for (int s = 0; s < KS; ++s) rd_row[s] = Gm::tr_img(rho, 4 * s + q);
    {
        const int qq = rho >> 2, pp = rho & 3, r = 4 * q + qq;
#pragma unroll
        for (int n = 0; n < MT; ++n) rd_tr[n] = r * BROWB + ((n ^ Gm::swz_v(r)) << 5) + 8 * pp;
    }

    // query rows are split over gridDim.z workgroups per key block (block 0 and the local blocks are selected by every
    // row: without the split their workgroups are a long serial tail); the partial sums are added by a second kernel
    // in fixed order, so the result stays bitwise reproducible
    const int row_begin = zsp * rows_per_split, row_end = min(P.S, row_begin + rows_per_split);
    const int wpb = (P.S + 63) >> 6;  // hit-map words per (bg, key block)
    const unsigned long long *hm = hitmap + ((int64_t)bg * nkb + j) * wpb;
    const unsigned long long *hf = fullmap + ((int64_t)bg * nkb + j) * wpb;
    // Hits are collected over 256-row chunks until at least 256 are pending (far-away key blocks see a handful of hits per
    // chunk at long context; staging rounds want to be full)
    int total_hits = 0, pend = 0;
    for (int base = row_begin; base < row_end; base += 256) {
        // ---- which of these 256 query rows selected keys of this block: 4 words of the hit map (lane = row)
        unsigned long long hw[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int wi = (base >> 6) + w;
            hw[w] = wi < wpb ? hm[wi] : 0ull;
        }
        const int nnew = __popcll(hw[0]) + __popcll(hw[1]) + __popcll(hw[2]) + __popcll(hw[3]);  // uniform over the workgroup
        total_hits += nnew;
        int off = pend;
        pend += nnew;
        if (pend == 0 || (pend < 256 && base + 256 < row_end && nnew == 0)) continue;
        unsigned long long hitb = 0ull;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) off += __popcll(hw[w]);
            if (w == wave) hitb = hw[w];
        }
        const int wi_own = (base >> 6) + wave;
        const unsigned long long fullb = wi_own < wpb ? hf[wi_own] : 0ull;  // rows whose hit is one range over the whole block: mask known
        if ((hitb >> lane) & 1ull) {
            const int t = base + tid;
            unsigned long long mask = ~0ull;
            if (!((fullb >> lane) & 1ull)) {  // partial coverage (or several ranges inside the block): the key mask from the row's ranges
                mask = 0ull;
                const int32_t *rg = P.ranges + (((int64_t)b * P.S + t) * P.G + g) * (int64_t)P.n * 2;
                for (int i = 0; i < P.n; ++i) {
                    int s0 = min(max(rg[2 * i], 0), P.S_kv), e0 = min(max(rg[2 * i + 1], 0), P.S_kv);
                    const int lo = max(s0, key0) - key0, hi = min(e0, key0 + 64) - key0;
                    if (hi > lo) mask |= ((hi - lo == 64) ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << lo;
                }
            }
            const int pos = off + __popcll(hitb & ((1ull << lane) - 1ull));
            s_t[pos] = t;
            s_m[pos] = mask;
        }
        if (pend < 256 && base + 256 < row_end) continue;
        const int nhit = pend;
        pend = 0;
        __syncthreads();

        // ---- process the hit rows, KB_NCT tiles of 16 (row, head) slots per staging round.  The global loads of
        // round r+1 (Q, dO rows, lse, delta) are issued into registers before the MFMAs of round r.
        // slots are laid end to end: slot = h * (row of the round) + head, so a round holds SLOTS / h rows and every 16-slot tile is
        // full (two rows x 6 heads per tile left a quarter of the MFMA rows idle; a slot is one independent (row, head) pair, its tile is
        // only the contraction group of the dV / dK products)
        const int rows_per_round = SLOTS / h;
        u32x4 qa[NLD], da[NLD];
        float l2n = 0.f, dln = 0.f;
        unsigned long long mkn = 0ull;
        auto fetch_round = [&](int r0) {
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int p = tid + 256 * i, slot = p / PIECES, pc = p % PIECES;
                const int qi = slot / h, hh = slot - qi * h;
                const int li = r0 + qi;
                qa[i] = (u32x4){0u, 0u, 0u, 0u};
                da[i] = (u32x4){0u, 0u, 0u, 0u};
                if (qi < rows_per_round && li < nhit) {
                    const int64_t rrow = ((int64_t)b * P.S + s_t[li]) * P.G + g;
                    qa[i] = *(const u32x4 *)((const T *)P.Q + (rrow * h + hh) * (int64_t)D + pc * 8);
                    da[i] = *(const u32x4 *)((const T *)P.dO + (rrow * h + hh) * (int64_t)D + pc * 8);
                }
            }
            l2n = 0.f;
            dln = 0.f;
            mkn = 0ull;
            if (tid < SLOTS) {
                const int qi = tid / h, hh = tid - qi * h;
                const int li = r0 + qi;
                if (qi < rows_per_round && li < nhit) {
                    const int64_t rrow = ((int64_t)b * P.S + s_t[li]) * P.G + g;
                    l2n = P.lse[rrow * h + hh] * LOG2E;
                    dln = delta[rrow * h + hh];
                    mkn = s_m[li];
                }
            }
        };
        if (PREFETCH && nhit > 0) fetch_round(0);
        for (int r0 = 0; r0 < nhit; r0 += rows_per_round) {
            if (!PREFETCH) fetch_round(r0);
            // stage Q and dO rows of every slot twice (row image + transposable image), plus lse / delta / mask per slot
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int p = tid + 256 * i, slot = p / PIECES, pc = p % PIECES;
                *(u32x4 *)(q_img + Gm::tr_img(slot, pc)) = qa[i];
                *(u32x4 *)(do_img + Gm::tr_img(slot, pc)) = da[i];
            }
            if (tid < SLOTS) {
                s_lse2[tid] = l2n;
                s_delta[tid] = dln;
                s_mask[tid] = mkn;
                // slots past the last hit row carry zero Q / dO rows, lse2 = delta = 0: p = 1 there multiplies zeros -- they count as full
                const int qi = tid / h;
                const bool fullslot = mkn == ~0ull || !(qi < rows_per_round && r0 + qi < nhit);
                const unsigned long long fb = __ballot(fullslot);  // waves 0 and 1: 64 slots = 4 tiles each
                if (lane < 4) s_tilefull[4 * wave + lane] = ((fb >> (16 * lane)) & 0xffffull) == 0xffffull;
            }
            if (PREFETCH && r0 + rows_per_round < nhit) fetch_round(r0 + rows_per_round);
            __syncthreads();
            // column tiles go in PAIRS: the dV / dK products contract over the 32 (row, head) slots of two tiles with ONE 16x16x32 MFMA per
            // 16 output columns (round 4: the 16x16x16 form they used costs the same issue cycles for half the work --
            // tools/ubench/issue_rates.hip: 19-20 reported cycles either way; the MFMA's k index is only a label, so k = 8q + r is slot
            // 4q + r of the first tile and k = 8q + 4 + r the same slot of the second, on both operands).  A second tile past the last
            // hit row is all zero rows (p = 1 times zero dO, dS = 0): it adds nothing.
            const int ntile = min(KB_NCT, (min(nhit - r0, rows_per_round) * h + 15) >> 4);
            for (int ct = 0; ct < ntile; ct += 2) {
                x8 pa8, dsa8;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int sbase = 16 * (ct + half);
                    f32x4 S = {0.f, 0.f, 0.f, 0.f}, dP = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < KS; ++s) {
                        const x8 kb = KV_LDS ? *(const x8 *)(k_img + kvrd[s]) : kB[KV_LDS ? 0 : s];
                        const x8 vb = KV_LDS ? *(const x8 *)(v_img + kvrd[s]) : vB[KV_LDS ? 0 : s];
                        S = M::mma(*(const x8 *)(q_img + rd_row[s] + sbase * BROWB), kb, S);
                        dP = M::mma(*(const x8 *)(do_img + rd_row[s] + sbase * BROWB), vb, dP);
                    }
                    // accumulator rows = slots sbase + 4q + r, column = key 16 wave + rho
                    const f32x4 l2 = *(const f32x4 *)(s_lse2 + sbase + 4 * q);
                    const f32x4 dl = *(const f32x4 *)(s_delta + sbase + 4 * q);
                    // dS carries no `scale` here: dK is multiplied once when it is written (MFMA and VALU issue add up: every VALU instruction
                    // of this loop is paid in full).  Most tiles are fully covered (whole selection blocks): no per-key mask test for them.
                    if (uniform(s_tilefull[ct + half])) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float p = __builtin_amdgcn_exp2f(fmaf(S[r], c2, -l2[r]));
                            pa8[4 * half + r] = Elt<T>::from_f(p);
                            dsa8[4 * half + r] = Elt<T>::from_f(p * (dP[r] - dl[r]));
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const bool cov = (s_mask[sbase + 4 * q + r] >> (16 * wave + rho)) & 1ull;
                            const float p = cov ? __builtin_amdgcn_exp2f(fmaf(S[r], c2, -l2[r])) : 0.f;
                            pa8[4 * half + r] = Elt<T>::from_f(p);
                            dsa8[4 * half + r] = Elt<T>::from_f(p * (dP[r] - dl[r]));
                        }
                    }
                    // D = 128: the second half's fragment reads are not hoisted above the first half's MFMAs (their registers would not fit)
                    if constexpr (D == 128) __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int n = 0; n < MT; ++n) {
                    const x4 d0 = M::tr(do_img + rd_tr[n] + 16 * ct * BROWB), d1 = M::tr(do_img + rd_tr[n] + 16 * (ct + 1) * BROWB);
                    const x4 q0 = M::tr(q_img + rd_tr[n] + 16 * ct * BROWB), q1 = M::tr(q_img + rd_tr[n] + 16 * (ct + 1) * BROWB);
                    x8 db, qb;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        db[jj] = d0[jj];
                        db[4 + jj] = d1[jj];
                        qb[jj] = q0[jj];
                        qb[4 + jj] = q1[jj];
                    }
                    dV[n] = M::mma(pa8, db, dV[n]);
                    dK[n] = M::mma(dsa8, qb, dK[n]);
                }
            }
            __syncthreads();
        }
    }
    // ---- write this wave's 16 keys: accumulator rows = key 16 wave + 4q + r, column = d 16 n + rho.  A split without
    // hits writes nothing and says so in flags[] (the reduce kernel skips it).
#ifdef NSA_DBG_WGTIME
    if (tid == 0) {
        const int64_t w = ((int64_t)zsp * nbg + bg) * nkb + j;
        if (w < 65536) {
            unsigned hwid;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(hwid));
            g_dbg[4 * w] = dbg_t0;
            g_dbg[4 * w + 1] = wall_clock64();
            g_dbg[4 * w + 2] = total_hits;
            g_dbg[4 * w + 3] = hwid;
        }
    }
#endif
    if (nsplit > 1) {
        if (tid == 0) flags[((int64_t)zsp * nbg + bg) * nkb + j] = total_hits > 0;
        if (total_hits == 0) return;
    }
    const int64_t slab = (int64_t)nbg * P.S_kv * D;  // floats of one [B*G,S_kv,D] tensor
    float *dKb = (nsplit > 1 ? part + (int64_t)zsp * 2 * slab : P.dK) + ((int64_t)bg * P.S_kv) * D;
    float *dVb = (nsplit > 1 ? part + (int64_t)zsp * 2 * slab + slab : P.dV) + ((int64_t)bg * P.S_kv) * D;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int key = key0 + 16 * wave + 4 * q + r;
        if (key < P.S_kv) {
#pragma unroll
            for (int n = 0; n < MT; ++n) {
                dKb[(int64_t)key * D + 16 * n + rho] = dK[n][r] * P.scale;
                dVb[(int64_t)key * D + 16 * n + rho] = dV[n][r];
            }
        }
    }
}

// sum the row-split partials [ns][2][slab] into dK / dV in ascending split order (splits without hits are skipped)
template <int D>
__global__ __launch_bounds__(256) void bwd_reduce_kernel(const float *__restrict__ part, const int *__restrict__ flags,
                                                          float *__restrict__ dK, float *__restrict__ dV, int64_t slab, int ns, int S_kv,
                                                          int nkb) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= 2 * slab) return;
    const int64_t e = i < slab ? i : i - slab;
    const int64_t krow = e / D, bg = krow / S_kv;
    const int jb = (int)(krow - bg * S_kv) >> 6;
    const int64_t nfl = slab / D / S_kv * nkb;  // flags per split
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < ns; ++z)
        if (flags[z * nfl + bg * nkb + jb]) acc += *(const f32x4 *)(part + (int64_t)z * 2 * slab + i);
    float *dst = i < slab ? dK + i : dV + (i - slab);
    *(f32x4 *)dst = acc;
}

// Inverted index of the selection: hitmap[bg][key block j][t / 64] bit (t % 64) = row t of (b,g) has a range reaching into
// keys [64 j, 64 j + 64).  One wave = the 64 rows of one word: lanes that reach the same block are gathered with a ballot, so
// a word gets one OR per (range slot, block) instead of one per row; OR-ing makes the result independent of the order.
// fullmap (same shape, round 4): bit = ONE range of the row covers all 64 keys of the block.  The dK/dV kernel then knows the row's key mask
// of the block (all ones) without reading the row's ranges -- every hit of a batched selection (whole blocks only), all but the clamped last
// block of a sequential one, the inner blocks of a band.
__global__ __launch_bounds__(256) void bwd_hitmap_kernel(const int32_t *__restrict__ ranges, unsigned long long *__restrict__ hitmap,
                                                          unsigned long long *__restrict__ fullmap, int64_t nwords, int S, int G, int n, int S_kv,
                                                          int nkb) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= nwords) return;
    const int wpb = (S + 63) >> 6;
    const int64_t bg = wid / wpb;
    const int tw = (int)(wid - bg * wpb), t = 64 * tw + lane;
    const int64_t b = bg / G, g = bg - b * G;
    const int32_t *rg = ranges + ((b * S + min(t, S - 1)) * G + g) * (int64_t)n * 2;
    unsigned long long *w = hitmap + bg * nkb * wpb + tw;
    unsigned long long *wf = fullmap + bg * nkb * wpb + tw;
    for (int i = 0; i < n; ++i) {
        const int s0 = min(max(rg[2 * i], 0), S_kv), e0 = min(max(rg[2 * i + 1], 0), S_kv);
        int j = s0 >> 6;
        const int jend = (t < S && e0 > s0) ? (e0 - 1) >> 6 : -1;
        for (;;) {
            const unsigned long long todo = __ballot(j <= jend);
            if (todo == 0ull) break;
            const int src = __ffsll((long long)todo) - 1;
            const int j0 = __shfl(j, src);
            const bool mine = j <= jend && j == j0;
            const unsigned long long m = __ballot(mine);
            const unsigned long long mf = __ballot(mine && s0 <= 64 * j0 && e0 >= 64 * j0 + 64);
            if (lane == src) {
                atomicOr(w + (int64_t)j0 * wpb, m);
                if (mf) atomicOr(wf + (int64_t)j0 * wpb, mf);
            }
            if (mine) ++j;
        }
    }
}

// ------------------------------------------------------------------------------------------ host
static int dkdv_splits(int S) {
    int ns = (S + 511) / 512;
    return ns < 1 ? 1 : (ns > 16 ? 16 : ns);
}

// workspace layout: delta [R*h] f32 | hit map [nbg][nkb][ceil(S/64)] u64 | full map (same shape) | flags [ns][nbg][nkb] i32 | ns partial [dK|dV] slabs
struct BwdWs {
    size_t hitmap, fullmap, flags, part, total, hitmap_bytes;
    int ns, nkb;
};
static BwdWs bwd_ws_layout(int64_t R, int h, int S, int64_t nbg, int S_kv, int D) {
    BwdWs w;
    w.ns = dkdv_splits(S);
    w.nkb = (S_kv + 63) / 64;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    w.hitmap = up(sizeof(float) * (size_t)R * h);
    w.hitmap_bytes = sizeof(unsigned long long) * (size_t)nbg * w.nkb * ((S + 63) / 64);
    w.fullmap = w.hitmap + up(w.hitmap_bytes);
    w.flags = w.fullmap + up(w.hitmap_bytes);
    w.part = w.flags + up(sizeof(int) * (size_t)w.ns * nbg * w.nkb);
    w.total = w.part + (w.ns > 1 ? sizeof(float) * (size_t)w.ns * 2 * (size_t)nbg * S_kv * D : 0);
    return w;
}
size_t sel_attn_bwd_mfma_workspace(int64_t R, int h, int S, int64_t nbg, int S_kv, int D) {
    return bwd_ws_layout(R, h, S, nbg, S_kv, D).total;
}

// The dQ launch.  The rows of one wave share the K/V tile images when 16/h >= 2 rows fit the MFMA columns (NSA_HIP_SEL_ROWS=0: one row
// per wave).  Workgroups of 4 waves go (b,g)-major (map_mode 1; 2 = whole pairs per XCD, see wg_pair); short sequences (S < 16) would leave
// most waves of such a workgroup idle, so the one-row kernel then takes the rows as they come (map_mode 0).
template <typename T, int D>
static int launch_bwd_dq(const SelAttnBwdParams &P, const float *delta, hipStream_t st) {
    const int tpw = tuning(TUNE_SEL_ROWS) == 0 ? 1 : 16 / P.h;
    const int nw = rows_sched_words(P.S_kv);
    const bool rows = tpw >= 2 && P.S >= 2 * tpw && P.n >= 1 && P.n <= 64 && nw <= 128;
    const int rpw = rows ? tpw : 1;                                         // rows per wave
    const int64_t nbg = P.R / P.S, W = ((P.S + rpw - 1) / rpw + 3) / 4;     // workgroups per (b,g)
    const bool fits = nbg * W < ((int64_t)1 << 31);
    // 34 KiB (D = 64), 66 KiB (D = 128) of tiles and segment list per workgroup of the one-row kernel
    const int wave_lds = rows ? 2 * Geo<D>::TILE_BYTES + rows_sched_bytes(tpw, P.n, nw) : Geo<D>::WAVE_LDS;
    const size_t lds = 4 * (size_t)wave_lds;
    NSA_CHECK_ARG(!rows || (fits && lds <= 160 * 1024), "bwd_dq_rows: launch too large");
    const bool pairs = rows || (P.S >= 16 && fits);
    const int map_mode = !pairs ? 0 : (nbg % 8 == 0) ? 2 : 1;
    const dim3 grid((unsigned)(pairs ? nbg * W : (P.R + 3) / 4));
    const void *k = rows ? (const void *)bwd_dq_rows_kernel<T, D> : (const void *)bwd_dq_kernel<T, D>;
    if (lds > 64 * 1024) NSA_HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (rows) {
        hipLaunchKernelGGL((bwd_dq_rows_kernel<T, D>), grid, dim3(256), lds, st, P, delta, map_mode, tpw, nw, wave_lds);
        NSA_LAUNCH_CHECK("bwd_dq_rows");
    } else {
        hipLaunchKernelGGL((bwd_dq_kernel<T, D>), grid, dim3(256), lds, st, P, delta, map_mode);
        NSA_LAUNCH_CHECK("bwd_dq");
    }
    return NSA_OK;
}

template <typename T, int D>
static int launch_bwd_t(const SelAttnBwdParams &P, int dtype, float *delta, hipStream_t st) {
    if (!P.skip_delta_dq) {
        if (const int rc = launch_bwd_delta(P.O, P.dO, delta, P.R * P.h, P.Dv, dtype, st)) return rc;
        if (const int rc = launch_bwd_dq<T, D>(P, delta, st)) return rc;
    }
    const int64_t nbg = (int64_t)(P.R / P.S);  // (at most 65535: both entry points test it)
    const BwdWs W = bwd_ws_layout(P.R, P.h, P.S, nbg, P.S_kv, D);
    const int ns = W.ns;
    const int rows_per_split = ((P.S + ns - 1) / ns + 255) / 256 * 256;
    unsigned char *ws = (unsigned char *)delta;
    unsigned long long *hitmap = (unsigned long long *)(ws + W.hitmap);
    unsigned long long *fullmap = (unsigned long long *)(ws + W.fullmap);
    int *flags = (int *)(ws + W.flags);
    float *part = (float *)(ws + W.part);
    NSA_HIP_TRY(hipMemsetAsync(hitmap, 0, W.fullmap - W.hitmap + W.hitmap_bytes, st));  // both maps (adjacent)
    const int64_t nwords = nbg * ((P.S + 63) / 64);
    hipLaunchKernelGGL(bwd_hitmap_kernel, dim3((unsigned)((nwords + 3) / 4)), dim3(256), 0, st, P.ranges, hitmap, fullmap, nwords, P.S, P.G,
                       P.n, P.S_kv, W.nkb);
    NSA_LAUNCH_CHECK("bwd_hitmap");
    const int64_t ngrid = ((nbg * ns + 7) / 8) * 8 * W.nkb;
    NSA_CHECK_ARG(ngrid < ((int64_t)1 << 31), "bwd: too many key-block workgroups for one launch");
    hipLaunchKernelGGL((bwd_dkdv_kernel<T, D>), dim3((unsigned)ngrid), dim3(256), 0, st, P, (const float *)delta, part,
                       (const unsigned long long *)hitmap, (const unsigned long long *)fullmap, flags, rows_per_split, W.nkb, (int)nbg, ns);
    NSA_LAUNCH_CHECK("bwd_dkdv");
    if (ns > 1) {
        const int64_t slab = nbg * P.S_kv * D;
        hipLaunchKernelGGL(bwd_reduce_kernel<D>, dim3((unsigned)((2 * slab / 4 + 255) / 256)), dim3(256), 0, st, (const float *)part,
                           (const int *)flags, P.dK, P.dV, slab, ns, P.S_kv, W.nkb);
        NSA_LAUNCH_CHECK("bwd_reduce");
    }
    return NSA_OK;
}

#ifdef NSA_DBG_WGTIME
extern "C" __attribute__((visibility("default"))) int nsa_dbg_read(void *host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_dbg), sizeof(unsigned long long) * 4 * 65536);
}
#endif
int launch_sel_attn_bwd_mfma(const SelAttnBwdParams &P, int dtype, float *delta_ws, hipStream_t st) {
    NSA_CHECK_ARG(slabs_under_2gib(P), "bwd MFMA: one (b,g) K/V slab must be smaller than 2 GiB");
    return with_elt<false>(dtype, [&](auto t) { return P.Dk == 64 ? launch_bwd_t<decltype(t), 64>(P, dtype, delta_ws, st) : launch_bwd_t<decltype(t), 128>(P, dtype, delta_ws, st); });
}

int launch_bwd_delta(const void *O, const void *dO, float *delta, int64_t n_rows, int Dv, int dtype, hipStream_t st) {
    const dim3 grid((unsigned)((n_rows * (Dv / 8) + 255) / 256));
    with_elt<false>(dtype, [&](auto t) {
        using T = decltype(t);
        if (Dv == 64) hipLaunchKernelGGL((bwd_delta_kernel<T, 64>), grid, dim3(256), 0, st, (const T *)O, (const T *)dO, delta, n_rows, Dv);
        else hipLaunchKernelGGL((bwd_delta_kernel<T, 128>), grid, dim3(256), 0, st, (const T *)O, (const T *)dO, delta, n_rows, Dv);
    });
    NSA_LAUNCH_CHECK("bwd_delta");
    return NSA_OK;
}

// the band as one [lo, hi) range per (b,t,g) row: input of the selection backward kernels
__global__ __launch_bounds__(256) void band_ranges_kernel(int32_t *__restrict__ ranges, int64_t R, int S, int G, int S_kv, int t0, int a, int dd,
                                                          int c, int w) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= R) return;
    const int t = (int)((row / G) % S);
    const int hi = band_hi(t0, a, dd, c, S_kv, t);
    ranges[2 * row] = max(0, hi - w);
    ranges[2 * row + 1] = hi;
}

int launch_band_ranges(int32_t *ranges, const BandAttnParams &P, hipStream_t st) {
    const int64_t R = (int64_t)P.B * P.S * P.G;
    if (R == 0) return NSA_OK;
    hipLaunchKernelGGL(band_ranges_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, ranges, R, P.S, P.G, P.S_kv, P.t0, P.a, P.dd, P.c, P.w);
    NSA_LAUNCH_CHECK("band_ranges");
    return NSA_OK;
}

}  // namespace nsa
