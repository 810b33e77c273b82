// One decode step of the selected branch in ONE launch (round 3): logits -> softmax statistics -> Eq.9 / Eq.10 -> sequential top-n ->
// selection attention, for the default block geometry (l = 2d, l' = 4d = 64: Eq.9 is the 5-tap stencil of SURVEY.md 8(a) A3).
// Replaces, per step: compute_pcmp_all -> map_pcmp_to_pslc_batched -> sum(dim=3) -> select_topn_ranges -> the selection executor
// (nsa/core/nsa_attention.py:651-672, 704-830; nsa/core/selection_scorer.py:42-61, 89-116, 124-249).
//
// Why a new kernel (profiles/r02/m_decode_timeline.txt): the round-2 kernel spent 6.5 of its 20 us (B = 64, 16k context) in a chain of
// on-chip phases between its two memory phases -- logits -> LDS -> barrier -> statistics -> barrier -> taps -> barrier -> head sums ->
// barrier -> top-n -> ranges -> barrier -> segment table / scan -> gather -- with HBM idle all the while, at one workgroup per CU.  Here:
//   * the logits never leave the registers: the MFMA accumulators of a wave hold 4 consecutive compressed rows = ONE selection block
//     per lane group, so Eq.9 is in-lane except one lane rotation and Eq.10 is a DPP row-shift add (the prefill scorer's trick,
//     sel_scores_mfma.hip); after ONE barrier (the per-chunk (max, sum) records and the halo logits of the chunk edges through LDS)
//     every wave forms the per-head log-sum-exp for itself -- in the butterfly order of wave_max / wave_sum, so p_grp has the bits of the
//     three-kernel route (decode_logits_mfma_kernel -> decode_pgrp_kernel) -- and writes its blocks' group scores;
//   * the selector leaves the picked BLOCKS in LDS (sel_select_row.hpp), wave e mod NW gathers block e: no range -> segment -> chunk
//     translation on the critical path; the merged ranges (the path's second result) are stored while the gather is in flight;
//   * NW = 8 (two workgroups per CU) from 257 rows on: one row's chain overlaps another row's memory phases (sel_attn_decode.hpp);
//   * long contexts / few rows: the K_cmp sweep of a row is SPLIT over NS workgroups (all on one XCD: they meet in its L2); each leaves
//     its scaled logits and chunk records in the workspace and takes a ticket, the LAST one to arrive carries on with the row (no
//     workgroup ever waits for another: no co-residency assumption, nothing to dead-lock) -- early rows reach their chain and gather
//     while later rows still sweep, which is the overlap the single-workgroup form cannot have at 64k.
// Results: ranges identical, O bit-identical to the three separate launches (tests: test_fused_decode_step,
// test_fused_decode_scorer_equals_three_kernel_route).
// Rows form (template flag ROWS; nsa_sel_decode_rows): S consecutive tokens per sequence at t0 .. t0 + S - 1 in one launch, on the cache
// that already holds them ("k draft tokens to verify", speculative-verify rows, the tail of a chunked prefill -- cases that otherwise take
// the extend route's three or more launches).  One workgroup is one row (b, s, g); only the row's bounds and position were launch-wide
// scalars (S_cmp, nchunk, t_token, and S_kv through t_end), so the workgroup derives its own from the row index, S, G and t0 and uses them
// everywhere.  With a device array of positions (P.t_pos, nsa_sel_decode_ragged) the same form is the ragged-batch step: t0 becomes
// t_pos[b], a slot without a sequence writes zeros, a row without a compressed token skips the score phases.  Unsplit exact forms only (form 0 at D = 64 / 128, form 1 at D = 64
// where the largest row exceeds form 0): no team of workgroups, no tickets, no wait of one workgroup on another, no band workgroups; shapes
// beyond them take the separate launches.  Ranges and O are those of S single steps (tests/test_hip_decode_rows.py).  Measured against S
// single steps and the separate launches: not slower in every cell but S = 1 on rows of >= 32 chunks, which default to the
// separate launches.
// Paged form (template flag PAGED on the ragged rows form; nsa_sel_decode_paged): the caches are pools of pages of 1024 tokens found
// through a device block table -- one scorer chunk and 16 selection blocks per page, so every K_cmp chunk, gathered block and forced block
// lies in ONE page and the table costs one wave-uniform lookup per chunk.  Same form, waves, values and order as the ragged form: ranges
// and O are its bits (tests/test_hip_decode_paged.py).  An instantiation of its own: no other one holds any of its code.
// Long-row form (template flag LONG on the ragged rows form and its paged form; plan form 3, switch DECODE_LONG): a row of up to DSTEP_CH =
// 128 chunks (t <= 131,071) in ONE workgroup, no workspace.  A wave owns chunks wave + NW k; the logits of its first two stay in the
// accumulators as in form 0, every further chunk is swept TWICE: the first sweep leaves only its (max, sum) record and edge logit, the
// second -- once the row's log-sum-exp is known -- loads it again and recomputes the logits with the same MFMAs on the same operands in the
// same order, so the scores, ranges and O are the bits of every other exact form (tests/test_hip_decode_long.py).
#include <algorithm>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <utility>

#define DEC_TS(i)  // (the shared device functions' own stamps belong to the round-2 kernel's timeline: this kernel stamps with DS_TS)
#include "nsa_host.hpp"
#include "nsa_internal.hpp"
#include "sel_attn_decode.hpp"
#include "sel_attn_params.hpp"
#include "sel_select_row.hpp"
#include "band_attn_fwd_body.hpp"

namespace nsa {

#ifdef NSA_DEC_TS  // make TIMELINE=1: s_memrealtime stamps of the workgroup(s) of the middle row, read back by nsa_debug_read_ts2 (tools/decode_timeline.py)
static __device__ long long g_ts2[32];
#define DS_TS(i) do { if (ts_on && threadIdx.x == 0) g_ts2[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define DS_TS(i)
#endif

constexpr int DSTEP_CH = 128;                  // chunks of 64 compressed rows per row of the step: contexts up to 128k tokens (S_cmp <= 8192)
constexpr int DSTEP_PART = 16 * DSTEP_CH * 2;  // floats: [head][chunk][2]
constexpr int DSTEP_HALO = DSTEP_CH * 16;      // floats: [chunk][head] scaled logit of the chunk's last row
constexpr int DSTEP_TAIL = 1024 + 4 * (128 + 68 + 4);  // bytes behind the V tiles: mlw [16][16] f32 | scr | list | misc
constexpr int DSTEP_PAGES = 128;               // paged form: table entries of a sequence kept in LDS behind everything else (the long-row form ends at 128 chunks = 131,072 tokens: pages 0 .. 127)
// The LDS map of a row workgroup, byte offsets for both kernel templates.  The score phases live where the V tiles of the gather will be:
// part | halo | pg.  PREF (16 waves, unsplit): waves 0, 14 and 15 fetch the row's forced blocks (0, t//64 - 1, t//64: known from t alone,
// selection_scorer.py:159-170) at kernel start, V into their own tiles, K into three tiles behind the tail -- so the score data starts at
// tile 1.  (Offsets, not a struct of pointers: with the pointers read back from a struct every kernel of the unit compiled to about 3000
// instructions fewer or more and some to more scratch, profiles/decode_step_fold/isa.txt.)
template <int NW, int D, bool PREF>
struct DecStepLds {
    static constexpr int TILE = dec_att_tile(D);  // V tile of a wave
    static constexpr int PART = PREF ? TILE : 0;  // f32 [head][chunk][2] (max, sum exp2)
    static constexpr int HALO = PART + 4 * DSTEP_PART, PG = HALO + 4 * DSTEP_HALO;  // f32 [chunk][head] edge logits | f32 [S_sel] group scores
    static constexpr int MLW = NW * TILE;  // f32 [NW][16] per-wave copy of the per-head log-sum-exp
    // int [128] run extraction of the selector | int [68] picked blocks, ascending | int [0] number of picked blocks, [1] ticket, [2] team assembled
    static constexpr int SCR = MLW + 4 * NW * 16, LIST = SCR + 4 * 128, MISC = LIST + 4 * 68;
    static constexpr int KTILES = NW * TILE + DSTEP_TAIL;  // PREF: [3] K images of the prefetched blocks
    static constexpr int PAGES = KTILES + (NW == 16 ? 3 * TILE : 0);  // PAGED: int [DSTEP_PAGES] the sequence's table entries
    static_assert(MISC + 4 * 4 <= KTILES, "mlw | scr | list | misc fit the tail behind the V tiles");
};
// The host's view of that map: bytes of a launch, bytes of score data the unsplit kernel keeps in the V-tile area, and what that area holds.
// D = 128 (eight waves): 8 x 16 KiB of V tiles + the tail = 132,896 bytes -- one workgroup per CU; the score phases (part 16 KiB | halo 8 KiB |
// pg <= 8 KiB) fit the 128 KiB of tiles with room to spare
static size_t dstep_lds(int nw, int D = 64) { return (size_t)nw * dec_att_tile(D) + DSTEP_TAIL + (nw == 16 ? 3 * dec_att_tile(D) : 0); }
static size_t dstep_score_bytes(int nw, int h, int S_sel, int cpw) {
    return sizeof(float) * (DSTEP_PART + DSTEP_HALO + (size_t)((S_sel + 3) & ~3)) + (cpw == 4 ? (size_t)3 * nw * 256 * h : 0);
}
static size_t dstep_score_room(int nw, int D = 64) { return (size_t)(nw == 16 ? 13 : nw) * dec_att_tile(D); }

// workgroup barrier for data exchanged through LDS only: waits for this wave's LDS operations, NOT for its vector memory operations
// (__syncthreads() drains vmcnt too, which would stall the three prefetching waves -- and with them the whole workgroup -- until their
// forced blocks have landed, moving that traffic back onto the critical path)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Workgroups behind the step's own (BP.n_sel ...) carry the sliding and the compressed branch of a layer step (nsa_layer_decode_step): the two
// are independent of the selected branch, and as a launch of their own they cost the step ~7 us of kernel plus a launch gap on a chain of
// five dependent launches.  Every wave of such a workgroup is one (row, key split) unit of band_attn_body's split form (wave-private LDS
// in the V tile of the wave, no workgroup barrier); they are dispatched behind the step's own workgroups, so a team of the split form finds
// its members resident as before.
template <typename T, int NW>
__device__ __forceinline__ bool decode_band_workgroup(const DecBandPair &BP) {
    if (blockIdx.x < BP.n_sel) return false;
    const unsigned bb = blockIdx.x - BP.n_sel;
    if (bb < BP.n_w) band_attn_body<T, 64, 1, true, 1>(BP.w, bb, NW, &BP.mg, true);
    else band_attn_body<T, 64, 1, true, 1>(BP.c, bb - BP.n_w, NW, &BP.mg, false);
    return true;
}

// logits of one chunk before scaling (MFMA rows = 64 compressed rows, columns = heads): the MFMAs of decode_logits_mfma_kernel.  Every
// chunk loop of both kernels but the two-chunk arm of phase 1, which keeps its written-out copy: called from there, the D = 64 and D = 128
// forms 0 compile to other code (profiles/decode_step_fold/isa.txt)
template <class M, int KS>
__device__ __forceinline__ void chunk_logits(const typename M::x8 (&src)[4][KS], const typename M::x8 (&qf)[KS], f32x4 (&z)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        f32x4 zz = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) zz = M::mma(src[u][s], qf[s], zz);
        z[u] = zz;
    }
}

// Eq.10 head sum: heads of the group = columns 0 .. h-1 of this 16-lane row, lane 0 collects them in ascending order by DPP row shifts.  HC =
// the group size at compile time (straight-line code); HC = 0: any h <= 16 -- columns >= h enter as zeros (p >= 0: adding +0 is exact), so
// the 15 shifted adds run unconditionally (a scalar branch per possible head cost 2 us per step at 64k)
template <int K>
__device__ __forceinline__ float dstep_shift_add(float grp, float src) {
    return grp + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, src), 0x100 | K, 0xf, 0xf, true));
}
template <int HC, int... K>
__device__ __forceinline__ float dstep_head_sum(float slc, int rho, int h, std::integer_sequence<int, K...>) {
    const float src = HC == 6 ? slc : rho < h ? slc : 0.f;
    float grp = src;
    ((grp = dstep_shift_add<K + 1>(grp, src)), ...);
    return grp;
}
template <int HC>
__device__ __forceinline__ float dstep_head_sum(float slc, int rho, int h) {
    return dstep_head_sum<HC>(slc, rho, h, std::make_integer_sequence<int, HC == 6 ? 5 : 15>{});
}

// CPW = chunks of 64 compressed rows per wave.  2: the logits of both stay in the MFMA accumulators (contexts to 32 NW chunks).  4 (round 4,
// unsplit only): a row of up to 4 NW chunks in ONE workgroup -- 64k contexts on 16 waves, 32k on 8 -- for batches whose rows times a team's
// workgroups do not fit the chip together (B >= 128 at 64k: a team must be co-resident, R NS <= slots): the first chunk's logits stay in
// registers, those of the later three wait in LDS ([slot][u][head][q] f32x4, 256 h bytes per chunk: each lane reads back exactly what it
// wrote, so no barrier guards them) until the row's log-sum-exp is known.  Two chunks (16 KiB per wave) are in flight throughout.  Same
// arithmetic on the same values: p_grp, ranges and O have the bits of every other form.
template <typename T, int NW, bool SPLIT, int HC, int CPW = 2, int D = 64, bool ROWS = false, bool PAGED = false, bool LONG = false>
__global__ __launch_bounds__(NW * 64, D == 64 ? 4 : 2) void decode_step_kernel(DecStepParams P, SelectParams SP, int cand, DecAttnArgs AT, DecBandPair BP) {
    static_assert(CPW == 2 || (CPW == 4 && !SPLIT), "four chunks per wave: unsplit form only");
    static_assert(!PAGED || ROWS, "paged caches: the ragged rows form only");
    static_assert(D == 64 || (D == 128 && NW == 8 && CPW == 2), "D = 128: eight waves per row, logits in the accumulators");
    constexpr int KS = D / 32;              // MFMA k-steps of a logit
    constexpr int TILE = dec_att_tile(D);   // V tile of a wave (the score phases live in the same LDS)
    static_assert(!ROWS || !SPLIT, "rows form: one workgroup per row, no meeting of workgroups");
    static_assert(!LONG || (ROWS && CPW == 2), "long-row form: the rows form, the first two chunks of a wave in the accumulators");
    if constexpr (!ROWS) {
        if (decode_band_workgroup<T, NW>(BP)) return;
    }
    using M = MfmaT<T>;
    using x8 = typename M::x8;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr bool PREF = NW == 16 && !SPLIT;
    using L = DecStepLds<NW, D, PREF>;
    float *part = (float *)(lds + L::PART), *halo = (float *)(lds + L::HALO), *pg = (float *)(lds + L::PG), *mlw = (float *)(lds + L::MLW);
    int *scr = (int *)(lds + L::SCR), *list = (int *)(lds + L::LIST), *misc = (int *)(lds + L::MISC);
    [[maybe_unused]] unsigned char *ktiles = lds + L::KTILES;
    [[maybe_unused]] int *pages = (int *)(lds + L::PAGES);

    const int lane = lane_id(), wave = uniform((int)(threadIdx.x >> 6)), rho = lane & 15, q = lane >> 4;
    const int h = P.h;
    auto xl_slot = [&](int k) -> float * {  // CPW = 4: [3 NW slots][4][h][4] f32x4 logits of the chunks beyond a wave's first, behind pg
        return pg + ((P.S_sel + 3) & ~3) + ((size_t)((k - 1) * NW + wave) * 4 * h) * 16;
    };
    int row = blockIdx.x, sp = 0;
    if constexpr (SPLIT) {  // the NS workgroups of a row sit on one XCD (workgroups go round-robin over the 8 XCDs)
        const int per = 8 * P.NS, grp = blockIdx.x / per, rem = blockIdx.x - grp * per;
        row = grp * 8 + (rem & 7);
        sp = rem >> 3;
        if (row >= P.R) return;
    }
    [[maybe_unused]] const bool ts_on = row == P.R / 2;
    DS_TS(0);
    const int g = row % P.G;
    const int64_t b = ROWS ? row / (P.S * P.G) : row / P.G;
    // ROWS: the workgroup's row is (b, s, g) of S consecutive tokens per sequence on ONE cache that already holds them; its token, the
    // compressed rows it sees (n_cmp(t) of the default geometry l = 32, d = 16; the host launches only where n_cmp(t0) >= 1) and its
    // chunks follow from the row index alone.  Otherwise they are the launch's.
    // Ragged form (P.t_pos, nsa_sel_decode_ragged): the sequence's position comes from the device array -- one scalar load, b is uniform --
    // instead of the launch.  A sequence that holds nothing (negative position) or whose rows would pass the caller's bound or the buffers
    // reads nothing and gets zero O and ranges rows: the whole workgroup leaves here, before any barrier.  A row too short to have a
    // compressed token (t < 31) has S_cmp = nchunk = 0: no chunk is loaded (load_chunk would clamp with S_cmp - 1) or scored, the group
    // scores keep their zeros, and the selector and the gather run as for any row -- the single step's route for such a token.
    // Paged form (PAGED, nsa_sel_decode_paged): the caches are pools of pages of 1024 tokens -- one scorer chunk of 64 compressed rows, 16
    // selection blocks -- and entry j of row b of P.block_table is the pool page of the sequence's tokens [1024 j, 1024 j + 1024) in all
    // three pools; AT.S_kv is the capacity max_pages * 1024.  A sequence whose position passes the bounds is inactive as above; one that
    // passes them needs the entries j = 0 .. (t_base + S - 1) >> 10 (< max_pages by the capacity bound), and is inactive too if any of
    // them lies outside [0, n_pages).  Every wave checks the needed entries for itself, lane L loading entries L and L + 64 (the long-row
    // form ends at 128 chunks, t <= 131,071: at most DSTEP_PAGES = 128 entries), so the verdict needs no barrier and is the same in every wave; entries behind the
    // needed ones are never read.  The checked entries go to LDS -- every wave stores the same values and reads only behind its own
    // stores -- for the wave-uniform lookups of the sweep, the forced-block prefetch and the gather (kept in the two registers for
    // v_readlane instead, the 16-wave form 1 spilled 17 - 24 VGPRs against 9 this way: DESIGN.md 4.1h).  No table value reaches an
    // address: only entries inside [0, n_pages) do.
    int t_base = P.t_token;
    if constexpr (ROWS) {
        if (P.t_pos) {
            t_base = P.t_pos[b];
            bool live = !(t_base < 0 || t_base + P.S - 1 > min(P.t_max, AT.S_kv - 1));
            if constexpr (PAGED) {
                if (live) {
                    const int need = ((t_base + P.S - 1) >> 10) + 1;
                    const int32_t *te = P.block_table + b * P.bt_stride;
                    const int pe0 = lane < need ? te[lane] : 0, pe1 = lane + 64 < need ? te[lane + 64] : 0;
                    live = __ballot((unsigned)pe0 >= (unsigned)P.n_pages || (unsigned)pe1 >= (unsigned)P.n_pages) == 0;
                    if (live) {
                        pages[lane] = pe0;
                        pages[lane + 64] = pe1;
                        wave_lds_fence();
                    }
                }
            }
            if (!live) {
                T *Or = (T *)AT.O + (int64_t)row * h * D;
                for (int i = threadIdx.x; i < h * D; i += NW * 64) Or[i] = Elt<T>::from_f(0.f);
                int32_t *out = SP.out + (int64_t)row * SP.W * 2;
                for (int i = threadIdx.x; i < 2 * SP.W; i += NW * 64) out[i] = 0;
                return;
            }
        }
    }
    // PAGED: the pool page of the sequence's page j (j wave uniform)
    [[maybe_unused]] auto page_of = [&](int j) -> int { return uniform(pages[j]); };
    const int t_tok = ROWS ? t_base + (row / P.G) % P.S : P.t_token;
    const int S_cmp = ROWS ? (t_tok < 31 ? 0 : min(P.S_cmp, decode_ncmp(t_tok))) : P.S_cmp;  // (t < 31: zero whatever P.S_cmp holds)
    const int nchunk = ROWS ? (S_cmp + 63) >> 6 : P.nchunk;
    [[maybe_unused]] const int64_t kvrow = ROWS ? b * P.G + g : (int64_t)row;  // the row's K/V plane
    const int hc = min(rho, h - 1);  // head of this lane's column (columns >= h repeat the last head: their results are never used)
    // ---- phase 1: logits of this workgroup's chunks (64 compressed rows each = MFMA rows; heads = columns), up to two per wave,
    // all loads out at once
    x8 qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *(const x8 *)((const T *)P.Q + ((int64_t)row * h + hc) * D + 32 * s + 8 * q);
    const T *kb = (const T *)P.Kc + b * P.csb + (int64_t)g * P.csg;
    const int c_lo = SPLIT ? sp * P.cpg : 0, c_hi = SPLIT ? min(nchunk, c_lo + P.cpg) : nchunk;
    constexpr int REGC = CPW == 2 ? 2 : 1;  // chunks of a wave whose logits stay in registers
    x8 a[2][4][KS];
    f32x4 acc[REGC][4];
    auto load_chunk = [&](int c, x8 (&dst)[4][KS]) {
        // PAGED: chunk c = the 64 compressed rows of the sequence's page c (P.csb: the page stride); the clamp stays inside the chunk
        // (c < nchunk), so inside its page
        [[maybe_unused]] const T *kp = nullptr;
        if constexpr (PAGED) kp = (const T *)P.Kc + (int64_t)page_of(c) * P.csb + (int64_t)g * P.csg;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = min(c * 64 + 16 * u + rho, S_cmp - 1);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if constexpr (PAGED) dst[u][s] = *(const x8 *)(kp + (int64_t)(r & 63) * P.css + 32 * s + 8 * q);
                else dst[u][s] = *(const x8 *)(kb + (int64_t)r * P.css + 32 * s + 8 * q);
            }
        }
    };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = c_lo + wave + NW * k;
        if (c < c_hi) load_chunk(c, a[k]);
    }
    // (behind the K_cmp loads in program order: vector memory operations complete in order, the scores must not wait for these)
    DecPrefetch pre{-1, nullptr};
    if constexpr (PREF) {
        const int cb = t_tok >> 6, t_end = min(t_tok + 1, AT.S_kv);
        const int slot = wave == 0 ? 0 : wave - 13;  // waves 14, 15 -> K tiles 1, 2
        if ((wave == 0 || wave >= 14) && cb >= 2 && cb < P.S_sel && AT.kss == 64) {
            const int blk = wave == 0 ? 0 : cb - (15 - wave);
            pre.tok0 = 64 * blk;
            pre.ktile = ktiles + slot * TILE;
            if constexpr (PAGED)  // block blk lies in the sequence's page blk >> 4, from row (blk & 15) * 64 of that page's plane
                decode_prefetch_chunk<T>(AT, (int64_t)page_of(blk >> 4) * P.G + g, (blk & 15) * 64, min(64, t_end - pre.tok0), lds + wave * TILE,
                                         ktiles + slot * TILE, DEC_PAGE_TOKENS);
            else decode_prefetch_chunk<T>(AT, kvrow, pre.tok0, min(64, t_end - pre.tok0), lds + wave * TILE, ktiles + slot * TILE);
        }
    }

    for (int i = threadIdx.x; i < P.S_sel; i += NW * 64) pg[i] = 0.f;  // blocks without a compressed row keep a zero score
    // scaled logits of chunk c (MFMA rows = 64 compressed rows, columns = heads) and the chunk's (max, sum exp2) per head: the arithmetic of
    // decode_logits_mfma_kernel
    // (to_ws: the records go to the team's workspace; otherwise to this workgroup's LDS)
    auto chunk_stats_as = [&](int c, f32x4 (&z)[4], auto to_ws) {
        float m = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = z[u][j] * P.c2;
                z[u][j] = v;
                if (c * 64 + 16 * u + 4 * q + j < S_cmp) m = fmaxf(m, v);
            }
        m = xor32_max(xor16_max(m));  // (= the xor-16, xor-32 shuffle steps of decode_logits_mfma_kernel: same bits)
        float l = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c * 64 + 16 * u + 4 * q + j < S_cmp) l += __builtin_amdgcn_exp2f(z[u][j] - m);
        l = xor32_add(xor16_add(l));
        if constexpr (decltype(to_ws)::value) {
            if (rho < h) {  // write-through (sc1) stores: no release fence needed (cdna guide, Guideline 16 R1)
                if (q == 0)
                    __hip_atomic_store((unsigned long long *)(P.part_g + (((int64_t)row * h + rho) * DSTEP_CH + c) * 2),
                                       ((unsigned long long)__float_as_uint(l) << 32) | __float_as_uint(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (q == 3)
                    __hip_atomic_store((unsigned *)(P.halo_g + ((int64_t)row * DSTEP_CH + c) * 16 + rho), __float_as_uint(z[3][3]), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            if (rho < h) {
                if (q == 0) *(f32x2 *)(part + (rho * DSTEP_CH + c) * 2) = (f32x2){m, l};
                if (q == 3) halo[c * 16 + rho] = z[3][3];  // row 64 c + 63: the half tap of the next chunk's first block
            }
        }
    };
    auto chunk_stats = [&](int c, f32x4 (&z)[4]) { chunk_stats_as(c, z, std::bool_constant<SPLIT>{}); };
    // LONG: the chunk whose loads follow chunk c into the same registers -- the chunk after next of the sweep, and behind the first sweep's
    // last chunks the first ones of the second sweep (wave + 2 NW, wave + 3 NW: same register parity), so two chunks stay in flight across
    // the barrier and the log-sum-exp.  (At D = 64 the 32 accumulator registers of the first two chunks beside two chunks in flight exceed
    // the 128 registers of a lane: 14 - 20 are spilled, with or without these early loads -- profiles/decode_long/resources.txt.)
    [[maybe_unused]] auto long_next = [&](int c, int k) -> int { return c + 2 * NW < c_hi ? c + 2 * NW : wave + NW * (2 + k); };
    if constexpr (LONG) {
        // chunks 0, 1 of the wave -> registers (form 0); every later one leaves its record and edge logit only (first sweep)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = wave + NW * k;
            if (c < c_hi) {
                chunk_logits<M, KS>(a[k], qf, acc[k]);
                if (c + 2 * NW < c_hi) load_chunk(c + 2 * NW, a[k]);
                chunk_stats(c, acc[k]);
            }
        }
        for (int c0 = wave + 2 * NW; c0 < c_hi; c0 += 2 * NW) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int c = c0 + NW * k;
                if (c < c_hi) {
                    f32x4 z[4];
                    chunk_logits<M, KS>(a[k], qf, z);
                    if (long_next(c, k) < c_hi) load_chunk(long_next(c, k), a[k]);
                    chunk_stats(c, z);
                }
            }
        }
    } else if constexpr (CPW == 2) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = c_lo + wave + NW * k;
            if (c < c_hi) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < KS; ++s) z = M::mma(a[k][u][s], qf[s], z);
                    acc[k][u] = z;
                }
                chunk_stats(c, acc[k]);
            }
        }
    } else {
        // chunk 0 -> registers, chunks 1 .. 3 -> LDS; the loads of chunk k + 2 go out as soon as the MFMAs of chunk k have read its fragments
#pragma unroll
        for (int k = 0; k < CPW; ++k) {
            const int c = wave + NW * k;
            if (c < c_hi) {
                f32x4 z[4];
                chunk_logits<M, KS>(a[k & 1], qf, z);
                if (k + 2 < CPW && c + 2 * NW < c_hi) load_chunk(c + 2 * NW, a[k & 1]);
                chunk_stats(c, z);
                if (k == 0) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[0][u] = z[u];
                } else if (rho < h) {
                    float *slot = xl_slot(k);
#pragma unroll
                    for (int u = 0; u < 4; ++u) *(f32x4 *)(slot + ((u * h + rho) * 4 + q) * 4) = z[u];
                }
            }
        }
    }
    DS_TS(1);
    if constexpr (SPLIT) {
        // The NS workgroups of the row meet ONCE: each has published the (max, sum) records and the edge logits of its chunks -- a few
        // hundred bytes, write-through (sc1) stores, every storing wave drained, then ONE lane's agent-scope add behind the workgroup
        // barrier (the hand-off form of the CDNA guide, Guideline 16 R1) -- and waits until all NS have (one lane polls with sc1 loads and
        // s_sleep; the others wait at the barrier it then joins).  The logits themselves never leave the registers: with the row's
        // log-sum-exp every workgroup scores its OWN blocks.  (First form of this kernel: the last arriver re-read all logits from the
        // workspace -- 98 KB per row at 64k, 3.3 us at the ~30 GB/s one CU pulls from memory, and scored all 64 chunks alone.)
        // The wait pays off while the row's workgroups are resident together: the host launches this form only while R NS workgroups fit
        // the chip at once.  It is bounded (P.spin polls), and a workgroup whose team does not assemble in time does the missing work itself
        // (below): no workgroup ever depends on another one being scheduled.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        DS_TS(2);
        __syncthreads();
        if (threadIdx.x == 0) {
            __hip_atomic_fetch_add(P.cnt + row, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int it = 0;
            while (__hip_atomic_load(P.cnt + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < P.NS && it < P.spin) {
                __builtin_amdgcn_s_sleep(2);
                ++it;
            }
            misc[2] = __hip_atomic_load(P.cnt + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= P.NS ? 1 : 0;
        }
        __syncthreads();
        DS_TS(3);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: keeps the compiler from moving the loads below above this point)
        if (misc[2]) {
            // the row's records and edge logits -> LDS, one sc1 load per thread
            for (int i = threadIdx.x; i < h * DSTEP_CH; i += NW * 64) {
                const int hh = i / DSTEP_CH, idx = i % DSTEP_CH;
                if (idx < nchunk) {
                    const unsigned long long r = __hip_atomic_load((const unsigned long long *)(P.part_g + (((int64_t)row * h + hh) * DSTEP_CH + idx) * 2), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_AGENT);
                    *(f32x2 *)(part + (hh * DSTEP_CH + idx) * 2) = (f32x2){__uint_as_float((unsigned)r), __uint_as_float((unsigned)(r >> 32))};
                }
            }
            for (int i = threadIdx.x; i < nchunk * 16; i += NW * 64)
                if ((i & 15) < h) halo[i] = __uint_as_float(__hip_atomic_load((const unsigned *)(P.halo_g + (int64_t)row * DSTEP_CH * 16 + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        } else {
            // The team did not assemble within the poll budget (its other workgroups are not resident yet: a second stream or process holds
            // the CUs).  Nobody waits for anybody here: this workgroup forms the records and edge logits of ALL chunks of the row itself --
            // the same instructions on the same data, so the same bits as its team mates publish -- and carries on.  Slower, never stuck.
            for (int c = wave; c < nchunk; c += NW) {
                x8 b2[4][KS];
                load_chunk(c, b2);
                f32x4 z[4];
                chunk_logits<M, KS>(b2, qf, z);
                chunk_stats_as(c, z, std::false_type{});
            }
        }
        __syncthreads();
        DS_TS(4);
    } else {
        lds_barrier();
        DS_TS(4);
    }

    // ---- phase 2a: per-head log-sum-exp of the row's logits from the chunk records, by every wave for itself.  One 16-lane row of the
    // wave per head, lane i holds records i, i+16, i+32, i+48: ((a_i + a_{i+32}) + (a_{i+16} + a_{i+48})) then xor 8, 4, 2, 1 is the
    // summation tree of wave_sum over 64 lanes (decode_pgrp_kernel / the round-2 fused kernel): same bits.
    const int nr = (nchunk + 15) >> 4;  // records per lane that exist at all (a context of 16k has 16 chunks: one; 128k: eight)
    for (int h0 = 0; h0 < h; h0 += 4) {
        const int hh = h0 + q;
        float mv[8], lv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = rho + 16 * i;
            mv[i] = -INFINITY;
            lv[i] = 0.f;
            if (i < nr && hh < h && idx < nchunk) {
                const f32x2 r = *(const f32x2 *)(part + (hh * DSTEP_CH + idx) * 2);
                mv[i] = r[0];
                lv[i] = r[1];
            }
        }
        float m = fmaxf(fmaxf(fmaxf(mv[0], mv[1]), fmaxf(mv[2], mv[3])), fmaxf(fmaxf(mv[4], mv[5]), fmaxf(mv[6], mv[7])));
        m = fmaxf(m, row_ror<8>(m));  // butterfly over the 16 lanes of the row by DPP rotations (nsa_common.hpp: no LDS crossbar on the chain)
        m = fmaxf(m, row_ror<4>(m));
        m = fmaxf(m, row_ror<2>(m));
        m = fmaxf(m, row_ror<1>(m));
        float av[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // (a record that does not exist adds +0: exact, so skipping its exponential changes nothing)
            av[i] = (i < nr && rho + 16 * i < nchunk) ? lv[i] * __builtin_amdgcn_exp2f(mv[i] - m) : 0.f;
            // beyond 64 chunks the three-kernel route lets lane L add records L and L + 64 before the butterfly: the same sum here
            if (i + 4 < nr && rho + 16 * (i + 4) < nchunk) av[i] += lv[i + 4] * __builtin_amdgcn_exp2f(mv[i + 4] - m);
        }
        float s = (av[0] + av[2]) + (av[1] + av[3]);
        s += row_ror<8>(s);
        s += row_ror<4>(s);
        s += row_ror<2>(s);
        s += row_ror<1>(s);
        if (rho == 0 && hh < h) mlw[wave * 16 + hh] = m + __builtin_amdgcn_logf(s);
    }
    wave_lds_fence();
    const float ml = mlw[wave * 16 + hc];
    DS_TS(5);

    // ---- phase 2b: p = exp2(x - ml), Eq.9 stencil (1/2, 1, 1, 1, 1/2 over rows 4j-1 .. 4j+3, ascending), Eq.10 head sum (ascending h)
    auto blocks_of_chunk = [&](int c, const f32x4 (&v)[4], float hprev) {
        float rot_prev = c > 0 ? __builtin_amdgcn_exp2f(hprev - ml) : 0.f;  // p of row 64 c - 1 (a chunk that exists has its predecessor complete)
        const bool tail = c * 64 + 64 > S_cmp;  // only the row's last chunk can reach past S_cmp (wave uniform): the others need no row masks
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = __builtin_amdgcn_exp2f(v[u][k] - ml);
            if (tail) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c * 64 + 16 * u + 4 * q + k >= S_cmp) p[k] = 0.f;
            }
            const float rot = __shfl(p[3], (lane + 48) & 63, 64);  // row 4j - 1 = last row of the previous lane group (previous sub-tile for q = 0)
            const float tapm1 = (q == 0) ? rot_prev : rot;
            rot_prev = rot;
            float slc = fmaf(0.5f, tapm1, p[0]);  // (0.5 x is exact: the fma rounds once, like the separate product and sum of the reference order)
            slc += p[1];
            slc += p[2];
            slc = fmaf(0.5f, p[3], slc);
            // heads of the group = columns 0 .. h-1 of this 16-lane row: lane 0 collects them in ascending order by DPP row shifts.  HC = the
            // group size at compile time (straight-line code); HC = 0: any h <= 16 -- columns >= h enter as zeros (p >= 0: adding +0 is exact),
            // so the 15 shifted adds run unconditionally (a scalar branch per possible head cost 2 us per step at 64k)
            const float grp = dstep_head_sum<HC>(slc, rho, h);
            const int j = 16 * c + 4 * u + q;
            if (rho == 0 && j < P.S_sel) {
                if constexpr (SPLIT) __hip_atomic_store((unsigned *)(P.pg_g + (int64_t)row * 2048 + j), __float_as_uint(grp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else pg[j] = grp;
            }
        }
    };
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
        const int c = c_lo + wave + NW * k;
        if (c < c_hi) {
            if (k < REGC) {
                blocks_of_chunk(c, acc[k], c > 0 ? halo[(c - 1) * 16 + hc] : 0.f);
            } else {
                f32x4 z[4];  // lanes of columns >= h read the last head's values, as their accumulators would hold them (never used)
                const float *slot = xl_slot(k);
#pragma unroll
                for (int u = 0; u < 4; ++u) z[u] = *(const f32x4 *)(slot + ((u * h + hc) * 4 + q) * 4);
                blocks_of_chunk(c, z, halo[(c - 1) * 16 + hc]);
            }
        }
    }
    if constexpr (LONG) {
        // second sweep: the later chunks again -- the same MFMAs on the same operands in the same order, the same scaling: the bits the
        // first sweep reduced to the chunk's record
        for (int c0 = wave + 2 * NW; c0 < c_hi; c0 += 2 * NW) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int c = c0 + NW * k;
                if (c < c_hi) {
                    f32x4 z[4];
                    chunk_logits<M, KS>(a[k], qf, z);
                    if (c + 2 * NW < c_hi) load_chunk(c + 2 * NW, a[k]);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int j = 0; j < 4; ++j) z[u][j] = z[u][j] * P.c2;
                    blocks_of_chunk(c, z, halo[(c - 1) * 16 + hc]);
                }
            }
        }
    }
    if constexpr (SPLIT) {
        // second meeting, nobody waits: the scores of this workgroup's blocks are published (sc1, drained), one lane takes a ticket; the
        // workgroup that draws the last one reads the row's scores (<= 4 KB) and carries on with the row, the others are done
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            const int tk = __hip_atomic_fetch_add(P.cnt + P.R + row, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tk == P.NS - 1) {  // every workgroup of the row is past the first meeting: both words go back to zero for the next launch
                __hip_atomic_store(P.cnt + row, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(P.cnt + P.R + row, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            misc[1] = tk;
        }
        __syncthreads();
        if (misc[1] != P.NS - 1) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int j = threadIdx.x; j < min(P.S_sel, 16 * nchunk); j += NW * 64)
            pg[j] = __uint_as_float(__hip_atomic_load((const unsigned *)(P.pg_g + (int64_t)row * 2048 + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    DS_TS(6);
    lds_barrier();
    DS_TS(7);

    // ---- phase 3: top-n + forced blocks (one wave); the picked blocks go to LDS for the gather, the merged ranges to the caller.
    // (Tried and dropped, profiles/r03/decode_notes.txt: the selection as a rank problem over the whole workgroup -- every block's rank by
    // all-pairs compares of 64-bit (key, ~index) images, three short phases instead of the threshold search's dependent rounds.  All-pairs
    // over 256 slots is 65,536 compares = ~1 us of VALU issue on one CU even at full rate, and v_cmp_gt_u64 is not full rate: 2.1 + 0.7 us
    // at 16k context against 2.8 us for this wave's search, 5.9 against 4.5 us at 64k.)
    int rs = 0, re = 0;
    if (wave == 0) {
        int nb = 0;
        switch (cand) {
            case 1: select_topn_row_regs<1>(SP, pg, t_tok, rs, re, scr, list, &nb); break;
            case 2: select_topn_row_regs<2>(SP, pg, t_tok, rs, re, scr, list, &nb); break;
            case 4: select_topn_row_regs<4>(SP, pg, t_tok, rs, re, scr, list, &nb); break;
            case 8: select_topn_row_regs<8>(SP, pg, t_tok, rs, re, scr, list, &nb); break;
            case 16: select_topn_row_regs<16>(SP, pg, t_tok, rs, re, scr, list, &nb); break;
            default: select_topn_row_regs<32, true>(SP, pg, t_tok, rs, re, scr, list, &nb); break;
        }
        if (lane == 0) misc[0] = nb;
    }
    DS_TS(8);
    lds_barrier();  // the scores are dead from here on: their space holds the V tiles
    if (wave == 0 && lane < SP.W) {
        int32_t *out = SP.out + (int64_t)row * SP.W * 2;
        out[2 * lane] = rs;
        out[2 * lane + 1] = re;
    }
    const int NC = uniform(misc[0]);
    // ---- phase 4: selection attention over the picked blocks (wave e mod NW gathers block e; partials merged through LDS)
    const ListChunks ch{list, min(t_tok + 1, AT.S_kv)};
    DS_TS(9);
    if constexpr (PAGED) {  // the same blocks, each on the plane of its page (kv_row = g: the planes of pool page 0)
        const PagedListChunks pch{list, ch.t_end, pages};
        decode_attend_chunks<T, NW, PagedListChunks, D>(AT, row, pch, NC, lds, qf, pre, g);
    } else if constexpr (ROWS) decode_attend_chunks<T, NW, ListChunks, D>(AT, row, ch, NC, lds, qf, pre, kvrow);
    else decode_attend_chunks<T, NW, ListChunks, D>(AT, row, ch, NC, lds, qf, pre);
    DS_TS(10);
}

// ---- one-pass form (round 4): many rows at a long context ------------------------------------------------------------------------
// B >= 128 sequences at 64k: a row's 64 chunks neither stay in the accumulators of one workgroup (2 per wave) nor can R teams of
// workgroups be resident together, and one 16-wave workgroup per CU with the later logits in LDS (CPW = 4 above) leaves every CU's
// chain -- log-sum-exp, scores, top-n: ~11 us of 50 per row, HBM idle -- exposed, all CUs in step (profiles/r04/decode_cold_notes.txt).
// Here a row is ONE 8-wave workgroup again (two rows per CU: one row's chain under the other's sweep / gather) at up to 8 chunks per wave:
// what a wave keeps of a chunk is not its 16 logits per lane but the Eq.9 sums of their exponentials RELATIVE TO THE CHUNK'S OWN MAXIMUM,
//     E[h, j] = 1/2 e(4j-1) + e(4j) + e(4j+1) + e(4j+2) + 1/2 e(4j+3),   e(i) = exp2(x[h, i] - m_c[h])
// -- 4 registers per chunk, and the exponentials are the ones the chunk's (max, sum) record needs anyway: ONE exponential per logit instead
// of two.  With the row's log-sum-exp ml[h] the score of block j is  sum_h E[h, j] exp2(m_c[h] - ml[h])  (+ the half tap of the previous
// chunk's last row for a chunk's first block, from the edge logits every form publishes).  Same (max, sum) records, same ml, same selector
// and gather as the other forms; the scores carry one more rounding (<= 2 ulp against exp2(x - ml) summed directly), so the RANGES are those
// of the exact forms wherever the 13th / 14th ranking keys are further apart than that -- the contract for scores computed from Q / K
//  -- and exact-tie order is only guaranteed by the exact forms.  The plan picks this form only where they do not apply.
template <typename T, int NW, int HC>
__global__ __launch_bounds__(NW * 64, 4) void decode_step_onepass_kernel(DecStepParams P, SelectParams SP, int cand, DecAttnArgs AT, DecBandPair BP) {
    if (decode_band_workgroup<T, NW>(BP)) return;
    using M = MfmaT<T>;
    using x8 = typename M::x8;
    constexpr int CPW = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr bool PREF = NW == 16;
    using L = DecStepLds<NW, 64, PREF>;
    float *part = (float *)(lds + L::PART), *halo = (float *)(lds + L::HALO), *pg = (float *)(lds + L::PG), *mlw = (float *)(lds + L::MLW);
    int *scr = (int *)(lds + L::SCR), *list = (int *)(lds + L::LIST), *misc = (int *)(lds + L::MISC);
    [[maybe_unused]] unsigned char *ktiles = lds + L::KTILES;
    [[maybe_unused]] int *pages = (int *)(lds + L::PAGES);

    const int lane = lane_id(), wave = uniform((int)(threadIdx.x >> 6)), rho = lane & 15, q = lane >> 4;
    const int h = P.h;
    const int row = blockIdx.x;
    [[maybe_unused]] const bool ts_on = row == P.R / 2;
    DS_TS(0);
    const int g = row % P.G;
    const int64_t b = row / P.G;
    const int hc = min(rho, h - 1);
    x8 qf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) qf[s] = *(const x8 *)((const T *)P.Q + ((int64_t)row * h + hc) * 64 + 32 * s + 8 * q);
    const T *kb = (const T *)P.Kc + b * P.csb + (int64_t)g * P.csg;
    const int nchunk = P.nchunk;
    x8 a[2][4][2];
    auto load_chunk = [&](int c, x8 (&dst)[4][2]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = min(c * 64 + 16 * u + rho, P.S_cmp - 1);
#pragma unroll
            for (int s = 0; s < 2; ++s) dst[u][s] = *(const x8 *)(kb + (int64_t)r * P.css + 32 * s + 8 * q);
        }
    };
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (wave + NW * k < nchunk) load_chunk(wave + NW * k, a[k]);
    DecPrefetch pre{-1, nullptr};
    if constexpr (PREF) {
        const int cb = P.t_token >> 6, t_end = min(P.t_token + 1, AT.S_kv);
        const int slot = wave == 0 ? 0 : wave - 13;
        if ((wave == 0 || wave >= 14) && cb >= 2 && cb < P.S_sel && AT.kss == 64) {
            const int blk = wave == 0 ? 0 : cb - (15 - wave);
            pre.tok0 = 64 * blk;
            pre.ktile = ktiles + slot * DEC_ATT_TILE;
            decode_prefetch_chunk<T>(AT, row, pre.tok0, min(64, t_end - pre.tok0), lds + wave * DEC_ATT_TILE, ktiles + slot * DEC_ATT_TILE);
        }
    }
    for (int i = threadIdx.x; i < P.S_sel; i += NW * 64) pg[i] = 0.f;

    // ---- phase 1: per chunk the (max, sum exp2) record, the edge logit, and the Eq.9 sums of the chunk's blocks relative to its maximum
    float E[CPW][4];
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
        const int c = wave + NW * k;
#pragma unroll
        for (int u = 0; u < 4; ++u) E[k][u] = 0.f;
        if (c < nchunk) {
            f32x4 z[4];
            chunk_logits<M, 2>(a[k & 1], qf, z);
            if (k + 2 < CPW && c + 2 * NW < nchunk) load_chunk(c + 2 * NW, a[k & 1]);  // two chunks (16 KiB per wave) in flight throughout
            float m = -INFINITY;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = z[u][j] * P.c2;
                    z[u][j] = v;
                    if (c * 64 + 16 * u + 4 * q + j < P.S_cmp) m = fmaxf(m, v);
                }
            m = xor32_max(xor16_max(m));
            const float edge = z[3][3];
            float l = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float e = (c * 64 + 16 * u + 4 * q + j < P.S_cmp) ? __builtin_amdgcn_exp2f(z[u][j] - m) : 0.f;
                    z[u][j] = e;
                    l += e;  // (a masked row adds +0: exact -- the sum has the bits of the other forms' record)
                }
            l = xor32_add(xor16_add(l));
            if (rho < h) {
                if (q == 0) *(f32x2 *)(part + (rho * DSTEP_CH + c) * 2) = (f32x2){m, l};
                if (q == 3) halo[c * 16 + rho] = edge;
            }
            float rot_prev = 0.f;  // (the half tap of row 64 c - 1 belongs to another chunk's scale: added in phase 2b)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float rot = __shfl(z[u][3], (lane + 48) & 63, 64);
                const float tapm1 = (q == 0) ? rot_prev : rot;
                rot_prev = rot;
                float slc = fmaf(0.5f, tapm1, z[u][0]);
                slc += z[u][1];
                slc += z[u][2];
                E[k][u] = fmaf(0.5f, z[u][3], slc);
            }
        }
    }
    DS_TS(1);
#ifdef DSTEP_SWEEP_ONLY  // ablation build (timing only, results meaningless): the K_cmp sweep alone -- B = 256 @64k cold: 46.7 of 75.5 us
    if (E[0][0] == 12345.f) pg[0] = E[7][3];
    return;
#endif
    lds_barrier();
    DS_TS(4);
    // ---- phase 2a: per-head log-sum-exp from the chunk records (decode_step_kernel's, statement for statement: same bits)
    const int nr = (nchunk + 15) >> 4;
    for (int h0 = 0; h0 < h; h0 += 4) {
        const int hh = h0 + q;
        float mv[8], lv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = rho + 16 * i;
            mv[i] = -INFINITY;
            lv[i] = 0.f;
            if (i < nr && hh < h && idx < nchunk) {
                const f32x2 r = *(const f32x2 *)(part + (hh * DSTEP_CH + idx) * 2);
                mv[i] = r[0];
                lv[i] = r[1];
            }
        }
        float m = fmaxf(fmaxf(fmaxf(mv[0], mv[1]), fmaxf(mv[2], mv[3])), fmaxf(fmaxf(mv[4], mv[5]), fmaxf(mv[6], mv[7])));
        m = fmaxf(m, row_ror<8>(m));
        m = fmaxf(m, row_ror<4>(m));
        m = fmaxf(m, row_ror<2>(m));
        m = fmaxf(m, row_ror<1>(m));
        float av[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            av[i] = (i < nr && rho + 16 * i < nchunk) ? lv[i] * __builtin_amdgcn_exp2f(mv[i] - m) : 0.f;
            if (i + 4 < nr && rho + 16 * (i + 4) < nchunk) av[i] += lv[i + 4] * __builtin_amdgcn_exp2f(mv[i + 4] - m);
        }
        float s = (av[0] + av[2]) + (av[1] + av[3]);
        s += row_ror<8>(s);
        s += row_ror<4>(s);
        s += row_ror<2>(s);
        s += row_ror<1>(s);
        if (rho == 0 && hh < h) mlw[wave * 16 + hh] = m + __builtin_amdgcn_logf(s);
    }
    wave_lds_fence();
    const float ml = mlw[wave * 16 + hc];
    DS_TS(5);
    // ---- phase 2b: scores of the wave's blocks: E scaled to the row's normaliser, the previous chunk's half tap, Eq.10 head sum (ascending h)
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
        const int c = wave + NW * k;
        if (c < nchunk) {
            const float f = __builtin_amdgcn_exp2f(part[(hc * DSTEP_CH + c) * 2] - ml);
            const float hp = c > 0 ? 0.5f * __builtin_amdgcn_exp2f(halo[(c - 1) * 16 + hc] - ml) : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float slc = E[k][u] * f;
                if (u == 0 && q == 0) slc += hp;
                const float grp = dstep_head_sum<HC>(slc, rho, h);
                const int j = 16 * c + 4 * u + q;
                if (rho == 0 && j < P.S_sel) pg[j] = grp;
            }
        }
    }
    DS_TS(6);
    lds_barrier();
    DS_TS(7);
    // ---- phase 3 / 4: top-n + forced blocks (one wave), then the gather over the picked blocks -- decode_step_kernel's
    int rs = 0, re = 0;
    if (wave == 0) {
        int nb = 0;
        switch (cand) {
            case 1: select_topn_row_regs<1>(SP, pg, P.t_token, rs, re, scr, list, &nb); break;
            case 2: select_topn_row_regs<2>(SP, pg, P.t_token, rs, re, scr, list, &nb); break;
            case 4: select_topn_row_regs<4>(SP, pg, P.t_token, rs, re, scr, list, &nb); break;
            case 8: select_topn_row_regs<8>(SP, pg, P.t_token, rs, re, scr, list, &nb); break;
            case 16: select_topn_row_regs<16>(SP, pg, P.t_token, rs, re, scr, list, &nb); break;
            default: select_topn_row_regs<32, true>(SP, pg, P.t_token, rs, re, scr, list, &nb); break;
        }
        if (lane == 0) misc[0] = nb;
    }
    DS_TS(8);
    lds_barrier();
    if (wave == 0 && lane < SP.W) {
        int32_t *out = SP.out + (int64_t)row * SP.W * 2;
        out[2 * lane] = rs;
        out[2 * lane + 1] = re;
    }
    const int NC = uniform(misc[0]);
    const ListChunks ch{list, min(P.t_token + 1, AT.S_kv)};
    DS_TS(9);
    decode_attend_chunks<T, NW>(AT, row, ch, NC, lds, qf, pre);
    DS_TS(10);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// arrival tickets of the split form: owned by the library, one zeroed array per (device, stream) -- launches of one stream are ordered
// and every launch leaves its tickets at zero, launches of different streams never share an array
static int *decode_tickets(hipStream_t st, int64_t rows) {
    static std::mutex mu;
    static std::unordered_map<uint64_t, std::pair<int *, int64_t>> tab;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const uint64_t key = ((uint64_t)(uintptr_t)st << 8) ^ (uint64_t)dev;
    std::lock_guard<std::mutex> lk(mu);
    auto it = tab.find(key);
    if (it != tab.end() && it->second.second >= rows) return it->second.first;
    const int64_t n = rows < 4096 ? 4096 : rows * 2;
    int *p = nullptr;
    if (hipMalloc(&p, sizeof(int) * n) != hipSuccess) return nullptr;
    // zeroed ON THE LAUNCH STREAM: the fill is ordered before the first kernel that reads the tickets whatever kind of stream `st` is (a plain
    // hipMemset runs on the null stream, which a non-blocking stream does not wait for).  Once per stream; an outgrown array stays
    // allocated -- a launch may still use it
    if (hipMemsetAsync(p, 0, sizeof(int) * n, st) != hipSuccess) {
        (void)hipFree(p);
        return nullptr;
    }
    tab[key] = {p, n};
    return p;
}

size_t decode_step_workspace(int64_t R, int h, int S_cmp) {  // split form: chunk records, edge logits, group scores of every row
    (void)S_cmp;
    return sizeof(float) * (size_t)R * ((size_t)h * DSTEP_CH * 2 + DSTEP_CH * 16 + 2048);
}

static int device_cu_count() {
    static std::mutex mu;
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    std::lock_guard<std::mutex> lk(mu);
    if (cus[dev] == 0) {
        int n = 0;
        cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    return cus[dev];
}

// waves per row workgroup, workgroups per row (1 = an unsplit kernel) and the kernel form; false = this shape is not for the one-launch step.
// form 0: logits in the accumulators (two chunks per wave; a long row as a team of NS workgroups that meet inside the launch: R * NS of them
// must be resident together); 1: one 16- or 8-wave workgroup per row with four chunks per wave, the later chunks' logits in LDS (exact: the
// bits of form 0); 2: the one-pass form, eight chunks per wave (decode_step_onepass_kernel: scores within 2 ulp of the exact forms).
// TUNE_DECODE_WIDE: -1 = form 2 where a team would not fit the chip (measured cold, profiles/r04/decode_cold_forms.txt: B=256@64k 75.5 us
// against 98.4 for form 1 and 98.1 for the round-2 two-launch route; B=128@64k 47.4 / 52.3 / 56.8), 0 = never, 1 / 2 = that form wherever
// the row fits it.
// D = 128: form 0 only, on eight waves with a CU each (132,896 bytes of LDS); a long row whose team does not fit the chip is declined (the
// forms that keep logits or exponential sums of later chunks are not built for it: the caller takes the two-launch route).
static bool decode_step_plan(int64_t R, int nchunk, int h, int S_sel, int D, int *nw_out, int *ns_out, int *form_out) {
    const int nw = dec_att_waves(R, D);
    const int64_t slots = (int64_t)device_cu_count() * (nw == 16 || D == 128 ? 1 : 2);  // 1024-thread workgroups hold a CU each (LDS), 512-thread ones share it
    const int mode = tuning(TUNE_DECODE_SPLIT), wide = tuning(TUNE_DECODE_WIDE);
    int ns = (nchunk + 2 * nw - 1) / (2 * nw);  // at most two chunks per wave (the accumulators of a wave's chunks stay in registers)
    const bool wide_fits = D == 64 && nchunk > 2 * nw && nchunk <= 4 * nw && dstep_score_bytes(nw, h, S_sel, 4) <= dstep_score_room(nw);
    const bool onepass_fits = D == 64 && nchunk <= 8 * nw && dstep_score_bytes(nw, h, S_sel, 2) <= dstep_score_room(nw);
    const bool no_team = ns > 1 && R * ns > slots;
    *nw_out = nw;
    *ns_out = 1;
    if (wide_fits && wide == 1) {
        *form_out = 1;
        return true;
    }
    if (onepass_fits && (wide == 2 || (wide < 0 && no_team))) {
        *form_out = 2;
        return true;
    }
    if (no_team) return false;
    if (mode > 0) {
        int want = mode < ns ? ns : (mode > nchunk ? nchunk : mode);
        while (want > ns && R * want > slots) --want;
        ns = want;
    } else {
        // measured rule (profiles/r03/decode_sweep_split_grid.txt).  A team costs two hand-offs (~2.5 us): a row that fits one workgroup
        // (<= 2 chunks per wave) is only split when every workgroup then gets 8 chunks (64 KiB: contexts from 32k on, few rows) -- at 16k
        // the unsplit form wins at every batch size, at 32k with 128 rows too.  A row that must be split anyway gets one chunk per wave
        // if the chip holds that many workgroups.
        const int ns1 = (nchunk + nw - 1) / nw;  // one chunk per wave
        if (ns >= 2 && ns1 > ns && R * ns1 <= slots) ns = ns1;
        const int t8 = nchunk / 8;  // workgroups of 8 chunks
        if (nchunk >= 32 && t8 > ns && R * t8 <= slots) ns = t8;
    }
    *ns_out = ns;
    *form_out = 0;
    return true;
}

// what both shape plans end with, for a launch of nw waves per workgroup in form fm: the formats and sizes the kernel's phases hold
static bool dstep_shape_ok(const SelDecodeCall &c, int nw, int fm) {
    return (c.dtype == NSA_DT_BF16 || c.dtype == NSA_DT_F16) && c.S_cmp <= 64 * DSTEP_CH && c.S_sel <= 2048 && c.n_top >= 3 && c.n_top <= 64 &&
           (int64_t)c.S_kv * 2 * c.Dv < ((int64_t)1 << 31) && sel_attn_decode_wg_shape_ok(c.dtype, c.h, c.Dk, c.Dv, c.n_top) &&
           dstep_score_bytes(nw, c.h, c.S_sel, fm == 1 ? 4 : 2) <= dstep_score_room(nw, c.Dk);
}
// what both forms ask of the call beyond its shape: the default block geometry (l = 2d, l' = 4d = 64), an aligned K_cmp with strides in
// multiples of 8 elements, and the operands of the row's attention (sel_attn_decode_wg_supported)
bool decode_step_operands_ok(const SelDecodeCall &c) {
    return c.d == 16 && c.l == 32 && c.l_sel == 64 && c.kcs % 8 == 0 && c.kcb % 8 == 0 && c.kcg % 8 == 0 && ((uintptr_t)c.K_cmp % 16 == 0) &&
           sel_attn_decode_wg_supported(attn_call(c, nullptr, 0, nullptr));
}

// the part of decode_step_supported that depends on the shape and the tuning switches alone (default block geometry assumed): the one
// predicate behind both the call and nsa_sel_decode_step_plan.  form / nsplit: the plan (-1 / 0 when declined)
bool decode_step_shape_plan(const SelDecodeCall &c, int *form, int *nsplit) {
    if (form) *form = -1;
    if (nsplit) *nsplit = 0;
    if (tuning(TUNE_DECODE_STEP) == 0 || tuning(TUNE_DECODE_UNFUSED) > 0) return false;
    int nw, ns, fm;
    if (c.rows() < 1 || c.S_cmp < 1 || c.S_sel < 1 || c.h < 1 || c.h > 16 || c.Dk != c.Dv || (c.Dk != 64 && c.Dk != 128) ||
        !decode_step_plan(c.rows(), (c.S_cmp + 63) / 64, c.h, c.S_sel, c.Dk, &nw, &ns, &fm))
        return false;
    if (c.S_kv < 1 || !dstep_shape_ok(c, nw, fm)) return false;
    if (form) *form = fm;
    if (nsplit) *nsplit = ns;
    return true;
}

bool decode_step_supported(const SelDecodeCall &c) {
    return decode_step_shape_plan(c, nullptr, nullptr) && c.t0 >= 0 && c.S_kv >= c.t0 + 1 && decode_step_operands_ok(c);
}

// raise the dynamic-LDS limit once per kernel (the runtime call costs about a millisecond)
static int dstep_raise_lds(void *k) {
    static std::mutex mu;
    static void *raised[112] = {};
    std::lock_guard<std::mutex> lk(mu);
    for (void *r : raised)
        if (r == k) return NSA_OK;
    NSA_HIP_TRY(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    for (void *&r : raised)
        if (!r) {
            r = k;
            break;
        }
    return NSA_OK;
}

// what both launchers hand the kernel besides DecStepParams: the sequential selector, its candidate width, the row attention (c2 = scale log2 e)
struct DecStepBlocks {
    SelectParams SP;
    int cand;
    DecAttnArgs AT;
};
static int dstep_blocks(const SelDecodeCall &c, float c2, DecStepBlocks *b) {
    if (int rc = select_params_fill(&b->SP, nullptr, c.rows(), c.S, c.G, c.S_sel, 64, decode_select_call(c))) return rc;
    const int n = (c.S_sel + 63) / 64;
    b->cand = n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32;
    b->AT = DecAttnArgs{c.Q, c.K, c.V, c.O, c.G, c.h, c.S_kv, c.n_top, c.ksb, c.ksg, c.kss, c.vsb, c.vsg, c.vss, c2};
    return NSA_OK;
}

// ---- the kernel table: one function answers the instantiation of a launch -------------------------------------------------------
using DecStepKernel = void (*)(DecStepParams, SelectParams, int, DecAttnArgs, DecBandPair);
// run-time choices to compile-time constants, one pair of alternatives at a time: dstep_consts(f, Alt<A, B>{first}, ...) = f(A or B, ...)
template <auto A, auto B>
struct Alt {
    bool first;
};
template <class F>
static DecStepKernel dstep_consts(F f) {
    return f();
}
template <class F, auto A, auto B, class... R>
static DecStepKernel dstep_consts(F f, Alt<A, B> x, R... r) {
    return x.first ? dstep_consts([&](auto... c) { return f(std::integral_constant<decltype(A), A>{}, c...); }, r...)
                   : dstep_consts([&](auto... c) { return f(std::integral_constant<decltype(B), B>{}, c...); }, r...);
}
// hc: 6 = the group size at compile time, 0 = any h <= 16; cpw: chunks per wave (4: form 1); lng: the long-row form; onepass: form 2.  Null
// for a combination no route launches: those are not instantiated either (the kernels' static_asserts forbid most of them)
static DecStepKernel dstep_kernel(int dtype, int nw, bool split, int hc, int cpw, int D, bool rows, bool paged, bool lng, bool onepass) {
    return dstep_consts(
        [](auto BF, auto NW, auto SPLIT, auto HC, auto CPW, auto D_, auto ROWS, auto PAGED, auto LONG, auto ONE) -> DecStepKernel {
            using T = std::conditional_t<BF, __bf16, _Float16>;
            [[maybe_unused]] constexpr bool geom = D_ == 64 || (NW == 8 && CPW == 2);  // D = 128: eight waves, two chunks per wave
            if constexpr (ONE) {
                if constexpr (D_ == 64 && CPW == 2 && !SPLIT && !ROWS && !PAGED && !LONG) return decode_step_onepass_kernel<T, NW, HC>;
            } else if constexpr (geom && (CPW == 2 || !(SPLIT || LONG)) && (ROWS ? !SPLIT : !(PAGED || LONG)))  // four chunks: unsplit, not long; rows: no team; paged, long: rows only
                return decode_step_kernel<T, NW, SPLIT, HC, CPW, D_, ROWS, PAGED, LONG>;
            return nullptr;
        },
        Alt<true, false>{dtype == NSA_DT_BF16}, Alt<16, 8>{nw == 16}, Alt<true, false>{split}, Alt<6, 0>{hc == 6}, Alt<2, 4>{cpw == 2}, Alt<64, 128>{D == 64},
        Alt<true, false>{rows}, Alt<true, false>{paged}, Alt<true, false>{lng}, Alt<true, false>{onepass});
}

// What both launchers end with, for nw waves per row workgroup, ns workgroups per row and the plan's form.  own: the caller's fields of the
// argument block (the team's workspace, tickets and poll budget; or S, the positions and the block table), the rest is filled here (c2 =
// scale log2 e).  BP: the band pair of a layer step, its n_sel / n_w set for `grid`; null: the launch carries no band work.  lds_extra:
// bytes behind the map (the paged form's table entries).  what: the launch's name in a HIP error
static int dstep_launch(const SelDecodeCall &c, const DecStepParams &own, int nw, int ns, int form, int nchunk, bool rows, int64_t grid, size_t lds_extra,
                        const DecBandPair *band, hipStream_t st, const char *what) {
    const int D = c.Dk, h = c.h, cpw = form == 1 ? 4 : 2;
    const float c2 = default_scale(c.scale, D) * LOG2E;
    const DecStepParams P{c.Q, c.K_cmp, own.part_g, own.halo_g, own.pg_g, own.cnt, (int)c.rows(), c.G, h, c.S_cmp, c.S_sel, ns, nchunk, (nchunk + ns - 1) / ns, c.t0,
                          own.spin, c.kcb, c.kcg, c.kcs, c2, own.S, own.t_pos, own.t_max, own.n_pages, own.block_table, own.bt_stride};
    DecStepBlocks A{};
    if (int rc = dstep_blocks(c, c2, &A)) return rc;
    const DecStepKernel k = dstep_kernel(c.dtype, nw, ns > 1, h == 6 ? 6 : 0, cpw, D, rows, own.block_table != nullptr, form == 3, form == 2);
    NSA_CHECK_ARG(k != nullptr, "decode step: no kernel for form %d at D = %d on %d waves", form, D, nw);
    // the score data sits in V tiles 1 .. (the prefetching waves of the 16-wave form own tiles 0, 14, 15)
    NSA_CHECK_ARG(dstep_score_bytes(nw, h, c.S_sel, cpw) <= dstep_score_room(nw, D), "decode step: S_sel too large");
    if (int rc = dstep_raise_lds((void *)k)) return rc;
    DecBandPair BP{};
    BP.n_sel = 0xffffffffu;
    if (band) BP = *band;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(nw * 64), dstep_lds(nw, D) + lds_extra, st, P, A.SP, A.cand, A.AT, BP);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_fail(e, what);
    return NSA_OK;
}

int launch_decode_step(const SelDecodeCall &c, void *ws, size_t ws_bytes, hipStream_t st, const DecBandPair *band) {
    const int64_t R = c.rows();
    const int D = c.Dk, h = c.h;
    NSA_CHECK_ARG(D == 64 || D == 128, "decode step: head dimension 64 or 128");
    NSA_CHECK_ARG(R >= 1 && R <= (1 << 24), "decode step: bad row count");
    const int nchunk = ((c.S_cmp + 63) / 64);
    int nw = 16, ns = 1, form = 0;
    NSA_CHECK_ARG(decode_step_plan(R, nchunk, h, c.S_sel, D, &nw, &ns, &form), "decode step: shape not covered (decode_step_supported)");
    DecStepParams own{};
    own.spin = tuning(TUNE_DECODE_TEAM_SPIN) >= 0 ? tuning(TUNE_DECODE_TEAM_SPIN) : 512;  // polls of ~0.5-1 us each before a workgroup goes on alone
    if (ns > 1) {
        NSA_CHECK_ARG(ws && ws_bytes >= decode_step_workspace(R, h, c.S_cmp) && ((uintptr_t)ws % 16 == 0), "decode step: workspace too small");
        own.part_g = (float *)ws;
        own.halo_g = own.part_g + (size_t)R * h * DSTEP_CH * 2;
        own.pg_g = own.halo_g + (size_t)R * DSTEP_CH * 16;
        own.cnt = decode_tickets(st, 2 * R);
        NSA_CHECK_ARG(own.cnt != nullptr, "decode step: could not allocate the arrival tickets");
    }
    NSA_CHECK_ARG(D == 64 || (form == 0 && nw == 8), "decode step: D = 128 runs form 0 on eight waves");
    int64_t grid = ns > 1 ? ((R + 7) / 8) * 8 * ns : R;
    DecBandPair BP{};
    if (band) {  // the layer step's sliding + compressed branches on workgroups behind the step's own (decode_band_workgroup)
        BP = *band;
        int64_t waves[2];
        NSA_CHECK_ARG(D == 64 && BP.w.Dk == 64 && BP.w.Dv == 64 && band_dual_plan(&BP.w, &BP.c, c.dtype, waves), "decode step: band branches not in split form");
        if (BP.mg.on) {  // splits merged by the workgroup that holds them: a unit = nsplit consecutive waves of one workgroup
            NSA_CHECK_ARG(BP.w.S == 1 && BP.c.S == 1 && BP.mg.gates && BP.w.O && BP.c.O && h <= 16, "decode step: band merge needs S = 1, outputs and a gate buffer");
            int nsm = 1;
            while (2 * nsm <= BP.w.nsplit && 2 * nsm <= nw) nsm *= 2;
            BP.w.nsplit = BP.c.nsplit = nsm;
            waves[0] = waves[1] = R * nsm;
        }
        const int64_t gw = (waves[0] + nw - 1) / nw, gc = (waves[1] + nw - 1) / nw;
        NSA_CHECK_ARG(grid + gw + gc < ((int64_t)1 << 31), "decode step: too many workgroups");
        BP.n_sel = (unsigned)grid;
        BP.n_w = (unsigned)gw;
        grid += gw + gc;
    }
    static_assert(2 * Geo<64>::TILE_BYTES <= DEC_ATT_TILE, "a band wave keeps its K and V tile in the wave's V tile of the step");
    return dstep_launch(c, own, nw, ns, form, nchunk, false, grid, 0, band ? &BP : nullptr, st, "decode_step launch");
}

// The measured rule behind DECODE_ROWS = -1 (tools/bench_sel_decode_rows.py, table in DESIGN.md 4.1f; S in {1, 2, 4, 8} x 4k / 16k / 32k x
// B in {1, 16}): one rows launch beat both S single decode steps and the separate launches in every cell except S = 1 at 32k, where the
// single step runs as a team of workgroups (rows of 32 chunks and more, decode_step_plan) and is 3.5 - 4.4 us faster than one workgroup per
// row.  Below 32 chunks the single step IS the unsplit kernel and the two tie.  So: S = 1 with a row of >= 32 chunks is declined.
static bool decode_rows_measured_ok(int S, int nchunk_max) { return !(S == 1 && nchunk_max >= 32); }

// ---- rows form: S consecutive tokens per sequence in one launch (nsa_sel_decode_rows) -----------------------------------------------
// the unsplit exact form that holds a row of nchunk chunks on nw waves: 0 (two chunks per wave), at D = 64 1 (four), -1 = neither
static int dstep_unsplit_form(int nw, int D, int nchunk) { return nchunk <= 2 * nw ? 0 : D == 64 && nchunk <= 4 * nw ? 1 : -1; }

// Shape / tuning part of the rows form's predicate (default block geometry assumed).  One workgroup per row (b, s, g), the form and the
// waves chosen for the launch from its LARGEST row (t0 + S - 1) and its row count B S G: form 0 (two chunks per wave) or, at D = 64, form 1
// (four chunks per wave) where that row exceeds form 0 -- the unsplit exact forms only, whatever DECODE_WIDE says; no team of workgroups,
// no one-pass form.  DECODE_ROWS: 0 = never, 1 = wherever the forms hold the shape, -1 = the measured rule.
bool decode_rows_shape_plan(const SelDecodeCall &c, int *form, int *nw_out) {
    if (form) *form = -1;
    const int sw = tuning(TUNE_DECODE_ROWS), S = c.S, t0 = c.t0;
    if (tuning(TUNE_DECODE_STEP) == 0 || tuning(TUNE_DECODE_UNFUSED) > 0 || sw == 0) return false;
    if (c.B < 1 || S < 1 || S > 16 || c.G < 1 || c.h < 1 || c.h > 16 || c.Dk != c.Dv || (c.Dk != 64 && c.Dk != 128) || c.S_cmp < 1 || c.S_sel < 1) return false;
    if (t0 < 0 || t0 > (1 << 30) || decode_ncmp(t0) < 1 || c.S_kv < t0 + S) return false;  // every row has a compressed row and its own token in the cache
    if (c.rows() > (1 << 24)) return false;
    const int nw = dec_att_waves(c.rows(), c.Dk);
    const int n_max = std::min(c.S_cmp, decode_ncmp(t0 + S - 1)), nchunk = (n_max + 63) / 64;
    const int fm = dstep_unsplit_form(nw, c.Dk, nchunk);
    if (fm < 0 || !dstep_shape_ok(c, nw, fm)) return false;
    if (sw < 0 && !decode_rows_measured_ok(S, nchunk)) return false;
    if (form) *form = fm;
    if (nw_out) *nw_out = nw;
    return true;
}

bool decode_rows_supported(const SelDecodeCall &c) { return decode_rows_shape_plan(c, nullptr, nullptr) && decode_step_operands_ok(c); }

// ---- ragged form (nsa_sel_decode_ragged): the rows form with the position of sequence b read from a device array.  The host never reads
// the array: form and waves are planned from the caller's bound t_max (the largest token any live row can sit at) and the row count exactly
// as decode_rows_shape_plan plans from t0 + S - 1; with DECODE_LONG = 1 a row beyond the unsplit forms gets form 3 (the long-row form, up to
// 128 chunks: t_max <= 131,071) instead of a decline -- a shape inside the unsplit forms keeps form 0 / 1 whatever the switch says.  What the rows form may decline on the host -- a row without a compressed token -- the
// kernel handles, so t_max < 31 is fine here; DECODE_ROWS does not apply (its measured rule weighs alternatives this call does not have: the
// separate launches cannot take per-sequence positions).  *why: the limit a declined call names.
bool decode_ragged_shape_plan(const SelDecodeCall &c, int t_max, int *form, int *nw_out, const char **why) {
    static const char *unused;
    if (!why) why = &unused;
    if (form) *form = -1;
    *why = "the one-launch decode step is switched off (DECODE_STEP = 0 or DECODE_UNFUSED = 1) and there is no other route with per-sequence positions";
    if (tuning(TUNE_DECODE_STEP) == 0 || tuning(TUNE_DECODE_UNFUSED) > 0) return false;
    *why = "needs bf16 / f16, Dk = Dv in {64, 128}, h <= 16, 1 <= S <= 16, 3 <= n_top <= 64 and at most 2048 selection blocks";
    if (c.B < 1 || c.S < 1 || c.S > 16 || c.G < 1 || c.h < 1 || c.h > 16 || c.Dk != c.Dv || (c.Dk != 64 && c.Dk != 128) || c.S_cmp < 0 || c.S_sel < 1 ||
        c.S_kv < 1 || t_max < 0 || t_max > (1 << 30) || c.rows() > (1 << 24))
        return false;
    const int nw = dec_att_waves(c.rows(), c.Dk);
    const int n_max = std::min(c.S_cmp, decode_ncmp(t_max)), nchunk = (n_max + 63) / 64;
    int fm = dstep_unsplit_form(nw, c.Dk, nchunk);
    if (fm < 0 && tuning(TUNE_DECODE_LONG) > 0) {
        // the long-row form (form 3): any row of up to DSTEP_CH chunks, its later chunks swept twice.  t_max itself bounds the selection
        // blocks a live row needs (block t >> 6 must be one of 2048), whatever the buffers hold beyond it
        if (nchunk > DSTEP_CH || t_max >= 64 * 2048) {
            *why = "t_max is beyond the long-row form: at most 131,072 tokens per sequence (t_max <= 131,071), 128 chunks of 64 compressed tokens and 2048 "
                   "selection blocks per row";
            return false;
        }
        fm = 3;
    } else if (fm < 0) {
        *why = c.Dk == 128 ? "t_max is beyond the unsplit form at D = 128: more than 16 chunks of 64 compressed tokens per row"
               : nw == 16  ? "t_max is beyond the unsplit forms at 16 waves per row: more than 64 chunks of 64 compressed tokens per row"
                           : "t_max is beyond the unsplit forms at 8 waves per row (more than 256 rows): more than 32 chunks of 64 compressed tokens per row";
        return false;
    }
    if (!dstep_shape_ok(c, nw, fm)) return false;
    if (form) *form = fm;
    if (nw_out) *nw_out = nw;
    return true;
}

// ---- paged form (nsa_sel_decode_paged): the ragged form over pools of pages.  c.K_cmp / c.K / c.V are the pools, kcb / ksb / vsb their PAGE
// strides and c.S_kv the capacity max_pages * 1024.  Form and waves are the ragged form's, from t_max and the row count alone -- same
// declines, same messages -- except that the byte offsets the kernel forms in 32 bits are those inside one (page, group) plane of 1024 rows
// (the bases are 64-bit: a pool has no size limit), so the plane stands where dstep_shape_ok asks for S_kv 2 Dv < 2^31.
bool decode_paged_shape_plan(const SelDecodeCall &c, int t_max, int *form, int *nw_out, const char **why) {
    SelDecodeCall plane = c;
    plane.S_kv = DEC_PAGE_TOKENS;
    return decode_ragged_shape_plan(plane, t_max, form, nw_out, why);
}

int launch_decode_rows(const SelDecodeCall &c, hipStream_t st, const int32_t *t_pos, int t_max, const DecPageTable *pt) {
    int nw = 16, form = 0;
    if (pt) NSA_CHECK_ARG(t_pos && decode_paged_shape_plan(c, t_max, &form, &nw, nullptr), "decode paged: shape not covered (decode_paged_shape_plan)");
    else if (t_pos) NSA_CHECK_ARG(decode_ragged_shape_plan(c, t_max, &form, &nw, nullptr), "decode ragged: shape not covered (decode_ragged_shape_plan)");
    else NSA_CHECK_ARG(decode_rows_shape_plan(c, &form, &nw), "decode rows: shape not covered (decode_rows_supported)");
    const int nchunk = (std::min(c.S_cmp, decode_ncmp(t_pos ? t_max : c.t0 + c.S - 1)) + 63) / 64;  // of the largest row: every row derives its own
    DecStepParams own{};
    own.S = c.S;
    own.t_pos = t_pos;
    own.t_max = t_max;
    if (pt) {
        // (every table entry the kernel follows is < n_pages, every needed index < max_pages: c.S_kv = max_pages * 1024 bounds the positions)
        NSA_CHECK_ARG(pt->table && pt->n_pages >= 1 && pt->stride >= (int64_t)c.S_kv / DEC_PAGE_TOKENS, "decode paged: bad block table");
        own.n_pages = pt->n_pages;
        own.block_table = pt->table;
        own.bt_stride = pt->stride;
    }
    // (the paged form is an instantiation of its own: the rows / ragged instantiations hold none of its code)
    if (form == 3) NSA_CHECK_ARG(c.Dk == 64 || nw == 8, "decode rows: D = 128 runs on eight waves");  // the long-row form: D = 64 on 16 / 8 waves, D = 128 on 8
    else NSA_CHECK_ARG(c.Dk == 64 || (form == 0 && nw == 8), "decode rows: D = 128 runs form 0 on eight waves");
    return dstep_launch(c, own, nw, 1, form, nchunk, true, c.rows(), pt ? sizeof(int) * DSTEP_PAGES : 0, nullptr, st, pt ? "decode_paged launch" : "decode_rows launch");
}

}  // namespace nsa

#ifdef NSA_DEC_TS
extern "C" __attribute__((visibility("default"))) int nsa_debug_read_ts2(long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(nsa::g_ts2), sizeof(long long) * 32);
}
#endif
