// The kernel of the one-launch decode step of the selected branch (sel_decode_fused.hip has the story, the one-pass kernel, the plans and
// the launch tail): decode_step_kernel with its LDS map and device helpers, in a header so that a family of instantiations can live in a
// translation unit of its own -- the FP8 K/V forms are built in sel_decode_fp8.hip, and the bf16 / f16 instantiations of
// sel_decode_fused.hip keep the module, the inlining order and the code they had without them.
#pragma once
#include <type_traits>
#include <utility>

#define DEC_TS(i)  // (the shared device functions' own stamps belong to the round-2 kernel's timeline: this kernel stamps with DS_TS)
#include "nsa_internal.hpp"
#include "sel_attn_decode.hpp"
#include "sel_attn_decode_fp8.hpp"
#include "sel_attn_params.hpp"
#include "sel_select_row.hpp"
#include "band_attn_fwd_body.hpp"

namespace nsa {

#ifdef NSA_DEC_TS  // make TIMELINE=1: s_memrealtime stamps of the workgroup(s) of the middle row, read back by nsa_debug_read_ts2 (tools/decode_timeline.py)
static __device__ long long g_ts2[32];  // (one copy per translation unit: nsa_debug_read_ts2 reads sel_decode_fused.hip's, the FP8 kernels' stamps are not read back)
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
// FP8 (ragged and paged rows form, bf16 Q / O, forms 0 and 1): K and V of the gather are e4m3 with per-row scales (sel_attn_decode_fp8.hpp).  The
// score phases, the selector and the LDS map are untouched -- the selection does not read K / V -- only the forced-block prefetch is left
// out (its K image is a bf16 one) and phase 4 calls the FP8 form of the row's attention.
template <typename T, int NW, bool SPLIT, int HC, int CPW = 2, int D = 64, bool ROWS = false, bool PAGED = false, bool LONG = false, bool FP8 = false>
__global__ __launch_bounds__(NW * 64, D == 64 ? 4 : 2) void decode_step_kernel(DecStepParams P, SelectParams SP, int cand, DecAttnArgs AT, DecBandPair BP) {
    static_assert(CPW == 2 || (CPW == 4 && !SPLIT), "four chunks per wave: unsplit form only");
    static_assert(!PAGED || ROWS, "paged caches: the ragged rows form only");
    static_assert(D == 64 || (D == 128 && NW == 8 && CPW == 2), "D = 128: eight waves per row, logits in the accumulators");
    constexpr int KS = D / 32;              // MFMA k-steps of a logit
    constexpr int TILE = dec_att_tile(D);   // V tile of a wave (the score phases live in the same LDS)
    static_assert(!ROWS || !SPLIT, "rows form: one workgroup per row, no meeting of workgroups");
    static_assert(!LONG || (ROWS && CPW == 2), "long-row form: the rows form, the first two chunks of a wave in the accumulators");
    static_assert(!FP8 || (ROWS && !LONG && std::is_same_v<T, __bf16>), "FP8 K/V: the ragged and paged rows form, unsplit forms 0 and 1, bf16 queries");
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
    if constexpr (PREF && !FP8) {
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
    if constexpr (FP8) {
        if constexpr (PAGED) decode_attend_chunks_fp8<NW, PagedListChunks, D>(AT, row, PagedListChunks{list, ch.t_end, pages}, NC, lds, qf, g);
        else decode_attend_chunks_fp8<NW, ListChunks, D>(AT, row, ch, NC, lds, qf, kvrow);
    } else if constexpr (PAGED) {  // the same blocks, each on the plane of its page (kv_row = g: the planes of pool page 0)
        const PagedListChunks pch{list, ch.t_end, pages};
        decode_attend_chunks<T, NW, PagedListChunks, D>(AT, row, pch, NC, lds, qf, pre, g);
    } else if constexpr (ROWS) decode_attend_chunks<T, NW, ListChunks, D>(AT, row, ch, NC, lds, qf, pre, kvrow);
    else decode_attend_chunks<T, NW, ListChunks, D>(AT, row, ch, NC, lds, qf, pre);
    DS_TS(10);
}

// one entry of the kernel table (dstep_kernel, sel_decode_fused.hip)
using DecStepKernel = void (*)(DecStepParams, SelectParams, int, DecAttnArgs, DecBandPair);
// the table's FP8 axis (sel_decode_fp8.hip): the FP8 K/V instantiation for nw waves, hc (6 / 0), cpw chunks per wave (2: form 0, 4: form 1), D and
// ragged / paged caches; null where none is built
DecStepKernel dstep_kernel_fp8(int nw, int hc, int cpw, int D, bool paged);

}  // namespace nsa
