// Kernel argument blocks for the selection-attention kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nsa_sel_hip.h"

namespace nsa {

struct SelAttnParams {
    const void *Q;          // [R,h,Dk]   (R = B*S*G rows, row = (b*S+s)*G+g)
    const void *K;          // [B,G,S_kv,Dk] with element strides ksb/ksg/kss
    const void *V;          // [B,G,S_kv,Dv] with element strides vsb/vsg/vss
    const int32_t *ranges;  // [R,n,2]
    void *O;                // [R,h,Dv]
    float *lse;             // [R,h] or null
    int64_t R;
    int S, G, h, Dk, Dv, S_kv, n;
    int64_t ksb, ksg, kss, vsb, vsg, vss;
    float scale;
    // split-KV (few rows): partial results, see sel_attn_mfma.hip
    float *part;  // workspace or null
    int nsplit;
    int map_mode;  // 0 rows linear in blockIdx; 1 workgroup = 4 tokens of one (b,g); 2 = 1 + XCD-aware order
    int defer_combine;  // split-KV: leave the partial records for the caller's own combine pass
    int fuse_select;    // the kernel first selects the row's ranges from its group scores (select = const SelectParams *, host)
    const void *select;
    int tpw, nw, wave_lds;  // query-tile form (sel_attn_rows_mfma.hip): rows per wave, 32-tile bitmap words per row, LDS bytes per wave
    void *ks_ws;            // key-split form of the block kernel (sel_attn_blocks_mfma.hip): caller's workspace (16-byte aligned) or null
    size_t ks_bytes;
    // key-split form, filled by its launcher: rows [0, ks_r1) of a (b,g) are walked unsplit, [ks_r1, ks_r2) in two key classes, [ks_r2, S) in
    // four (multiples of the 32 rows of a workgroup); workgroups per XCD of one class of each zone
    int ks_r1, ks_r2, ks_w1, ks_w2, ks_wa, ks_wb, ks_wc;  // (ks_w1 / ks_w2: first workgroup of zones 1 / 2; ks_r = min(ks_w * rows per workgroup, S))
};

struct SelAttnBwdParams {
    const void *Q, *K, *V;
    const int32_t *ranges;
    const void *O;
    const float *lse;
    const void *dO;
    void *dQ;
    float *dK, *dV;
    int64_t R;
    int S, G, h, Dk, Dv, S_kv, n;
    int64_t ksb, ksg, kss, vsb, vsg, vss;
    float scale;
    int skip_delta_dq;  // MFMA route: delta is already in the workspace and dQ is produced elsewhere (band backward)
};

// Band attention (sliding-window and compressed branches): query row t (position t0 + t) attends keys [max(0, hi - w), hi),
//   hi(t) = (t0 + t + 1 >= a) ? min(S_kv, (t0 + t + 1 - a) / dd + c) : 0.
// sliding window: a = 0, dd = 1, c = 0 (hi = t + 1), w = window; compressed: a = l, dd = d, c = 1, w = "infinite".
struct BandAttnParams {
    const void *Q;  // [B,S,G,h,D]
    const void *K;  // [B,G,S_kv,D] with element strides ksb/ksg/kss
    const void *V;
    void *O;        // [B,S,G,h,D]
    float *lse;     // [B,S,G,h] or null
    int B, S, G, h, Dk, Dv, S_kv;
    int64_t ksb, ksg, kss, vsb, vsg, vss;
    float scale;
    int t0, a, dd, c, w;
    float *part;  // split-KV partial records (few rows) or null
    int nsplit;
    int map_mode;  // 0 linear, 1 workgroup = 4 token groups of one (b,g), 2 = 1 + XCD-aware order
    int tpw;       // tokens per wave
    int defer_combine;  // split-KV: leave the partial records for the caller's own combine pass
    // ragged form (nsa_band_attn_fwd_ragged): device [B] positions or null; with it query row (b, t) sits at t_pos[b] + t instead of t0 + t,
    // and a sequence outside [0, t_max - S + 1] or whose last row's interval would end past S_kv has every interval empty (band_pos)
    const int32_t *t_pos;
    int t_max;
};
__host__ __device__ inline int band_hi(int t0, int a, int dd, int c, int S_kv, int t) {
    const int e = t0 + t + 1 - a;
    if (e < 0) return 0;
    const int hi = e / dd + c;
    return hi < S_kv ? hi : S_kv;
}
// the position of sequence b's first query row and whether the sequence is live: the launch's t0, or with a position array t_pos[b] -- one
// scalar load per wave (b is wave uniform).  Not live: a padding slot (negative position), a position past the caller's bound t_max, or
// one whose last row would need keys the buffers do not hold; band_row_hi then gives 0 for every row, the existing empty-interval case
// (zero output rows, lse = -inf).  No silent clamp.
struct BandPos {
    int t0;
    bool live;
};
__device__ __forceinline__ BandPos band_pos(const BandAttnParams &P, int b) {
    if (!P.t_pos) return BandPos{P.t0, true};
    const int t0 = P.t_pos[b], last = t0 + P.S - 1;
    const int e = last + 1 - P.a;
    return BandPos{t0, t0 >= 0 && last <= P.t_max && (e < 0 || e / P.dd + P.c <= P.S_kv)};
}
__device__ __forceinline__ int band_row_hi(const BandAttnParams &P, const BandPos &bp, int t) {
    return bp.live ? band_hi(bp.t0, P.a, P.dd, P.c, P.S_kv, t) : 0;
}
// paged form (nsa_band_attn_fwd_paged): K / V are pools [n_pages, G, page_rows, D], key row r of sequence b is row r & (page_rows - 1) of
// pool page table[b * stride + (r >> shift)].  An argument block of its own behind BandAttnParams (which sits twice inside DecBandPair: a
// member there would move the kernarg offsets of every decode-step kernel).  In that launch P.ksb / P.vsb are the PAGE strides and P.S_kv
// the capacity max_pages * page_rows.
struct BandPageTable {
    const int32_t *table;  // device [B, max_pages] int32
    int64_t stride;        // elements between its rows
    int n_pages;           // pages of the pools: a needed entry outside [0, n_pages) makes the sequence inactive
    int shift;             // log2(page_rows), 5 .. 16
};
size_t band_attn_workspace(int B, int S, int G, int h, int Dk, int Dv, int dtype, int *nsplit_out);
// pt: the paged form -- the PAGED instantiations (LDS-DMA staging, the ragged call's three forms); needs P.t_pos
int launch_band_attn_fwd_mfma(const BandAttnParams &P, int dtype, hipStream_t st, const BandPageTable *pt = nullptr);
// band_attn_paged.hip: the PAGED kernels live in a translation unit of their own -- new instantiations inside band_attn_mfma.hip's module
// change the inlining order, and with it the registers and code, of that module's existing D = 128 kernels.  One launch of the form the
// caller planned (nt column tiles, split or not); the caller checks the launch.
void launch_band_attn_paged_kernel(const BandAttnParams &P, const BandPageTable &pt, int dtype, int nt, bool split, unsigned grid, size_t lds, hipStream_t st);
int launch_band_attn_fwd_dual(const BandAttnParams &P0, const BandAttnParams &P1, int dtype, hipStream_t st);
// the sliding (w) and compressed (c) branch of a decode step as extra workgroups of ANOTHER launch (the one-launch decode step of the
// selected branch): workgroups [n_sel, n_sel + n_w) take w, those behind them c; every wave of such a workgroup is one (row, split) unit
// mg.on: the splits of a (row, branch) unit are the consecutive waves of ONE workgroup (nsplit divides the workgroup's waves) and are merged
// through LDS by those waves -- the branch output O is final in the activation dtype (the arithmetic of the decode finish kernel's merge, bit
// for bit), no partial record goes to memory; the sliding branch's unit also evaluates the row's gate probabilities into gates [R,3]
struct BandMergeArgs {
    int on;
    int Hd;
    float tau;
    const void *gw1, *gb1, *gw2, *gb2;  // gate MLP (fc1 weight / bias, fc2 weight / bias)
    float *gates;
};
struct DecBandPair {
    BandAttnParams w, c;
    BandMergeArgs mg;
    unsigned n_sel;  // workgroups of the host kernel's own work (0xffffffff: the launch carries no band work)
    unsigned n_w;    // workgroups of the sliding branch
};
// argument blocks of the one-launch decode step (here so that the host check of the dispatch layer reads them too): the row's selection
// attention (sel_attn_decode.hpp) and the scoring part (sel_decode_fused.hip)
struct DecAttnArgs {
    const void *Q;  // [R,h,D]
    const void *K;  // [B,G,S_kv,D] strided
    const void *V;
    void *O;        // [R,h,D]
    int G, h, S_kv, n;
    int64_t ksb, ksg, kss, vsb, vsg, vss;
    float c2;  // scale * log2(e)
};
struct DecStepParams {
    const void *Q;   // [R,h,D]
    const void *Kc;  // [B,G,S_cmp,D] strided
    float *part_g;   // SPLIT: [R][h][64][2] per-chunk (max, sum exp2)
    float *halo_g;   // SPLIT: [R][64][16] scaled logit of every chunk's last row, per head
    float *pg_g;     // SPLIT: [R][2048] group scores of the row's blocks
    int *cnt;        // SPLIT: [2][R] arrivals (records published) and tickets (scores published); zero between launches
    int R, G, h, S_cmp, S_sel, NS, nchunk, cpg, t_token, spin;
    int64_t csb, csg, css;
    float c2;
    int S;           // rows form: query rows per sequence, row (b, s, g) at token t_token + s (in the struct's tail padding: the layout of the rest is unchanged)
    // ragged form of the rows form (nsa_sel_decode_ragged): device [B] positions or null; with it row (b, s, g) sits at t_pos[b] + s, and a
    // sequence with t_pos[b] < 0 or t_pos[b] + S - 1 > min(t_max, S_kv - 1) reads nothing and gets zero O and ranges rows
    const int32_t *t_pos;
    int t_max;
    // paged form of the ragged form (nsa_sel_decode_paged; the kernel's PAGED instantiations alone read these): the caches are pools of
    // pages of DEC_PAGE_TOKENS tokens (K / V) and DEC_PAGE_TOKENS / 16 compressed rows (K_cmp); entry j of row b of the table is the pool
    // page of the sequence's tokens [1024 j, 1024 j + 1024).  csb (here) and ksb / vsb (DecAttnArgs) are then the PAGE strides, S_kv the
    // capacity max_pages * 1024; a sequence with a needed entry outside [0, n_pages) is inactive like one with a position out of bounds
    int n_pages;
    const int32_t *block_table;  // device [B, max_pages] int32, row stride bt_stride
    int64_t bt_stride;
};
constexpr int DEC_PAGE_TOKENS = 1024;  // one scorer chunk (64 compressed rows at d = 16) = 16 selection blocks of 64
// fills tpw of both argument blocks and returns the (row, split) units = waves of each; false: not both in split form with deferred combine
bool band_dual_plan(BandAttnParams *P0, BandAttnParams *P1, int dtype, int64_t waves[2]);
int launch_band_attn_bwd_dq(const BandAttnParams &P, const void *dO, const float *lse, const float *delta, void *dQ, int dtype,
                            hipStream_t st);
int launch_bwd_delta(const void *O, const void *dO, float *delta, int64_t n_rows, int Dv, int dtype, hipStream_t st);
int launch_band_ranges(int32_t *ranges, const BandAttnParams &P, hipStream_t st);  // the band as one [lo, hi) range per row
int launch_band_attn_fwd_generic(const BandAttnParams &P, int dtype, hipStream_t st);

// ---- what the MFMA attention kernels (selection forward and backward, band) ask, stated once.  The shapes they cover:
inline bool attn_mfma_shape_ok(int dtype, int h, int Dk, int Dv) {
    return (dtype == NSA_DT_BF16 || dtype == NSA_DT_F16) && Dk == Dv && (Dk == 64 || Dk == 128) && h >= 1 && h <= 16;
}
// Their operands (A: the host's AttnCall or any of the kernel blocks above):
// 16-byte loads and LDS-DMA pieces at K + b ksb + g ksg + row kss: every K / V stride a multiple of 8 elements, Q, K and V 16-byte aligned
template <class A>
inline bool qkv_aligned(const A &a) {
    return a.kss % 8 == 0 && a.vss % 8 == 0 && a.ksb % 8 == 0 && a.vsb % 8 == 0 && a.ksg % 8 == 0 && a.vsg % 8 == 0 && ((uintptr_t)a.Q % 16 == 0) &&
           ((uintptr_t)a.K % 16 == 0) && ((uintptr_t)a.V % 16 == 0);
}
// the forward kernels' extras: 8-byte stores of O rows, and the K / V slab of one (b,g) under 2 GiB (buffer addressing)
template <class A>
inline bool out_aligned(const A &a) {
    return (uintptr_t)a.O % 8 == 0;
}
template <class A>
inline bool slabs_under_2gib(const A &a) {
    return (int64_t)a.S_kv * a.kss * 2 < ((int64_t)1 << 31) && (int64_t)a.S_kv * a.vss * 2 < ((int64_t)1 << 31);
}

struct AttnCall;  // nsa_host.hpp: the arguments of the attention family's entry points
int launch_sel_attn_fwd_generic(const SelAttnParams &P, int dtype, hipStream_t st);
int launch_sel_attn_bwd_generic(const SelAttnBwdParams &P, int dtype, hipStream_t st);
int launch_sel_first_key(const SelAttnParams &P, int dtype, hipStream_t st);    // parity mode of the packed / gather executors (reads V, ranges, O)
int launch_sel_head_causal(const SelAttnParams &P, int dtype, hipStream_t st);  // parity mode of _sdpa_over_ranges
// decode form (S = 1): one 1024-thread workgroup per row, partials merged through LDS (sel_attn_decode.hpp)
bool sel_attn_decode_wg_shape_ok(int dtype, int h, int Dk, int Dv, int n);  // shape / tuning part of the next one
bool sel_attn_decode_wg_supported(const AttnCall &c);
int launch_sel_attn_decode_wg(const SelAttnParams &P, int dtype, hipStream_t st);
size_t sel_attn_mfma_workspace(int64_t R, int h, int Dv, int *nsplit_out);
// The kernel form launch_sel_attn_fwd_mfma runs a filled block in, decided here alone.  SPLIT: few rows, the keys of a row over P.nsplit waves;
// BLOCKS: 64-key blocks, nt column tiles of 16/h rows per wave (flat: 8 rows over 3 tiles; ksplit: key classes on different XCDs, records in
// P.ks_ws); ROWS: query tiles of tpw rows per wave, nt column tiles; ONE_ROW: one row per wave
struct SelAttnForm {
    enum Kind { SPLIT, BLOCKS, ROWS, ONE_ROW } kind;
    int nt, tpw;
    bool flat, ksplit;
};
SelAttnForm sel_attn_mfma_form(const SelAttnParams &P, int dtype);
int launch_sel_attn_fwd_mfma(const SelAttnParams &P, int dtype, hipStream_t st);
// key-split form of the block kernel: bytes of partial records it needs, 0 = not wanted for this shape (rule / tuning in sel_attn_blocks_mfma.hip)
size_t sel_attn_ksplit_workspace(int dtype, int h, int Dk, int Dv, int S, int S_kv, int n, int64_t R);
// the forms' own shape rules (0 = not covered) and launchers: for sel_attn_mfma_form / launch_sel_attn_fwd_mfma alone
int sel_attn_rows_tpw(const SelAttnParams &P, int dtype, int *nt);
int sel_attn_blocks_nt(const SelAttnParams &P, int dtype);
int launch_sel_attn_rows_mfma(const SelAttnParams &P, int dtype, const SelAttnForm &f, hipStream_t st);
int launch_sel_attn_blocks_mfma(const SelAttnParams &P, int dtype, const SelAttnForm &f, hipStream_t st);
size_t sel_attn_bwd_mfma_workspace(int64_t R, int h, int S, int64_t nbg, int S_kv, int D);  // D = Dk = Dv
int launch_sel_attn_bwd_mfma(const SelAttnBwdParams &P, int dtype, float *delta_ws, hipStream_t st);

}  // namespace nsa
