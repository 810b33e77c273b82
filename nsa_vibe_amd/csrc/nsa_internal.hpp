// Internal forms of the C-ABI entry points and the launchers behind them.  Every family takes its argument block (nsa_host.hpp: AttnCall with
// Band / AttnGrads, SelDecodeCall, ScoresCall, SelectCall), filled once by the entry point or built from the block the caller already holds.
// The attention forwards add the split-KV hand-over used by the fused decode step (defer != 0: the partial records stay in the workspace,
// *ns_used tells how many splits were written; 1 = O is final).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace nsa {

struct AttnCall;   // nsa_host.hpp: the arguments of the attention family (nsa_sel_attn_* / nsa_band_attn_* / nsa_sel_select_attn_fwd)
struct Band;       // nsa_host.hpp: the band of a band-attention call
struct AttnGrads;  // nsa_host.hpp: dO, dQ, dK, dV
struct SelectCall;  // nsa_host.hpp: the top-n selection of a call's rows
int sel_attn_fwd_impl(const AttnCall &c, int defer, int *ns_used);
int band_attn_fwd_impl(const AttnCall &c, const Band &band, int defer, int *ns_used);
int sel_attn_bwd_impl(const AttnCall &c, const AttnGrads &g);
// top-n ranges of the call's rows from p_grp [R, S_sel] into s.ranges_out (= c.ranges), then the attention over them: one launch or two
int sel_select_attn_impl(const float *p_grp, int S_sel, int l_sel, const SelectCall &s, const AttnCall &c);
// The route of an attention forward (selection or band), decided in one function each.  fast_ok: the MFMA kernels cover the shape and can
// read the operands (band: with the forward's extras, out_aligned and slabs_under_2gib); nsplit: the splits of a row the shape asks for (few
// rows); ws: the call's workspace holds the split records, may hold the block form's key-split records (selection), or is not used
struct AttnRoute {
    enum Kind { ZERO_FILL, DECODE_WG, MFMA, GENERIC } kind;
    enum Ws { WS_NONE, WS_SPLIT, WS_KSPLIT } ws;
    bool fast_ok;
    int nsplit;
};
AttnRoute sel_attn_route(const AttnCall &c);
AttnRoute band_attn_route(const AttnCall &c, const Band &band);
struct DecBandPair;    // sel_attn_params.hpp
struct SelDecodeCall;  // nsa_host.hpp: the arguments of nsa_sel_decode_step / nsa_sel_decode_rows (S tokens per sequence from t0 on; the step: S = 1)
// band / band_taken: the layer step's sliding + compressed branches (split form, deferred combine); *band_taken = 1 when the selected branch ran
// as the one-launch decode step and carried them on its launch (otherwise the caller launches them itself)
int sel_decode_step_impl(const SelDecodeCall &c, void *workspace, size_t workspace_bytes, void *stream, int defer, int *ns_used, float **part_used,
                         const DecBandPair *band = nullptr, int *band_taken = nullptr);
int sel_decode_rows_impl(const SelDecodeCall &c, void *workspace, size_t workspace_bytes, void *stream);

struct ScoresCall;  // nsa_host.hpp: the arguments of the scorer family (nsa_sel_scores* and every launcher below them)
struct SelectParams;  // sel_scores_params.hpp
// scores + top-n of a decode step's rows in one launch (sel_scores.hip): the shape / tuning part, and with the operands' alignment
bool decode_score_select_shape_ok(const ScoresCall &c);
bool decode_score_select_supported(const ScoresCall &c);
int launch_decode_score_select(const ScoresCall &c, const SelectCall &s, int stencil);
// the one-launch decode step (sel_decode_fused.hip): default block geometry, bf16 / f16, Dk = Dv = 64 or 128
bool decode_step_supported(const SelDecodeCall &c);
size_t decode_step_workspace(int64_t R, int h, int S_cmp);
int launch_decode_step(const SelDecodeCall &c, void *ws, size_t ws_bytes, hipStream_t st, const DecBandPair *band = nullptr);
// shape / tuning part of decode_step_supported (default block geometry; the tensors are not read): false = declined (form -1, nsplit 0)
bool decode_step_shape_plan(const SelDecodeCall &c, int *form, int *nsplit);
// rows form of the one-launch step (nsa_sel_decode_rows): S consecutive tokens per sequence at t0 .. t0 + S - 1, one workgroup per row
bool decode_rows_shape_plan(const SelDecodeCall &c, int *form, int *nw_out);
bool decode_rows_supported(const SelDecodeCall &c);
// what every form asks of the call beyond its shape: default block geometry, an aligned K_cmp, the operands of the row's attention
bool decode_step_operands_ok(const SelDecodeCall &c);
// compressed rows a decode step at token t sees, default geometry (l = 32, d = 16)
__host__ __device__ inline int decode_ncmp(int t) { return t + 1 < 32 ? 0 : (t + 1 - 32) / 16 + 1; }
// t_pos (device, [B]) / t_max: the ragged form (nsa_sel_decode_ragged) -- row (b, s, g) at t_pos[b] + s, planned from t_max
// pt: the paged form (nsa_sel_decode_paged) -- the caches are pools of pages found through a device table, c.S_kv the capacity max_pages * 1024
struct DecPageTable {
    const int32_t *table;  // device [B, max_pages] int32
    int64_t stride;        // elements between its rows
    int n_pages;           // pages of the pools: entries outside [0, n_pages) make a sequence inactive
};
int launch_decode_rows(const SelDecodeCall &c, hipStream_t st, const int32_t *t_pos = nullptr, int t_max = 0, const DecPageTable *pt = nullptr);
// shape / tuning part of the ragged form's predicate, from the host bound t_max alone (the position array is never read on the host);
// *why (optional): the limit a declined shape ran into
bool decode_ragged_shape_plan(const SelDecodeCall &c, int t_max, int *form, int *nw_out, const char **why);
int sel_decode_ragged_impl(const SelDecodeCall &c, const int32_t *t_pos, int t_max, void *stream);
// the paged form's plan: the ragged form's with one (page, group) plane of 1024 rows as the extent of the 32-bit offsets
bool decode_paged_shape_plan(const SelDecodeCall &c, int t_max, int *form, int *nw_out, const char **why);
int sel_decode_paged_impl(const SelDecodeCall &c, const DecPageTable &pt, int max_pages, int page_tokens, const int32_t *t_pos, int t_max, void *stream);
// the band forward with per-sequence positions (nsa_band_attn_fwd_ragged): band.t0 is ignored
int band_attn_fwd_ragged_impl(const AttnCall &c, const Band &band, const int32_t *t_pos, int t_max);
// the ragged band forward over paged caches (nsa_band_attn_fwd_paged): c.K / c.V are the pools, c.ksb / c.vsb their page strides, c.S_kv is
// ignored (the capacity is max_pages * page_rows); pt.shift is filled from page_rows
struct BandPageTable;  // sel_attn_params.hpp
int band_attn_fwd_paged_impl(const AttnCall &c, const Band &band, const BandPageTable &pt, int max_pages, int page_rows, const int32_t *t_pos, int t_max);

// ---- the scorer and selector family behind the C ABI (nsa_api.hip): what nsa_sel_scores[_rows], nsa_sel_scores_select[_rows] and
// nsa_select_topn_ranges run once their arguments are in the blocks
int sel_scores_impl(ScoresCall c, int variant);
int sel_scores_select_impl(ScoresCall c, const SelectCall &s);
int select_topn_impl(const float *p_grp, int64_t R, int S, int G, int S_sel, int l_sel, const SelectCall &s, hipStream_t st);
// The scorer's route: 1 generic (pcmp + map), 2 the tiled MFMA scorers, 3 the decode-shaped pair.  `route` rests on the shape, dtype, block
// geometry, variant and norm alone (what the workspace and plan queries ask: no tensors); `mfma` adds the operands: Q / K_cmp also allow
// the MFMA kernels of that route (kcmp_aligned; on route 3 the MFMA form of decode_logits).  norm = 1 (decode-normalised rows of an
// extend): the decode-shaped pair only for chunks of fewer than 64 rows, so that chunks whose boundaries are multiples of 64 all take the
// same (prefill) route and a row's scores do not depend on the chunk it sits in
struct ScoresRoute {
    int route;
    bool decode_fits;  // the decode-shaped pair holds the h heads' queries in LDS
    bool mfma;
};
ScoresRoute scores_route(const ScoresCall &c, int variant);
constexpr int64_t DECODE_MAX_ROWS = 1024;  // rows (B*S*G) up to which the decode-shaped scorer is used

// ---- launchers the C ABI dispatches to; every translation unit that defines one includes this header, so a definition whose return type
// disagrees does not compile (a changed parameter list still declares an overload and fails at link time).
// sel_select.hip
int launch_select_topn(const SelectParams &P, hipStream_t st);
int launch_indices_to_ranges(const int32_t *idx, int64_t R, int S, int G, int t0, int K, int S_sel, int l_sel, int32_t *out, hipStream_t st);
int batched_width(int S, int S_sel, int l_sel, int n_top, int force_init, int force_local);
// sel_scores.hip
int launch_map_pcmp(const float *p_cmp, int64_t R, int h, int S_cmp_cur, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals,
                    int S_sel, float *p_slc, float *p_grp, hipStream_t st);
int launch_pcmp(const ScoresCall &c, int64_t row0, int64_t nrows);  // rows [row0, row0 + nrows) -> c.ws
size_t scores_workspace(int64_t R, int h, int S_cmp);
int launch_sel_scores(const ScoresCall &c);
size_t decode_scores_workspace(int64_t R, int h, int S_cmp);
int launch_decode_scores(const ScoresCall &c);
// sel_scores_mfma.hip
bool scores_mfma_supported(const ScoresCall &c);  // bf16 / f16, Dk 64 or 128, h <= 16, the default block geometry l = 2d, l' = 4d
// sel / sel_done: the caller wants the top-n ranges of every row too; *sel_done says whether the launch produced them
int launch_sel_scores_mfma(const ScoresCall &c, const SelectParams *sel, int *sel_done);

}  // namespace nsa
