// C ABI of the layer-level entry points (include/nsa_sel_hip.h, "Layer-level entry points").
#include "nsa_host.hpp"
#include "nsa_internal.hpp"

using namespace nsa;

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

static int check_layer(const nsa_layer_desc *L, const char *who) {
    NSA_CHECK_ARG(L, "%s: null layer descriptor", who);
    NSA_CHECK_ARG(dtype_ok(L->dtype), "%s: unknown dtype %d", who, L->dtype);
    NSA_CHECK_ARG(L->dim >= 1 && L->G >= 1 && L->h >= 1 && L->Dk >= 2 && L->Dv >= 1 && L->Dk % 2 == 0 && L->Dv % 2 == 0,
                  "%s: bad geometry (Dk, Dv must be even)", who);
    NSA_CHECK_ARG(L->l >= 1 && L->d >= 1 && L->l_sel >= 1 && L->n_sel >= 1 && L->w >= 0, "%s: bad block parameters", who);
    return NSA_OK;
}
static int check_kv(const nsa_kv_desc *kv, const char *who) {
    NSA_CHECK_ARG(kv && kv->K_sel && kv->V_sel && kv->K_win && kv->V_win && kv->K_raw && kv->V_raw && kv->K_cmp && kv->V_cmp,
                  "%s: null cache pointer", who);
    NSA_CHECK_ARG(kv->B >= 1 && kv->S_max >= 1 && kv->n_cmp_max >= 1, "%s: bad cache sizes", who);
    return NSA_OK;
}

extern "C" {

int nsa_linear_small(const void *A, const void *W, void *out, int M, int N, int K, int dtype, int epilogue, const void *residual, void *stream) {
    NSA_CHECK_ARG(dtype_ok(dtype), "linear_small: unknown dtype %d", dtype);
    NSA_CHECK_ARG(M >= 0 && N >= 0 && K >= 1, "linear_small: bad sizes");
    NSA_CHECK_ARG(epilogue >= 0 && epilogue <= 2 && (epilogue != 2 || residual), "linear_small: bad epilogue");
    if (M == 0 || N == 0) return NSA_OK;
    NSA_CHECK_ARG(A && W && out, "linear_small: null pointer");
    return launch_linear_small_epi(LinearCall{A, W, out, M, N, K, dtype, epilogue, residual, (hipStream_t)stream});
}

int nsa_rmsnorm_rows(const void *x, const void *w, void *y, int M, int dim, float eps, int dtype, void *stream) {
    NSA_CHECK_ARG(dtype_ok(dtype), "rmsnorm_rows: unknown dtype %d", dtype);
    NSA_CHECK_ARG(M >= 0 && dim >= 1, "rmsnorm_rows: bad sizes");
    if (M == 0) return NSA_OK;
    NSA_CHECK_ARG(x && w && y, "rmsnorm_rows: null pointer");
    return launch_rmsnorm_rows(x, w, y, M, dim, eps, dtype, (hipStream_t)stream);
}

size_t nsa_rmsnorm_rows_bwd_workspace(int M, int dim) { return M > 0 && dim > 0 ? rmsnorm_rows_bwd_workspace(M, dim) : 0; }

int nsa_rmsnorm_rows_bwd(const void *x, const void *w, const void *dy, void *dx, void *dw, int M, int dim, float eps, int dtype,
                         void *workspace, size_t workspace_bytes, void *stream) {
    NSA_CHECK_ARG(dtype_ok(dtype), "rmsnorm_rows_bwd: unknown dtype %d", dtype);
    NSA_CHECK_ARG(M >= 1 && dim >= 1, "rmsnorm_rows_bwd: bad sizes");
    NSA_CHECK_ARG(x && w && dy && dx && dw, "rmsnorm_rows_bwd: null pointer");
    return launch_rmsnorm_rows_bwd(x, w, dy, dx, dw, M, dim, eps, dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

int nsa_rope_cache_append(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *proj, void *Q_out, int S, int t0,
                          void *stream) {
    if (int rc = check_layer(L, "rope_cache_append")) return rc;
    if (int rc = check_kv(kv, "rope_cache_append")) return rc;
    NSA_CHECK_ARG(S >= 0 && t0 >= 0 && t0 + S <= kv->S_max, "rope_cache_append: tokens [%d,%d) exceed the cache capacity %d", t0, t0 + S,
                  kv->S_max);
    if (S == 0) return NSA_OK;
    NSA_CHECK_ARG(proj && Q_out, "rope_cache_append: null pointer");
    return launch_rope_cache_append(rope_append_params(L, kv, proj, Q_out, S, t0), L->dtype, (hipStream_t)stream);
}

int nsa_cmp_pool_append(const nsa_layer_desc *L, const nsa_kv_desc *kv, int j0, int j1, void *stream) {
    if (int rc = check_layer(L, "cmp_pool_append")) return rc;
    if (int rc = check_kv(kv, "cmp_pool_append")) return rc;
    NSA_CHECK_ARG(j0 >= 0 && j1 >= j0 && j1 <= kv->n_cmp_max, "cmp_pool_append: tokens [%d,%d) exceed n_cmp_max %d", j0, j1, kv->n_cmp_max);
    NSA_CHECK_ARG(j1 == j0 || (int64_t)(j1 - 1) * L->d + L->l <= kv->S_max, "cmp_pool_append: window past the cache capacity");
    CmpPoolParams P = cmp_pool_params(L, kv->B, kv->K_raw, kv->V_raw, kv->K_cmp, kv->V_cmp, kv->S_max, kv->n_cmp_max);
    P.j0 = j0; P.j1 = j1;
    return launch_cmp_pool(P, L->dtype, (hipStream_t)stream);
}

int nsa_gate_combine(const nsa_layer_desc *L, const void *Q, const void *O_cmp, const void *O_sel, const void *O_win, void *O_out,
                     float *gates_out, int64_t R, void *stream) {
    if (int rc = check_layer(L, "gate_combine")) return rc;
    NSA_CHECK_ARG(R >= 0, "gate_combine: negative size");
    if (R == 0) return NSA_OK;
    NSA_CHECK_ARG(Q && O_cmp && O_sel && O_win && O_out && L->gate_w1 && L->gate_b1 && L->gate_w2 && L->gate_b2, "gate_combine: null pointer");
    GateCombineParams P{};
    P.Q = Q; P.O_cmp = O_cmp; P.O_sel = O_sel; P.O_win = O_win; P.O_out = O_out; P.gates_out = gates_out;
    P.w1 = L->gate_w1; P.b1 = L->gate_b1; P.w2 = L->gate_w2; P.b2 = L->gate_b2;
    P.R = R; P.h = L->h; P.Dk = L->Dk; P.Dv = L->Dv; P.Hd = L->gate_hidden; P.tau = L->gate_tau;
    return launch_gate_combine(P, L->dtype, (hipStream_t)stream);
}

int nsa_rope_cache_append_bwd(const nsa_layer_desc *L, int B, int S, int t0, const void *dQ, const void *dK_sel, const void *dV_sel,
                              const void *dK_win, const void *dV_win, const void *dK_raw, const void *dV_raw, void *dproj, void *stream) {
    if (int rc = check_layer(L, "rope_cache_append_bwd")) return rc;
    NSA_CHECK_ARG(B >= 0 && S >= 0 && t0 >= 0, "rope_cache_append_bwd: negative size");
    if (B == 0 || S == 0) return NSA_OK;
    NSA_CHECK_ARG(dQ && dproj, "rope_cache_append_bwd: null pointer");
    // the forward's argument block with the gradients in the tensors' places: dproj is written, dQ and the "cache" of capacity S are read
    nsa_kv_desc g{};
    g.K_sel = (void *)dK_sel; g.V_sel = (void *)dV_sel; g.K_win = (void *)dK_win; g.V_win = (void *)dV_win;
    g.K_raw = (void *)dK_raw; g.V_raw = (void *)dV_raw;
    g.B = B; g.S_max = S;
    return launch_rope_cache_append_bwd(rope_append_params(L, &g, dproj, (void *)dQ, S, t0), L->dtype, (hipStream_t)stream);
}

int nsa_cmp_pool_bwd(const nsa_layer_desc *L, int B, int S, int n_cmp, const void *dK_cmp, const void *dV_cmp, void *dK_raw, void *dV_raw,
                     void *stream) {
    if (int rc = check_layer(L, "cmp_pool_bwd")) return rc;
    NSA_CHECK_ARG(B >= 0 && S >= 0 && n_cmp >= 0, "cmp_pool_bwd: negative size");
    if (B == 0 || S == 0) return NSA_OK;
    NSA_CHECK_ARG(dK_raw && dV_raw && ((dK_cmp && dV_cmp) || n_cmp == 0), "cmp_pool_bwd: null pointer");
    NSA_CHECK_ARG(n_cmp == 0 || (int64_t)(n_cmp - 1) * L->d + L->l <= S, "cmp_pool_bwd: windows reach past S");
    const CmpPoolParams P = cmp_pool_params(L, B, nullptr, nullptr, nullptr, nullptr, 0, 0);  // (the geometry and the rotation alone)
    return launch_cmp_pool_bwd(P, dK_cmp, dV_cmp, dK_raw, dV_raw, S, n_cmp, L->dtype, (hipStream_t)stream);
}

int nsa_gate_combine_bwd(const nsa_layer_desc *L, const void *dO, const void *O_cmp, const void *O_sel, const void *O_win, const float *gates,
                         void *dO_cmp, void *dO_sel, void *dO_win, float *dgates, int64_t R, void *stream) {
    if (int rc = check_layer(L, "gate_combine_bwd")) return rc;
    NSA_CHECK_ARG(R >= 0, "gate_combine_bwd: negative size");
    if (R == 0) return NSA_OK;
    NSA_CHECK_ARG(dO && O_cmp && O_sel && O_win && gates && dO_cmp && dO_sel && dO_win && dgates, "gate_combine_bwd: null pointer");
    GateCombineParams P{};
    P.O_cmp = O_cmp; P.O_sel = O_sel; P.O_win = O_win;
    P.R = R; P.h = L->h; P.Dk = L->Dk; P.Dv = L->Dv;
    return launch_gate_combine_bwd(P, dO, gates, dO_cmp, dO_sel, dO_win, dgates, L->dtype, (hipStream_t)stream);
}

// workspace of a layer call over S rows at positions t0 .. t0 + S - 1 (prefill: t0 = 0):
// Q | p_grp | O_cmp | O_sel | O_win | scorer scratch | attention scratch | band scratch (all sized by the S rows; only the attention's
// key-split records and the scorer's columns grow with the context t0 + S).  norm: the scorer's flag (its route depends on it)
struct RowsWs {
    size_t q, pgrp, ocmp, osel, owin, sc, att, band, total, sc_bytes, att_bytes, band_bytes;
};
static RowsWs rows_ws(const nsa_layer_desc *L, int B, int S, int t0, int S_sel, int norm) {
    RowsWs w;
    const size_t e = esize(L->dtype);
    const size_t NQ = (size_t)L->G * L->h * L->Dk, NO = (size_t)L->G * L->h * L->Dv;
    const int S_kv = t0 + S;
    const int n_cmp = ncmp_of(S_kv, L->l, L->d);
    size_t o = 0;
    w.q = o; o += up256((size_t)B * S * NQ * e);
    w.pgrp = o; o += up256(sizeof(float) * (size_t)B * S * L->G * (size_t)(S_sel > 0 ? S_sel : 1));
    w.ocmp = o; o += up256((size_t)B * S * NO * e);
    w.osel = o; o += up256((size_t)B * S * NO * e);
    w.owin = o; o += up256((size_t)B * S * NO * e);
    w.sc_bytes = nsa_sel_scores_rows_workspace(B, S, L->G, L->h, L->Dk, n_cmp, S_sel, L->l, L->d, L->l_sel, L->dtype, 0, norm);
    const size_t sc1 = nsa_sel_scores_rows_workspace(B, S, L->G, L->h, L->Dk, n_cmp, S_sel, L->l, L->d, L->l_sel, L->dtype, 1, norm);
    if (sc1 > w.sc_bytes) w.sc_bytes = sc1;  // the generic route may be taken for unaligned inputs
    w.sc = o; o += up256(w.sc_bytes);
    w.att_bytes = nsa_sel_attn_fwd_workspace_kv(B, S, L->G, L->h, L->Dk, L->Dv, S_kv, L->n_sel, L->dtype);
    w.att = o; o += up256(w.att_bytes);
    w.band_bytes = nsa_band_attn_fwd_workspace(B, S, L->G, L->h, L->Dk, L->Dv, L->dtype);
    w.band = o; o += up256(w.band_bytes);
    w.total = o;
    return w;
}

// The layer over S rows at positions t0 .. t0 + S - 1 of the caches: RoPE + append, pooling, the three branches, gate mix.
// norm = 0 with t0 = 0 is the prefill (scores normalised over all columns, either selector, out_width ranges per row); norm = 1 is the
// extend (decode semantics: every row normalises over its own columns and selects sequentially at its token).
static int layer_rows(const char *who, const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *proj, int t0, int S, int selector, int norm,
                      const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, int out_width,
                      void *O_mix, float *gates_out, void *workspace, size_t workspace_bytes, void *stream) {
    const bool prefill = norm == 0;
    if (int rc = check_layer(L, who)) return rc;
    if (int rc = check_kv(kv, who)) return rc;
    NSA_CHECK_ARG(proj && O_mix && ranges_out, "%s: null pointer", who);
    if (prefill)
        NSA_CHECK_ARG(S >= 1 && S <= kv->S_max, "%s: %d tokens exceed the cache capacity %d", who, S, kv->S_max);
    else
        NSA_CHECK_ARG(t0 >= 0 && S >= 1 && (int64_t)t0 + S <= kv->S_max, "%s: tokens [%d,%d) exceed the cache capacity %d", who, t0, t0 + S,
                      kv->S_max);
    NSA_CHECK_ARG(S_sel >= 1 && (int64_t)S_sel * L->l_sel >= (int64_t)t0 + S, "%s: block metadata (S_sel=%d) does not cover %d tokens", who,
                  S_sel, t0 + S);
    NSA_CHECK_ARG(selector == NSA_SEL_BATCHED || selector == NSA_SEL_SEQUENTIAL, "%s: unknown selector %d", who, selector);
    const int B = kv->B, G = L->G, h = L->h, Dk = L->Dk, dt = L->dtype;
    const int S_kv = t0 + S;
    const RowsWs W = rows_ws(L, B, S, t0, S_sel, norm);
    if (int rc = check_workspace(who, workspace, workspace_bytes, W.total)) return rc;
    unsigned char *ws = (unsigned char *)workspace;
    void *Q = ws + W.q, *Ocmp = ws + W.ocmp, *Osel = ws + W.osel, *Owin = ws + W.owin;
    float *p_grp = (float *)(ws + W.pgrp);
    // compressed tokens emitted before the rows (n_cmp(t0 - 1)) and after them (n_cmp(t0 + S - 1)), on the absolute schedule
    const int n0 = ncmp_of(t0, L->l, L->d), n1 = ncmp_of(S_kv, L->l, L->d);
    NSA_CHECK_ARG(n1 <= kv->n_cmp_max, "%s: compressed cache too small", who);
    if (int rc = nsa_rope_cache_append(L, kv, proj, Q, S, t0, stream)) return rc;
    if (n1 > n0)
        if (int rc = nsa_cmp_pool_append(L, kv, n0, n1, stream)) return rc;
    const CacheStrides C(L, kv);
    // selected branch: scores of rows t0 .. t0 + S - 1 (blocks no selector can read at row t are skipped) -> top-n at their tokens -> the
    // attention over K_sel[:t + 1]
    // (causal_skip 2: skipped blocks stay unwritten, only the selector reads p_grp)
    const ScoresCall sc{Q, kv->K_cmp, p_grp, csc_ptr, csc_rows, csc_vals, B, S, G, h, Dk, n1, S_sel, C.kcb, C.kcg, Dk, L->l, L->d, L->l_sel, 2, dt, C.scale,
                        t0, norm, ws + W.sc, W.sc_bytes, (hipStream_t)stream};
    const bool aligned = kcmp_aligned(Q, kv->K_cmp, C.kcb, C.kcg, Dk);
    const SelectCall select{t0, nullptr, L->n_sel, 1, 2, selector, S, ranges_out, out_width};
    const AttnCall attend = selected_call(L, kv, C, Q, ranges_out, Osel, S, S_kv, out_width, ws + W.att, W.att_bytes, stream);
    if (!prefill || (aligned && n1 >= 1 && tuning(TUNE_SEL_FUSE) <= 0)) {
        // scores + top-n in one call (on the 32x32x16 scorer's route one LAUNCH, the selection in the scorer's epilogue), then the attention
        if (int rc = sel_scores_select_impl(sc, select)) return rc;
        if (int rc = sel_attn_fwd_impl(attend, 0, nullptr)) return rc;
    } else {  // prefill only (t0 = 0): the selector inside the attention launch (SEL_FUSE), an unaligned K_cmp, or no compressed token yet
        if (int rc = sel_scores_impl(sc, aligned ? 0 : 1)) return rc;
        if (int rc = sel_select_attn_impl(p_grp, S_sel, L->l_sel, select, attend)) return rc;
    }
    // sliding and compressed branches at the rows' absolute positions
    if (int rc = band_attn_fwd_impl(sliding_call(L, kv, C, Q, Owin, S, S_kv, ws + W.band, W.band_bytes, stream), sliding_band(t0, L->w), 0, nullptr)) return rc;
    if (int rc = band_attn_fwd_impl(compressed_call(L, kv, C, Q, Ocmp, S, n1, ws + W.band, W.band_bytes, stream), compressed_band(t0, L->l, L->d), 0, nullptr))
        return rc;
    return nsa_gate_combine(L, Q, Ocmp, Osel, Owin, O_mix, gates_out, (int64_t)B * S * G, stream);
}

size_t nsa_layer_prefill_workspace(const nsa_layer_desc *L, int B, int S, int S_sel) {
    if (!L || !dtype_ok(L->dtype) || B < 1 || S < 1) return 0;
    return rows_ws(L, B, S, 0, S_sel, 0).total;
}

int nsa_layer_prefill(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *proj, int S, int selector, const int32_t *csc_ptr,
                      const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, int out_width, void *O_mix,
                      float *gates_out, void *workspace, size_t workspace_bytes, void *stream) {
    return layer_rows("layer_prefill", L, kv, proj, 0, S, selector, 0, csc_ptr, csc_rows, csc_vals, S_sel, ranges_out, out_width, O_mix, gates_out,
                      workspace, workspace_bytes, stream);
}

size_t nsa_layer_extend_workspace(const nsa_layer_desc *L, int B, int S, int t0, int S_sel) {
    if (!L || !dtype_ok(L->dtype) || B < 1 || S < 1 || t0 < 0) return 0;
    return rows_ws(L, B, S, t0, S_sel, 1).total;
}

int nsa_layer_extend(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *proj, int t0, int S, const int32_t *csc_ptr,
                     const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, void *O_mix, float *gates_out,
                     void *workspace, size_t workspace_bytes, void *stream) {
    return layer_rows("layer_extend", L, kv, proj, t0, S, NSA_SEL_SEQUENTIAL, 1, csc_ptr, csc_rows, csc_vals, S_sel, ranges_out,
                      L ? L->n_sel : 0 /* a null L is refused there */, O_mix, gates_out, workspace, workspace_bytes, stream);
}

// workspace: proj | Q | O_cmp | O_sel | O_win | O_mix | ranges | selection-decode scratch | band scratch
// S = 0: the single step (B rows); S >= 1: the rows call, every piece sized by its B S rows
struct DecodeWs {
    size_t proj, q, ocmp, osel, owin, omix, ranges, gates, sel, band, band2, total, sel_bytes, band_bytes;
};
static DecodeWs decode_ws(const nsa_layer_desc *L, int B1, int S_max, int S = 0) {
    DecodeWs w;
    const size_t B = (size_t)B1 * (S > 0 ? S : 1);
    const size_t e = esize(L->dtype);
    const size_t NQ = (size_t)L->G * L->h * L->Dk, NO = (size_t)L->G * L->h * L->Dv;
    const int n_cmp_max = ncmp_of(S_max, L->l, L->d);
    const int S_sel_max = (S_max + L->l_sel - 1) / L->l_sel + 1;
    size_t o = 0;
    w.proj = o; o += up256(B * qkv_cols(L) * e);
    w.q = o; o += up256(B * NQ * e);
    w.ocmp = o; o += up256(B * NO * e);
    w.osel = o; o += up256(B * NO * e);
    w.owin = o; o += up256(B * NO * e);
    w.omix = o; o += up256(B * NO * e);
    w.ranges = o; o += up256(sizeof(int32_t) * B * L->G * L->n_sel * 2);
    w.gates = o; o += up256(sizeof(float) * B * L->G * 3);
    w.sel_bytes = nsa_sel_decode_step_workspace(B1, L->G, L->h, L->Dk, L->Dv, n_cmp_max, S_sel_max, L->n_sel, L->dtype);
    if (S > 0) w.sel_bytes = std::max(w.sel_bytes, nsa_sel_decode_rows_workspace(B1, S, L->G, L->h, L->Dk, L->Dv, n_cmp_max, S_sel_max, L->n_sel, L->dtype));
    w.sel = o; o += up256(w.sel_bytes);
    w.band_bytes = nsa_band_attn_fwd_workspace(B1, S > 0 ? S : 1, L->G, L->h, L->Dk, L->Dv, L->dtype);
    w.band = o; o += up256(w.band_bytes);
    w.band2 = o; o += up256(w.band_bytes);
    w.total = o;
    return w;
}

size_t nsa_layer_decode_step_workspace(const nsa_layer_desc *L, int B, int S_max) {
    if (!L || !dtype_ok(L->dtype) || B < 1 || S_max < 1) return 0;
    return decode_ws(L, B, S_max).total;
}

// One layer decode call over S rows per sequence at t0 .. t0 + S - 1: what its prologue checks, carves from the workspace and derives
struct LayerDecode {
    const nsa_layer_desc *L;
    const nsa_kv_desc *kv;
    DecodeWs W;
    unsigned char *ws;
    void *Q, *Ocmp, *Osel, *Owin, *Omix;
    int S, t0, n0, n1;  // n0 / n1: compressed tokens emitted before the rows (n_cmp(t0 - 1)) and after them (n_cmp(t0 + S - 1))
    // ragged call (nsa_layer_decode_ragged): the device positions and te = min(t_max, S_max - 1), the last token a live row can sit at.
    // Then the launches are planned for the LARGEST sequence there can be: te + 1 tokens after the call (tokens()), n1 = n_cmp(te)
    // compressed ones, t0 = max(0, te + 1 - S) (never negative: with te < S - 1 no sequence is live and every row is a zero row); every
    // kernel takes its rows' positions from t_pos
    const int32_t *t_pos;
    int te;
    // paged call (nsa_layer_decode_paged): the block table; kv then names the POOLS with one page as its extent (S_max = 1024, n_cmp_max = 64,
    // so that CacheStrides gives the page strides), t_pos is the pre-pass's t_live and te = min(t_max, max_pages 1024 - 1)
    const LayerPageTable *pg;
    int tokens() const { return t_pos ? te + 1 : t0 + S; }  // tokens the caches hold after the call (of the largest sequence)
};
constexpr int LAYER_ROWS_MAX_S = 16;

// the call at a scalar position: rows t0 .. t0 + S - 1 of every sequence, its pieces carved from the (checked) workspace
static LayerDecode layer_decode_at(const nsa_layer_desc *L, const nsa_kv_desc *kv, const DecodeWs &W, void *workspace, int S, int t0) {
    LayerDecode D{};
    D.L = L; D.kv = kv; D.W = W; D.ws = (unsigned char *)workspace;
    D.Q = D.ws + W.q; D.Ocmp = D.ws + W.ocmp; D.Osel = D.ws + W.osel; D.Owin = D.ws + W.owin; D.Omix = D.ws + W.omix;
    D.S = S; D.t0 = t0; D.n0 = ncmp_of(t0, L->l, L->d); D.n1 = ncmp_of(t0 + S, L->l, L->d);
    return D;
}

// What a call with a position array plans its launches from, and what its route answers: the largest sequence there can be (LayerDecode;
// check_bound derives it) and the launches -- 0 and why where the shape is declined
struct PositionsPlan {
    int te, t0, n1, launches;
    const char *why;
};
// the call at the positions t_pos (pg: through a block table), planned as p says
static LayerDecode layer_decode_positions(const nsa_layer_desc *L, const nsa_kv_desc *kv, const DecodeWs &W, void *workspace, int S,
                                          const PositionsPlan &p, const int32_t *t_pos, const LayerPageTable *pg = nullptr) {
    LayerDecode D = layer_decode_at(L, kv, W, workspace, S, p.t0);
    D.n0 = 0; D.n1 = p.n1; D.t_pos = t_pos; D.te = p.te; D.pg = pg;
    return D;
}

// ---- what the calls of the family check alike.  x, y and the projections' weights; with a device position array (never read on the host)
static int check_io(const char *who, const nsa_layer_desc *L, const void *x, const void *y) {
    NSA_CHECK_ARG(x && y && L->W_qkv && L->W_out, "%s: null pointer", who);
    return NSA_OK;
}
static int check_io(const char *who, const nsa_layer_desc *L, const void *x, const void *y, const int32_t *t_pos) {
    if (int rc = check_io(who, L, x, y)) return rc;
    NSA_CHECK_ARG(t_pos, "%s: null position array t_pos", who);
    NSA_CHECK_ARG((uintptr_t)t_pos % 4 == 0, "%s: t_pos must be 4-byte aligned", who);
    return NSA_OK;
}
static int check_rows_count(const char *who, int S) {
    NSA_CHECK_ARG(S >= 1 && S <= LAYER_ROWS_MAX_S, "%s: 1 to %d tokens per sequence (got %d)", who, LAYER_ROWS_MAX_S, S);
    return NSA_OK;
}
// the host bound of a position array over caches of `cap` tokens and the block metadata: *p = the planned sequence
static int check_bound(const char *who, const nsa_layer_desc *L, int S, int cap, int t_max, int S_sel, PositionsPlan *p) {
    NSA_CHECK_ARG(t_max >= 0, "%s: t_max (the host bound of t_pos[b] + S - 1) must not be negative", who);
    p->te = std::min(t_max, cap - 1);  // no live row sits beyond te
    p->t0 = std::max(0, p->te + 1 - S);
    p->n1 = ncmp_of(p->te + 1, L->l, L->d);
    NSA_CHECK_ARG(S_sel >= 1 && (int64_t)S_sel * L->l_sel >= (int64_t)p->te + 1, "%s: block metadata (S_sel=%d) does not cover %d tokens", who, S_sel,
                  p->te + 1);
    return NSA_OK;
}
// what every launch with per-sequence positions asks of the layer (each route names the limit in its own words)
static bool dtype_16bit(int dt) { return dt == NSA_DT_BF16 || dt == NSA_DT_F16; }
static bool default_decode_geometry(const nsa_layer_desc *L) {
    return L->Dk == L->Dv && (L->Dk == 64 || L->Dk == 128) && L->l == 32 && L->d == 16 && L->l_sel == 64;
}
// stands in for aligned caches in a route: its predicates read the sizes and the pointers' alignment only
static nsa_kv_desc stand_in_kv(int B, int S_max, int n_cmp_max) {
    nsa_kv_desc kv{};
    kv.K_sel = kv.V_sel = kv.K_win = kv.V_win = kv.K_raw = kv.V_raw = kv.K_cmp = kv.V_cmp = (void *)(uintptr_t)256;
    kv.B = B; kv.S_max = S_max; kv.n_cmp_max = n_cmp_max;
    return kv;
}
// a plan query's answer from its route's: (0, -1) for bad arguments (with the status) and for a declined shape, else (launches, 1)
static int plan_answer(int rc, const PositionsPlan &p, int *launches, int *route) {
    *launches = p.launches;  // (set behind the route's last check alone)
    *route = p.launches ? 1 : -1;
    return rc;
}

// rows = false: the single step at token t0 (S = 1, its own wording of the position checks, the workspace of one row per sequence)
static int layer_decode_begin(const char *who, const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *x, void *y, int t0, int S, bool rows,
                              int S_sel, void *workspace, size_t workspace_bytes, LayerDecode *D) {
    if (int rc = check_layer(L, who)) return rc;
    if (int rc = check_kv(kv, who)) return rc;
    if (int rc = check_io(who, L, x, y)) return rc;
    if (!rows) {
        NSA_CHECK_ARG(t0 >= 0 && t0 < kv->S_max, "%s: position %d outside the cache capacity %d", who, t0, kv->S_max);
        NSA_CHECK_ARG(S_sel >= 1 && (int64_t)S_sel * L->l_sel >= t0 + 1, "%s: block metadata (S_sel=%d) does not cover token %d", who, S_sel, t0);
    } else {
        if (int rc = check_rows_count(who, S)) return rc;
        NSA_CHECK_ARG(t0 >= 0 && (int64_t)t0 + S <= kv->S_max, "%s: tokens [%d,%d) exceed the cache capacity %d", who, t0, t0 + S, kv->S_max);
        NSA_CHECK_ARG(S_sel >= 1 && (int64_t)S_sel * L->l_sel >= (int64_t)t0 + S, "%s: block metadata (S_sel=%d) does not cover %d tokens", who, S_sel,
                      t0 + S);
    }
    const DecodeWs W = decode_ws(L, kv->B, kv->S_max, rows ? S : 0);
    if (int rc = check_workspace(who, workspace, workspace_bytes, W.total)) return rc;
    *D = layer_decode_at(L, kv, W, workspace, S, t0);
    return NSA_OK;
}

// The sliding and the compressed branch of the call's rows: over K_win[:t0 + S] (the last w tokens) and over the n1 compressed tokens
// (emission schedule), each with its own scratch
struct BandBranches {
    AttnCall w, c;
    Band bw, bc;
};
static BandBranches band_branches(const LayerDecode &D, const CacheStrides &C, void *stream) {
    return BandBranches{sliding_call(D.L, D.kv, C, D.Q, D.Owin, D.S, D.tokens(), D.ws + D.W.band, D.W.band_bytes, stream),
                        compressed_call(D.L, D.kv, C, D.Q, D.Ocmp, D.S, D.n1, D.ws + D.W.band2, D.W.band_bytes, stream), sliding_band(D.t0, D.L->w),
                        compressed_band(D.t0, D.L->l, D.L->d)};
}
// When the finish kernel can take split-KV partial records (Dv = 64) the branches skip their own combine kernels: one kernel then merges the
// splits of all branches, evaluates the gate and mixes
static int finish_defers(const nsa_layer_desc *L) { return L->Dv == 64 ? 1 : 0; }
// Whether both run as ONE launch (launch_band_attn_fwd_dual, or riding on the selected branch's), both in split form with the combine left to
// the finish kernel: their common split count, 0 for a launch each.  The shape, the strides and the caches' alignment decide -- Q and the
// outputs lie in the 256-byte aligned workspace.  (The whole-cache bound is this launch's own: stricter than the slab bound of the route.)
static int band_pair_splits(const nsa_layer_desc *L, const nsa_kv_desc *kv, const CacheStrides &C, int S, int t0, int tokens, int n1) {
    void *const in_ws = (void *)(uintptr_t)256;
    const AttnRoute rw = band_attn_route(sliding_call(L, kv, C, in_ws, in_ws, S, tokens, nullptr, 0, nullptr), sliding_band(t0, L->w));
    const AttnRoute rc = band_attn_route(compressed_call(L, kv, C, in_ws, in_ws, S, n1, nullptr, 0, nullptr), compressed_band(t0, L->l, L->d));
    const bool one = finish_defers(L) && rw.nsplit > 1 && rw.fast_ok && rc.fast_ok && C.ksb * 2 < ((int64_t)1 << 31) && C.vsb * 2 < ((int64_t)1 << 31);
    return one ? rw.nsplit : 0;
}
// the pair of a call that runs: BP gets the blocks of both branches
static bool band_pair(const LayerDecode &D, const CacheStrides &C, DecBandPair &BP) {
    const int nsplit = band_pair_splits(D.L, D.kv, C, D.S, D.t0, D.tokens(), D.n1);
    if (!nsplit) return false;
    const BandBranches b = band_branches(D, C, nullptr);
    BP.w = band_attn_params(b.w, b.bw);
    BP.c = band_attn_params(b.c, b.bc);
    BP.w.part = (float *)b.w.ws; BP.c.part = (float *)b.c.ws;
    BP.w.nsplit = BP.c.nsplit = nsplit;
    BP.w.defer_combine = BP.c.defer_combine = 1;
    if (D.t_pos) {  // the ragged call: every sequence at its own position (the launch's t0 is not read)
        BP.w.t_pos = BP.c.t_pos = D.t_pos;
        BP.w.t_max = BP.c.t_max = D.te;
        BP.w.t0 = BP.c.t0 = 0;
    }
    return true;
}

// the selected branch of the call as the decode family's argument block (ranges_out null: the ranges stay in the workspace)
static SelDecodeCall layer_sel_call(const LayerDecode &D, const CacheStrides &C, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals,
                                    int S_sel, int32_t *ranges_out) {
    SelDecodeCall c = sel_decode_call(D.L, D.kv, C, D.S, D.t0, D.n1, S_sel);
    if (D.t_pos) c.t0 = 0;  // as nsa_sel_decode_ragged / _paged hand it over: every row's token comes from the position array
    c.Q = D.Q; c.csc_ptr = csc_ptr; c.csc_rows = csc_rows; c.csc_vals = csc_vals; c.O = D.Osel;
    c.ranges_out = ranges_out ? ranges_out : (int32_t *)(D.ws + D.W.ranges);
    return c;
}

// the output projection of the call's rows from the mixed O (+ residual in its epilogue when given)
static LinearCall out_proj_call(const LayerDecode &D, void *y, const void *residual, void *stream) {
    const nsa_layer_desc *L = D.L;
    return LinearCall{D.Omix, L->W_out, y, D.kv->B * D.S, L->dim, L->G * L->h * L->Dv, L->dtype, residual ? 2 : 0, residual, (hipStream_t)stream};
}

// the finish kernel's block: one pass merges the splits of all three branches, evaluates the gate and mixes (ns / part: set by the branches)
static DecodeFinishParams decode_finish_params(const LayerDecode &D, float *gates_out) {
    const nsa_layer_desc *L = D.L;
    DecodeFinishParams F{};
    F.Q = D.Q; F.O_out = D.Omix; F.gates_out = gates_out;
    F.w1 = L->gate_w1; F.b1 = L->gate_b1; F.w2 = L->gate_w2; F.b2 = L->gate_b2;
    F.R = (int64_t)D.kv->B * D.S * L->G; F.h = L->h; F.Dk = L->Dk; F.Dv = L->Dv; F.Hd = L->gate_hidden; F.tau = L->gate_tau;
    F.O[0] = D.Ocmp; F.O[1] = D.Osel; F.O[2] = D.Owin;
    F.ns[0] = F.ns[1] = F.ns[2] = 1;  // every O final, until a branch leaves its split records instead
    return F;
}

// The rest of a call once its selected branch is under way.  The sliding and the compressed branch of the rows: BP = both in split form with the
// combine left to the finish kernel, as ONE launch of their own unless they rode on the selected branch's (ridden: the single step); null = one
// band_attn_fwd_impl each.  Then split combine + gates + mix (Dv = 64: the finish kernel), and the output projection of the B S rows.
static int layer_decode_tail(const LayerDecode &D, const CacheStrides &C, DecodeFinishParams &F, const DecBandPair *BP, bool ridden, float *gates_out,
                             void *y, const void *residual, void *stream) {
    const nsa_layer_desc *L = D.L;
    const nsa_kv_desc *kv = D.kv;
    hipStream_t st = (hipStream_t)stream;
    const int B = kv->B, S = D.S, G = L->G, dt = L->dtype, defer = finish_defers(L);
    if (BP) {
        if (!ridden)
            if (int rc = launch_band_attn_fwd_dual(BP->w, BP->c, dt, st)) return rc;
        F.ns[2] = F.ns[0] = BP->w.nsplit;
        F.part[2] = BP->w.part;
        F.part[0] = BP->c.part;
    } else if (D.pg) {  // the paged call: one paged launch each -- 1024-row pages of K_win / V_win, 64-row pages of K_cmp / V_cmp -- combined by the branch itself
        const BandBranches b = band_branches(D, C, stream);
        const BandPageTable pt{D.pg->table, D.pg->stride, D.pg->n_pages, 0};
        if (int rc = band_attn_fwd_paged_impl(b.w, b.bw, pt, D.pg->max_pages, LAYER_PAGE_TOKENS, D.t_pos, D.te)) return rc;
        if (int rc = band_attn_fwd_paged_impl(b.c, b.bc, pt, D.pg->max_pages, LAYER_PAGE_CMP, D.t_pos, D.te)) return rc;
    } else if (D.t_pos) {  // the ragged call: one ragged launch each, combined by the branch itself (O final)
        const BandBranches b = band_branches(D, C, stream);
        if (int rc = band_attn_fwd_ragged_impl(b.w, b.bw, D.t_pos, D.te)) return rc;
        if (int rc = band_attn_fwd_ragged_impl(b.c, b.bc, D.t_pos, D.te)) return rc;
    } else {
        const BandBranches b = band_branches(D, C, stream);
        if (int rc = band_attn_fwd_impl(b.w, b.bw, defer, &F.ns[2])) return rc;
        F.part[2] = (const float *)b.w.ws;
        if (int rc = band_attn_fwd_impl(b.c, b.bc, defer, &F.ns[0])) return rc;
        F.part[0] = (const float *)b.c.ws;
    }
    if (defer) {
        if (int rc = launch_decode_finish(F, dt, st)) return rc;
    } else {
        if (int rc = nsa_gate_combine(L, D.Q, D.Ocmp, D.Osel, D.Owin, D.Omix, gates_out, (int64_t)B * S * G, stream)) return rc;
    }
    return launch_linear_small_epi(out_proj_call(D, y, residual, stream));
}
// The tail of the rows, ragged and paged calls (O_sel is final; no residual and no folded norm: the block step alone has them): the
// pair-or-not decision is taken here, on the call's own operands.  (The paged branches have no dual launch: one paged launch each.)
static int layer_decode_rows_tail(const LayerDecode &D, const CacheStrides &C, float *gates_out, void *y, void *stream) {
    DecodeFinishParams F = decode_finish_params(D, gates_out);
    DecBandPair BP{};
    const bool dual = !D.pg && band_pair(D, C, BP);
    return layer_decode_tail(D, C, F, dual ? &BP : nullptr, false, gates_out, y, nullptr, stream);
}

static int layer_decode_step_impl(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *x, void *y, int t, const int32_t *csc_ptr,
                                  const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out,
                                  void *workspace, size_t workspace_bytes, void *stream, const void *residual, const void *norm_w,
                                  float norm_eps) {
    LayerDecode D;
    if (int rc = layer_decode_begin("layer_decode_step", L, kv, x, y, t, 1, false, S_sel, workspace, workspace_bytes, &D)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int dt = L->dtype, B = kv->B, G = L->G, h = L->h, Dk = L->Dk, Dv = L->Dv, n_cmp = D.n1;
    // 1+2. fused QKV projection with RoPE + cache append at position t in its epilogue
    if (int rc = launch_qkv_rope_append(rope_append_params(L, kv, D.ws + D.W.proj, D.Q, 1, t), qkv_call(L, x, B, norm_w, norm_eps, stream), false)) return rc;
    // 3. emit a compressed token when a window completes (nsa_attention.py:588-604)
    NSA_CHECK_ARG(n_cmp <= kv->n_cmp_max, "layer_decode_step: compressed cache too small");
    if (n_cmp > D.n0)
        if (int rc = nsa_cmp_pool_append(L, kv, D.n0, n_cmp, stream)) return rc;
    const CacheStrides C(L, kv);
    const int defer = finish_defers(L);
    DecodeFinishParams F = decode_finish_params(D, gates_out);
    // 4 + 5. the three branches.  The sliding and the compressed branch run in split-KV form with the combine left to the finish kernel; when
    // the selected branch runs as the one-launch decode step they ride on ITS launch (workgroups behind the step's own: sel_decode_fused.hip),
    // otherwise they are one launch of their own.
    DecBandPair BP{};
    const bool dual = band_pair(D, C, BP);
    const int band_mode = tuning(TUNE_DECODE_BAND);  // 0 own launch, 1 ride, 2 ride + merge in the workgroup, -1 / 3: 2 + the mix in the output projection
    const bool ride = dual && Dk == 64 && band_mode != 0;
    float *gates = gates_out ? gates_out : (float *)(D.ws + D.W.gates);
    if (ride && band_mode != 1 && h <= 16) BP.mg = BandMergeArgs{1, L->gate_hidden, L->gate_tau, L->gate_w1, L->gate_b1, L->gate_w2, L->gate_b2, gates};
    float *sel_part = nullptr;
    int band_taken = 0;
    if (int rc = sel_decode_step_impl(layer_sel_call(D, C, csc_ptr, csc_rows, csc_vals, S_sel, ranges_out), D.ws + D.W.sel, D.W.sel_bytes, stream, defer, &F.ns[1],
                                      &sel_part, ride ? &BP : nullptr, &band_taken))
        return rc;
    F.part[1] = sel_part;
    if (!(dual && band_taken && BP.mg.on)) return layer_decode_tail(D, C, F, dual ? &BP : nullptr, band_taken != 0, gates_out, y, residual, stream);
    // O_win, O_cmp (merged by the workgroups that held their splits), O_sel and the row gates are final: with few rows the mix is the
    // A operand of the output projection -- three launches per step (F.ns stays 1 for all three)
    // (measured: the mix in the projection wins up to 32 rows -- 43.3 -> 40.5 us at B = 32 -- and loses from 64 on, where every one of the
    // projection's 48 workgroups would redo the mix of all rows: 47.1 -> 50.6 us; DECODE_BAND = 3 takes it at any batch)
    const LinearCall out = out_proj_call(D, y, residual, stream);
    LinearCall mixed = out;
    mixed.A = D.Ocmp; mixed.Os = D.Osel; mixed.Ow = D.Owin; mixed.gates = gates; mixed.G = G;
    if (((band_mode < 0 && B <= 32) || band_mode == 3) && F.ns[1] == 1 && Dv == 64 && linear_small_mix_supported(mixed))
        return launch_linear_small_mix(mixed);
    // 6. split combine + gates + mix, 7. output projection
    if (int rc = launch_decode_finish(F, dt, st)) return rc;
    return launch_linear_small_epi(out);
}

int nsa_layer_decode_step(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *x, void *y, int t, const int32_t *csc_ptr,
                          const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out,
                          void *workspace, size_t workspace_bytes, void *stream) {
    return layer_decode_step_impl(L, kv, x, y, t, csc_ptr, csc_rows, csc_vals, S_sel, ranges_out, gates_out, workspace, workspace_bytes, stream,
                                  nullptr, nullptr, 0.f);
}

// ------------------------------------------------------------------------------ layer decode step for S consecutive tokens
// the launches of the call and the route of its selected branch (1 = the one-launch rows form, 0 = its separate launches), from the shape and
// the switches alone: aligned caches of capacity S_max assumed.  Returns false for a shape the call refuses.
static bool layer_decode_rows_route(const nsa_layer_desc *L, int B, int S, int S_max, int t0, int S_sel, int *launches, int *route) {
    if (check_layer(L, "layer_decode_rows_plan")) return false;
    if (B < 1 || S < 1 || S > LAYER_ROWS_MAX_S || t0 < 0 || (int64_t)t0 + S > S_max || S_sel < 1 || (int64_t)S_sel * L->l_sel < (int64_t)t0 + S) return false;
    const nsa_kv_desc kv = stand_in_kv(B, S_max, std::max(1, ncmp_of(S_max, L->l, L->d)));
    const CacheStrides C(L, &kv);
    const int n0 = ncmp_of(t0, L->l, L->d), n1 = ncmp_of(t0 + S, L->l, L->d);
    int n = 1 + (n1 > n0 ? 1 : 0);  // projection + RoPE + append, pooling
    SelDecodeCall c = sel_decode_call(L, &kv, C, S, t0, n1, S_sel);
    c.Q = kv.K_sel;
    const bool one = decode_rows_supported(c);
    if (one) {
        n += 1;
    } else {
        int nl = 3, form = -1;  // (the selected branch's own estimate of its separate launches)
        if (nsa_sel_decode_rows_plan(B, S, L->G, L->h, L->Dk, L->Dv, n1, S_sel, t0 + S, L->n_sel, L->dtype, &nl, &form) != NSA_OK || nl < 2) nl = 3;
        n += nl;
    }
    n += band_pair_splits(L, &kv, C, S, t0, t0 + S, n1) ? 1 : 2;  // (an undeferred split branch adds its combine: not counted)
    n += 2;  // finish (or gate + mix), output projection
    *launches = n;
    *route = one ? 1 : 0;
    return true;
}

// The measured rule behind LAYER_DECODE_ROWS = -1 (tools/bench_layer_decode_rows.py): S = 1 stays with the single step, whose
// band branches ride on the selected branch's launch (three launches against five here)
static bool layer_decode_rows_measured_ok(int B, int S, int t0) { return S >= 2; }

size_t nsa_layer_decode_rows_workspace(const nsa_layer_desc *L, int B, int S, int S_max) {
    if (!L || !dtype_ok(L->dtype) || B < 1 || S < 1 || S > LAYER_ROWS_MAX_S || S_max < 1) return 0;
    return decode_ws(L, B, S_max, S).total;
}

int nsa_layer_decode_rows(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *x, void *y, int t0, int S, const int32_t *csc_ptr,
                          const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out, void *workspace,
                          size_t workspace_bytes, void *stream) {
    LayerDecode D;
    if (int rc = layer_decode_begin("layer_decode_rows", L, kv, x, y, t0, S, true, S_sel, workspace, workspace_bytes, &D)) return rc;
    NSA_CHECK_ARG(D.n1 <= kv->n_cmp_max, "layer_decode_rows: compressed cache too small");
    // 1. fused QKV projection of the B S rows, each rotated and appended at its own position t0 + s
    if (int rc = launch_qkv_rope_append(rope_append_params(L, kv, D.ws + D.W.proj, D.Q, S, t0), qkv_call(L, x, kv->B * S, nullptr, 0.f, stream), true))
        return rc;
    // 2. the compressed tokens whose windows complete inside the call
    if (D.n1 > D.n0)
        if (int rc = nsa_cmp_pool_append(L, kv, D.n0, D.n1, stream)) return rc;
    const CacheStrides C(L, kv);
    // 3. selected branch: every row's scores -> top-n at its token -> attention over K_sel[:t + 1] (one launch, or the separate launches)
    if (int rc = sel_decode_rows_impl(layer_sel_call(D, C, csc_ptr, csc_rows, csc_vals, S_sel, ranges_out), D.ws + D.W.sel, D.W.sel_bytes, stream)) return rc;
    // 4. sliding and compressed branches of the S rows: one launch in split form with the combine left to the finish kernel, else one each;
    // 5. split combine + gates + mix, 6. output projection of the B S rows (no residual, no folded norm: the block step alone has them)
    return layer_decode_rows_tail(D, C, gates_out, y, stream);
}

int nsa_layer_decode_rows_plan(const nsa_layer_desc *L, int B, int S, int S_max, int t0, int S_sel, int *launches, int *route) {
    NSA_CHECK_ARG(launches && route, "layer_decode_rows_plan: null pointer");
    *launches = 0;
    *route = -1;
    int n = 0, r = -1;
    NSA_CHECK_ARG(layer_decode_rows_route(L, B, S, S_max, t0, S_sel, &n, &r), "layer_decode_rows_plan: a shape nsa_layer_decode_rows refuses");
    const int sw = tuning(TUNE_LAYER_DECODE_ROWS);
    if (sw == 0 || (sw < 0 && !layer_decode_rows_measured_ok(B, S, t0))) return NSA_OK;  // declined: S single steps
    *launches = n;
    *route = r;
    return NSA_OK;
}

// ------------------------------------------------------------------------------ ragged-batch layer decode: per-sequence positions
// What the call and its plan share, from the shape, the host bound and the switches alone (aligned caches of capacity S_max assumed; the
// position array is never read on the host).  NSA_OK with p->launches = n: the call runs; p->launches = 0 and p->why = the limit: DECLINED --
// there is no scalar route to stand in (every other launch of the layer takes one position per call); an error status: bad arguments.
static int layer_decode_ragged_route(const char *who, const nsa_layer_desc *L, int B, int S, int S_max, int t_max, int S_sel, int n_cmp_max,
                                     PositionsPlan *p) {
    *p = PositionsPlan{};
    if (int rc = check_layer(L, who)) return rc;
    if (int rc = check_rows_count(who, S)) return rc;
    NSA_CHECK_ARG(B >= 1 && S_max >= 1, "%s: bad cache sizes", who);
    if (int rc = check_bound(who, L, S, S_max, t_max, S_sel, p)) return rc;
    NSA_CHECK_ARG(n_cmp_max < 0 || n_cmp_max >= p->n1, "%s: compressed cache too small (n_cmp_max=%d) for %d tokens", who, n_cmp_max, p->te + 1);
    p->why = !dtype_16bit(L->dtype)          ? "bf16 / f16 only (the launches that take per-sequence positions have no fp32 form)"
             : !default_decode_geometry(L) ? "Dk = Dv in {64, 128} and the default block geometry only (l = 32, d = 16, l' = 64)" : nullptr;
    if (p->why) return NSA_OK;
    const nsa_kv_desc kv = stand_in_kv(B, S_max, std::max(1, ncmp_of(S_max, L->l, L->d)));
    const CacheStrides C(L, &kv);
    SelDecodeCall sc = sel_decode_call(L, &kv, C, S, p->t0, p->n1, S_sel);
    sc.S_kv = p->te + 1;
    if (!decode_ragged_shape_plan(sc, p->te, nullptr, nullptr, &p->why)) return NSA_OK;
    p->why = nullptr;
    // projection + RoPE + append, pooling (always: the host cannot know whether a window completes), the selected branch's one launch,
    // the band pair (or one launch each; an undeferred split branch adds its combine: not counted), finish (or gate + mix), output projection
    p->launches = 3 + (band_pair_splits(L, &kv, C, S, p->t0, p->te + 1, p->n1) ? 1 : 2) + 2;
    return NSA_OK;
}

size_t nsa_layer_decode_ragged_workspace(const nsa_layer_desc *L, int B, int S, int S_max) { return nsa_layer_decode_rows_workspace(L, B, S, S_max); }

int nsa_layer_decode_ragged_plan(const nsa_layer_desc *L, int B, int S, int S_max, int t_max, int S_sel, int *launches, int *route) {
    NSA_CHECK_ARG(launches && route, "layer_decode_ragged_plan: null pointer");
    PositionsPlan p;
    return plan_answer(layer_decode_ragged_route("layer_decode_ragged_plan", L, B, S, S_max, t_max, S_sel, -1, &p), p, launches, route);
}

int nsa_layer_decode_ragged(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *x, void *y, const int32_t *t_pos, int t_max, int S,
                            const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out,
                            void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "layer_decode_ragged";
    if (int rc = check_layer(L, who)) return rc;
    if (int rc = check_kv(kv, who)) return rc;
    if (int rc = check_io(who, L, x, y, t_pos)) return rc;
    PositionsPlan p;  // the largest sequence the launches are planned for: te + 1 tokens after the call, n1 compressed ones (LayerDecode)
    if (int rc = layer_decode_ragged_route(who, L, kv->B, S, kv->S_max, t_max, S_sel, kv->n_cmp_max, &p)) return rc;
    NSA_CHECK_ARG(!p.why, "%s: %s (B = %d, S = %d, D = %d, t_max = %d)", who, p.why, kv->B, S, L->Dk, t_max);
    const CacheStrides C(L, kv);
    SelDecodeCall probe = sel_decode_call(L, kv, C, S, 0, p.n1, S_sel);
    probe.S_kv = p.te + 1;
    probe.Q = probe.O = kv->K_cmp;  // (Q and O come from the 256-byte aligned workspace)
    NSA_CHECK_ARG(decode_step_operands_ok(probe) && (uintptr_t)kv->K_cmp % 16 == 0,
                  "%s: K_cmp, K_sel and V_sel must be 16-byte aligned with strides in multiples of 8 elements", who);
    const DecodeWs W = decode_ws(L, kv->B, kv->S_max, S);
    if (int rc = check_workspace(who, workspace, workspace_bytes, W.total)) return rc;
    const LayerDecode D = layer_decode_positions(L, kv, W, workspace, S, p, t_pos);
    hipStream_t st = (hipStream_t)stream;
    // 1. fused QKV projection of the B S rows, row (b, s) rotated at t_pos[b] + s and appended there where sequence b is live
    RopeAppendParams R = rope_append_params(L, kv, D.ws + W.proj, D.Q, S, 0);
    R.t_pos = t_pos;
    R.t_max = p.te;
    if (int rc = launch_qkv_rope_append(R, qkv_call(L, x, kv->B * S, nullptr, 0.f, stream), true)) return rc;
    // 2. every live sequence's compressed tokens whose windows complete inside its rows (launched every call: its blocks exit where none does)
    CmpPoolParams P = cmp_pool_params(L, kv->B, kv->K_raw, kv->V_raw, kv->K_cmp, kv->V_cmp, kv->S_max, kv->n_cmp_max);
    P.t_pos = t_pos; P.t_max = p.te; P.S = S; P.G = L->G;
    if (int rc = launch_cmp_pool_ragged(P, L->dtype, st)) return rc;
    // 3. selected branch: the rows form with the position array (one launch; zero O and ranges rows for a sequence that is not live)
    SelDecodeCall c = layer_sel_call(D, C, csc_ptr, csc_rows, csc_vals, S_sel, ranges_out);
    c.S_kv = p.te + 1;  // (the paged call leaves t0 + S)
    if (int rc = launch_decode_rows(c, st, t_pos, p.te)) return rc;
    // 4. both band branches in one dual launch (split form, deferred combine; Dv = 128: one ragged launch each), 5. finish (or the gate
    // kernel), 6. output projection -- the rows call's tail with the position array in D
    return layer_decode_rows_tail(D, C, gates_out, y, stream);
}

// ------------------------------------------------------------------------------ paged layer decode: append, pool and attend through a block table
// The pools under a nsa_kv_desc whose extent is ONE page (S_max = 1024, n_cmp_max = 64): CacheStrides then gives the page and group strides
// of the pools, and every block that is filled from a nsa_kv_desc (the branches' calls, the selected branch's block) names the pools.
static nsa_kv_desc page_extent_kv(const nsa_paged_kv_desc *p) {
    nsa_kv_desc kv{};
    kv.K_sel = p->K_sel; kv.V_sel = p->V_sel; kv.K_win = p->K_win; kv.V_win = p->V_win; kv.K_raw = p->K_raw; kv.V_raw = p->V_raw;
    kv.K_cmp = p->K_cmp; kv.V_cmp = p->V_cmp;
    kv.B = p->B; kv.S_max = LAYER_PAGE_TOKENS; kv.n_cmp_max = LAYER_PAGE_CMP;
    return kv;
}
constexpr int LAYER_PAGED_MAX_PAGES = 1 << 20;  // (the paged operators' bound: the capacity max_pages * 1024 stays a positive int)
// the workspace is the ragged call's for the longest context a live row can sit in -- the long-row form of the selected branch ends at 128 chunks of 64
// compressed tokens, te = 2^17 - 1 -- plus the verdicts t_live [B]; it does not grow with max_pages
static int paged_ws_tokens(int max_pages) { return (int)std::min<int64_t>((int64_t)max_pages * LAYER_PAGE_TOKENS, 1 << 17); }

// What the call and its plan share, from the shape, the host bound and the switches alone (aligned pools assumed; neither the positions nor
// the table are read on the host).  Answers as layer_decode_ragged_route does (declined: there is no fallback).
static int layer_decode_paged_route(const char *who, const nsa_layer_desc *L, int B, int S, int max_pages, int t_max, int S_sel, PositionsPlan *p) {
    *p = PositionsPlan{};
    if (int rc = check_layer(L, who)) return rc;
    if (int rc = check_rows_count(who, S)) return rc;
    NSA_CHECK_ARG(B >= 1, "%s: bad batch size %d", who, B);
    NSA_CHECK_ARG(max_pages >= 1 && max_pages <= LAYER_PAGED_MAX_PAGES, "%s: max_pages = %d, must be in [1, 2^20]", who, max_pages);
    const int cap = max_pages * LAYER_PAGE_TOKENS;
    if (int rc = check_bound(who, L, S, cap, t_max, S_sel, p)) return rc;
    p->why = !dtype_16bit(L->dtype) ? "bf16 / f16 only (no kernel reads or writes pools of pages in fp32)"
             : !default_decode_geometry(L)
                 ? "Dk = Dv in {64, 128} and the default block geometry only (l = 32, d = 16, l' = 64: pages of 1024 tokens and 64 compressed rows)"
                 : L->w < 1 ? "the sliding window must hold at least one key (w >= 1)" : nullptr;
    if (p->why) return NSA_OK;
    const nsa_kv_desc kv = stand_in_kv(B, LAYER_PAGE_TOKENS, LAYER_PAGE_CMP);  // (aligned pools under their page extent: page_extent_kv)
    const CacheStrides C(L, &kv);
    SelDecodeCall sc = sel_decode_call(L, &kv, C, S, 0, p->n1, S_sel);
    sc.S_kv = cap;
    if (!decode_paged_shape_plan(sc, p->te, nullptr, nullptr, &p->why)) return NSA_OK;
    p->why = nullptr;
    int ns = 1;
    band_attn_workspace(B, S, L->G, L->h, L->Dk, L->Dv, L->dtype, &ns);
    // the verdicts, projection + RoPE + append, pooling (always), the selected branch's one launch, the sliding and the compressed branch (each
    // one paged launch, with its combine behind it in split form), finish (or gate + mix), output projection
    p->launches = 4 + 2 * (ns > 1 ? 2 : 1) + 2;
    return NSA_OK;
}

size_t nsa_layer_decode_paged_workspace(const nsa_layer_desc *L, int B, int S, int max_pages) {
    if (!L || !dtype_ok(L->dtype) || B < 1 || S < 1 || S > LAYER_ROWS_MAX_S || max_pages < 1 || max_pages > LAYER_PAGED_MAX_PAGES) return 0;
    return decode_ws(L, B, paged_ws_tokens(max_pages), S).total + up256(sizeof(int32_t) * (size_t)B);
}

int nsa_layer_decode_paged_plan(const nsa_layer_desc *L, int B, int S, int max_pages, int t_max, int S_sel, int *launches, int *route) {
    NSA_CHECK_ARG(launches && route, "layer_decode_paged_plan: null pointer");
    PositionsPlan p;
    return plan_answer(layer_decode_paged_route("layer_decode_paged_plan", L, B, S, max_pages, t_max, S_sel, &p), p, launches, route);
}

int nsa_layer_decode_paged(const nsa_layer_desc *L, const nsa_paged_kv_desc *pkv, const void *x, void *y, const int32_t *t_pos, int t_max, int S,
                           const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out,
                           void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "layer_decode_paged";
    if (int rc = check_layer(L, who)) return rc;
    NSA_CHECK_ARG(pkv && pkv->K_sel && pkv->V_sel && pkv->K_win && pkv->V_win && pkv->K_raw && pkv->V_raw && pkv->K_cmp && pkv->V_cmp, "%s: null pool pointer", who);
    NSA_CHECK_ARG(pkv->B >= 1 && pkv->n_pages >= 1, "%s: bad pool sizes (B = %d, n_pages = %d)", who, pkv->B, pkv->n_pages);
    if (int rc = check_io(who, L, x, y, t_pos)) return rc;
    NSA_CHECK_ARG(pkv->block_table, "%s: null block table", who);
    PositionsPlan p;  // the largest sequence the launches are planned for: te + 1 tokens after the call, n1 compressed ones (LayerDecode)
    if (int rc = layer_decode_paged_route(who, L, pkv->B, S, pkv->max_pages, t_max, S_sel, &p)) return rc;
    NSA_CHECK_ARG((uintptr_t)pkv->block_table % 4 == 0 && pkv->table_stride >= pkv->max_pages,
                  "%s: the block table must be 4-byte aligned with a row stride of at least max_pages = %d (got %lld)", who, pkv->max_pages,
                  (long long)pkv->table_stride);
    NSA_CHECK_ARG(!p.why, "%s: %s (B = %d, S = %d, D = %d, t_max = %d)", who, p.why, pkv->B, S, L->Dk, t_max);
    NSA_CHECK_ARG(((uintptr_t)pkv->K_sel | (uintptr_t)pkv->V_sel | (uintptr_t)pkv->K_win | (uintptr_t)pkv->V_win | (uintptr_t)pkv->K_raw | (uintptr_t)pkv->V_raw |
                   (uintptr_t)pkv->K_cmp | (uintptr_t)pkv->V_cmp) % 16 == 0,
                  "%s: the eight pools must be 16-byte aligned", who);
    const int B = pkv->B, cap = pkv->max_pages * LAYER_PAGE_TOKENS;
    const nsa_kv_desc kv = page_extent_kv(pkv);
    const CacheStrides C(L, &kv);
    const DecodeWs W = decode_ws(L, B, paged_ws_tokens(pkv->max_pages), S);
    if (int rc = check_workspace(who, workspace, workspace_bytes, W.total + up256(sizeof(int32_t) * (size_t)B))) return rc;
    int32_t *t_live = (int32_t *)((unsigned char *)workspace + W.total);
    const LayerPageTable pg{pkv->block_table, pkv->table_stride, pkv->n_pages, pkv->max_pages};
    // every launch behind the pre-pass takes t_live as its position array: one verdict per sequence for the writers and the readers
    const LayerDecode D = layer_decode_positions(L, &kv, W, workspace, S, p, t_live, &pg);
    hipStream_t st = (hipStream_t)stream;
    // 0. the verdicts: t_live[b] = t_pos[b] where sequence b is live (positions, and every table entry it needs inside [0, n_pages)), else -1
    if (int rc = launch_paged_live(PagedLiveParams{t_pos, t_live, pg, B, S, p.te}, st)) return rc;
    // 1. fused QKV projection of the B S rows, row (b, s) rotated at pos = t_live[b] + s and appended to row pos & 1023 of page
    // table[b][pos >> 10] of the six token pools where sequence b is live
    RopePagedParams R{};
    static_cast<RopeAppendParams &>(R) = rope_append_params(L, &kv, D.ws + W.proj, D.Q, S, 0);
    R.S_max = cap;
    R.t_pos = t_live;
    R.t_max = p.te;
    R.pg = pg;
    if (int rc = launch_qkv_rope_append_paged(R, qkv_call(L, x, B * S, nullptr, 0.f, stream))) return rc;
    // 2. every live sequence's compressed tokens whose windows complete inside its rows, each window row and the compressed row through its page
    CmpPoolPagedParams P{};
    static_cast<CmpPoolParams &>(P) = cmp_pool_params(L, B, pkv->K_raw, pkv->V_raw, pkv->K_cmp, pkv->V_cmp, cap, pkv->max_pages * LAYER_PAGE_CMP);
    P.t_pos = t_live; P.t_max = p.te; P.S = S; P.G = L->G;
    P.pg = pg;
    if (int rc = launch_cmp_pool_paged(P, L->dtype, st)) return rc;
    // 3. selected branch: the paged rows form (one launch; zero O and ranges rows for a sequence that is not live; S_kv stays t0 + S)
    const SelDecodeCall c = layer_sel_call(D, C, csc_ptr, csc_rows, csc_vals, S_sel, ranges_out);
    if (int rc = sel_decode_paged_impl(c, DecPageTable{pg.table, pg.stride, pg.n_pages}, pg.max_pages, LAYER_PAGE_TOKENS, t_live, p.te, stream)) return rc;
    // 4. the sliding and the compressed branch, one paged launch each with its own combine, 5. finish (or the gate kernel), 6. output projection
    return layer_decode_rows_tail(D, C, gates_out, y, stream);
}

// block workspace: xn | h | hn | u [B, mlp_hidden] | layer decode workspace
struct BlockWs {
    size_t xn, h, hn, u, layer, total, layer_bytes;
};
static BlockWs block_ws(const nsa_block_desc *Bk, int B, int S_max) {
    BlockWs w;
    const size_t e = esize(Bk->attn.dtype);
    size_t o = 0;
    w.xn = o; o += up256((size_t)B * Bk->attn.dim * e);
    w.h = o; o += up256((size_t)B * Bk->attn.dim * e);
    w.hn = o; o += up256((size_t)B * Bk->attn.dim * e);
    w.u = o; o += up256((size_t)B * Bk->mlp_hidden * e);
    w.layer_bytes = decode_ws(&Bk->attn, B, S_max).total;
    w.layer = o; o += up256(w.layer_bytes);
    w.total = o;
    return w;
}

size_t nsa_block_decode_step_workspace(const nsa_block_desc *Bk, int B, int S_max) {
    if (!Bk || !dtype_ok(Bk->attn.dtype) || B < 1 || S_max < 1 || Bk->mlp_hidden < 1) return 0;
    return block_ws(Bk, B, S_max).total;
}

int nsa_block_decode_step(const nsa_block_desc *Bk, const nsa_kv_desc *kv, const void *x, void *y, int t, const int32_t *csc_ptr,
                          const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out,
                          void *workspace, size_t workspace_bytes, void *stream) {
    NSA_CHECK_ARG(Bk, "block_decode_step: null descriptor");
    if (int rc = check_layer(&Bk->attn, "block_decode_step")) return rc;
    if (int rc = check_kv(kv, "block_decode_step")) return rc;
    NSA_CHECK_ARG(x && y && Bk->norm1_w && Bk->norm2_w && Bk->mlp_w1 && Bk->mlp_w2 && Bk->mlp_hidden >= 1, "block_decode_step: null pointer");
    const int B = kv->B, dim = Bk->attn.dim, dt = Bk->attn.dtype;
    const BlockWs W = block_ws(Bk, B, kv->S_max);
    if (int rc = check_workspace("block_decode_step", workspace, workspace_bytes, W.total)) return rc;
    unsigned char *ws = (unsigned char *)workspace;
    hipStream_t st = (hipStream_t)stream;
    void *xn = ws + W.xn, *h = ws + W.h, *hn = ws + W.hn, *u = ws + W.u;
    const float eps = Bk->norm_eps > 0.f ? Bk->norm_eps : 1e-6f;
    // small batches: both RMSNorms are folded into the projections that consume them (two launches fewer per block)
    const bool fold1 = proj_route(qkv_call(&Bk->attn, x, B, Bk->norm1_w, eps, stream), PROJ_ROPE).fold_norm;
    if (!fold1)
        if (int rc = launch_rmsnorm_rows(x, Bk->norm1_w, xn, B, dim, eps, dt, st)) return rc;
    // h = x + attn(norm1(x)): the residual rides in the output projection's epilogue
    if (int rc = layer_decode_step_impl(&Bk->attn, kv, fold1 ? x : xn, h, t, csc_ptr, csc_rows, csc_vals, S_sel, ranges_out, gates_out,
                                        ws + W.layer, W.layer_bytes, stream, x, fold1 ? Bk->norm1_w : nullptr, eps))
        return rc;
    if (int rc = launch_linear_normed(LinearCall{h, Bk->mlp_w1, u, B, Bk->mlp_hidden, dim, dt, 1, nullptr, st, Bk->norm2_w, eps}, hn)) return rc;  // silu(fc1)
    return launch_linear_small_epi(LinearCall{u, Bk->mlp_w2, y, B, dim, Bk->mlp_hidden, dt, 2, h, st});  // fc2 + h
}

// model workspace: x ping | x pong | block workspace
size_t nsa_model_decode_step_workspace(const nsa_block_desc *blocks, int n_blocks, int B, int S_max) {
    if (!blocks || n_blocks < 1 || B < 1 || S_max < 1) return 0;
    const size_t xb = up256((size_t)B * blocks[0].attn.dim * esize(blocks[0].attn.dtype));
    size_t bw = 0;
    for (int i = 0; i < n_blocks; ++i) {
        const size_t w = nsa_block_decode_step_workspace(&blocks[i], B, S_max);
        if (w == 0) return 0;
        if (w > bw) bw = w;
    }
    return 2 * xb + up256(bw) + up256((size_t)B * 64 * 8);  // + argmax partials (up to 64 chunks of 4096 logits)
}

int nsa_model_decode_step(const nsa_block_desc *blocks, const nsa_kv_desc *kvs, int n_blocks, const int32_t *tokens, const void *embed,
                          const void *norm_f_w, const void *lm_head, int vocab, void *logits, int32_t *next_tokens, int t,
                          const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, void *workspace,
                          size_t workspace_bytes, void *stream) {
    NSA_CHECK_ARG(blocks && kvs && n_blocks >= 1 && tokens && embed && norm_f_w && lm_head && logits && vocab >= 1, "model_decode_step: null pointer");
    const int B = kvs[0].B, dim = blocks[0].attn.dim, dt = blocks[0].attn.dtype;
    for (int i = 0; i < n_blocks; ++i)
        NSA_CHECK_ARG(kvs[i].B == B && blocks[i].attn.dim == dim && blocks[i].attn.dtype == dt && kvs[i].S_max == kvs[0].S_max,
                      "model_decode_step: blocks / caches disagree on batch, width, dtype or capacity");
    const size_t need = nsa_model_decode_step_workspace(blocks, n_blocks, B, kvs[0].S_max);
    NSA_CHECK_ARG(need > 0 && workspace && ((uintptr_t)workspace % 256 == 0) && workspace_bytes >= need,
                  "model_decode_step: workspace missing, misaligned or too small");  // need = 0: a block the workspace query refuses
    hipStream_t st = (hipStream_t)stream;
    const size_t xb = up256((size_t)B * dim * esize(dt));
    unsigned char *ws = (unsigned char *)workspace;
    void *xa = ws, *xc = ws + xb;
    unsigned char *bws = ws + 2 * xb;
    if (int rc = launch_embed_rows(tokens, embed, xa, B, dim, vocab, dt, st)) return rc;
    for (int i = 0; i < n_blocks; ++i) {
        if (int rc = nsa_block_decode_step(&blocks[i], &kvs[i], xa, xc, t, csc_ptr, csc_rows, csc_vals, S_sel, nullptr, nullptr, bws,
                                           workspace_bytes - 2 * xb, stream))
            return rc;
        void *tmp = xa;
        xa = xc;
        xc = tmp;
    }
    const float eps = blocks[0].norm_eps > 0.f ? blocks[0].norm_eps : 1e-6f;
    if (int rc = launch_linear_normed(LinearCall{xa, lm_head, logits, B, vocab, dim, dt, 0, nullptr, st, norm_f_w, eps}, xc)) return rc;
    if (next_tokens) {
        NSA_CHECK_ARG(argmax_rows_workspace(B, vocab) <= (size_t)B * 64 * 8, "model_decode_step: vocabulary too large for the in-call argmax");
        return launch_argmax_rows(logits, next_tokens, B, vocab, dt, ws + need - up256((size_t)B * 64 * 8), st);
    }
    return NSA_OK;
}

}  // extern "C"
