// Host-only helpers of the C ABI's dispatch layer (nsa_api.hip, nsa_layer_api.hip): the predicates, defaults and argument-block fills
// that every entry point shares.  One of each; a call site keeps its own extra conditions next to the call.
#pragma once
#include <climits>
#include <cmath>

#include "nsa_common.hpp"
#include "layer_fused.hpp"
#include "sel_attn_params.hpp"
#include "sel_scores_params.hpp"

namespace nsa {

inline bool dtype_ok(int dt) { return dt == NSA_DT_F32 || dt == NSA_DT_BF16 || dt == NSA_DT_F16; }
inline size_t esize(int dt) { return dt == NSA_DT_F32 ? 4 : 2; }
inline float default_scale(float scale, int Dk) { return scale > 0.f ? scale : 1.0f / sqrtf((float)Dk); }

// compressed tokens of a context of S tokens: what its last position S - 1 sees on the emission schedule (ncmp_at), (S - l) / d + 1 from S = l on
inline int ncmp_of(int S, int l, int d) { return ncmp_at(S - 1, l, d, INT_MAX); }

// "<who>: workspace missing, misaligned or too small" unless `need` bytes at a 256-byte boundary are there
inline int check_workspace(const char *who, const void *ws, size_t bytes, size_t need) {
    NSA_CHECK_ARG(ws && ((uintptr_t)ws % 256 == 0) && bytes >= need, "%s: workspace missing, misaligned or too small", who);
    return NSA_OK;
}

// what the MFMA scorer kernels ask of their operands: every K_cmp stride a multiple of 8 elements, Q and K_cmp 16-byte aligned
inline bool kcmp_aligned(const void *Q, const void *Kc, int64_t csb, int64_t csg, int64_t css) {
    return csb % 8 == 0 && csg % 8 == 0 && css % 8 == 0 && ((uintptr_t)Q % 16 == 0) && ((uintptr_t)Kc % 16 == 0);
}

// O [R,h,Dv] = 0: the output of rows that select nothing (attention_kernels.py:718-719)
inline int zero_rows(void *O, int64_t R, int h, int Dv, int dtype, hipStream_t st) {
    const size_t esz = esize(dtype);
    NSA_HIP_TRY(hipMemsetAsync(O, 0, (size_t)R * h * Dv * esz, st));
    return NSA_OK;
}

// element strides of a layer's caches ([B,G,S_max,D] and [B,G,n_cmp_max,D], rows contiguous) and the softmax scale
struct CacheStrides {
    int64_t ksb, ksg, vsb, vsg;  // K_sel / K_win / K_raw and their V
    int64_t kcb, kcg, vcb, vcg;  // K_cmp / V_cmp
    float scale;
    CacheStrides(const nsa_layer_desc *L, const nsa_kv_desc *kv)
        : ksb((int64_t)L->G * kv->S_max * L->Dk), ksg((int64_t)kv->S_max * L->Dk), vsb((int64_t)L->G * kv->S_max * L->Dv),
          vsg((int64_t)kv->S_max * L->Dv), kcb((int64_t)L->G * kv->n_cmp_max * L->Dk), kcg((int64_t)kv->n_cmp_max * L->Dk),
          vcb((int64_t)L->G * kv->n_cmp_max * L->Dv), vcg((int64_t)kv->n_cmp_max * L->Dv), scale(1.0f / sqrtf((float)L->Dk)) {}
};

// What the selected-branch decode family (nsa_sel_decode_step / nsa_sel_decode_rows and everything below them) passes around: the arguments
// of the C ABI, once.  S consecutive tokens per sequence at t0 .. t0 + S - 1; the single step is S = 1 with t0 = its token.
struct SelDecodeCall {
    const void *Q, *K_cmp, *K, *V;
    const int32_t *csc_ptr, *csc_rows;
    const float *csc_vals;
    int32_t *ranges_out;
    void *O;
    int B, S, G, h, Dk, Dv, S_cmp, S_sel, S_kv;
    int l, d, l_sel, n_top, t0;
    int64_t kcb, kcg, kcs, ksb, ksg, kss, vsb, vsg, vss;
    int dtype;
    float scale;
    int64_t rows() const { return (int64_t)B * S * G; }
};
// the layer calls' block: rows t0 .. t0 + S - 1 over the caches kv, which then hold t0 + S tokens and n_cmp compressed ones; the caller adds
// what the caches do not hold (Q, the CSC arrays, ranges_out, O)
inline SelDecodeCall sel_decode_call(const nsa_layer_desc *L, const nsa_kv_desc *kv, const CacheStrides &C, int S, int t0, int n_cmp, int S_sel) {
    SelDecodeCall c{};
    c.K_cmp = kv->K_cmp; c.K = kv->K_sel; c.V = kv->V_sel;
    c.B = kv->B; c.S = S; c.G = L->G; c.h = L->h; c.Dk = L->Dk; c.Dv = L->Dv; c.S_cmp = n_cmp; c.S_sel = S_sel; c.S_kv = t0 + S;
    c.l = L->l; c.d = L->d; c.l_sel = L->l_sel; c.n_top = L->n_sel; c.t0 = t0;
    c.kcb = C.kcb; c.kcg = C.kcg; c.kcs = L->Dk; c.ksb = C.ksb; c.ksg = C.ksg; c.kss = L->Dk; c.vsb = C.vsb; c.vsg = C.vsg; c.vss = L->Dv;
    c.dtype = L->dtype; c.scale = C.scale;
    return c;
}

// the public plan queries' block: no tensors, default block geometry, the S rows at the end of a cache of S_kv tokens
inline SelDecodeCall sel_decode_plan_call(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int n_top, int dtype) {
    SelDecodeCall c{};
    c.B = B; c.S = S; c.G = G; c.h = h; c.Dk = Dk; c.Dv = Dv; c.S_cmp = S_cmp; c.S_sel = S_sel; c.S_kv = S_kv; c.n_top = n_top; c.dtype = dtype;
    c.l = 32; c.d = 16; c.l_sel = 64; c.t0 = S_kv - S;
    return c;
}

// What the scorer family (nsa_sel_scores* / nsa_pcmp_all and every launcher below them) passes around: the arguments of the C ABI, once.
// Rows (b, s, g) at tokens q0 + s; norm = 1: a row normalises over the n_cmp(q0 + s) columns a decode step at its token sees.
struct ScoresCall {
    const void *Q, *K_cmp;
    float *p_grp;
    const int32_t *csc_ptr, *csc_rows;
    const float *csc_vals;
    int B, S, G, h, Dk, S_cmp, S_sel;
    int64_t csb, csg, css;
    int l, d, l_sel, causal_skip, dtype;
    float scale;
    int q0, norm;
    void *ws;  // the route's scratch (nsa_sel_scores_rows_workspace); nsa_pcmp_all: p_cmp itself
    size_t ws_bytes;
    hipStream_t st;
    int64_t rows() const { return (int64_t)B * S * G; }
};
// the shape alone (workspace and plan queries: no tensors, the route of variant 0 is what they ask)
inline ScoresCall scores_shape_call(int B, int S, int G, int h, int Dk, int S_cmp, int S_sel, int l, int d, int l_sel, int dtype, int norm) {
    ScoresCall c{};
    c.B = B; c.S = S; c.G = G; c.h = h; c.Dk = Dk; c.S_cmp = S_cmp; c.S_sel = S_sel; c.l = l; c.d = d; c.l_sel = l_sel; c.dtype = dtype; c.norm = norm;
    return c;
}
// the scorer's block of a decode-family call: norm = 1 scores its S rows at their own tokens t0 + s, norm = 0 over all S_cmp columns
inline ScoresCall scores_call(const SelDecodeCall &c, float *p_grp, int causal_skip, int norm, void *ws, size_t ws_bytes, void *stream) {
    return ScoresCall{c.Q, c.K_cmp, p_grp, c.csc_ptr, c.csc_rows, c.csc_vals, c.B, c.S, c.G, c.h, c.Dk, c.S_cmp, c.S_sel, c.kcb, c.kcg, c.kcs, c.l, c.d, c.l_sel,
                      causal_skip, c.dtype, c.scale, norm ? c.t0 : 0, norm, ws, ws_bytes, (hipStream_t)stream};
}

// The top-n selection of a call's rows: row (b, s, g) selects at token t0 + s (or t_rows[row]) into ranges_out [R, out_width, 2].
struct SelectCall {
    int t0;
    const int32_t *t_rows;
    int n_top, force_init, force_local, mode, S_total;
    int32_t *ranges_out;
    int out_width;
};
// a decode step's selection: sequential, block 0 and the two newest blocks forced, n_top ranges per row
inline SelectCall decode_select_call(const SelDecodeCall &c) { return SelectCall{c.t0, nullptr, c.n_top, 1, 2, NSA_SEL_SEQUENTIAL, c.S, c.ranges_out, c.n_top}; }

// RoPE + append of S tokens at position t0 of the caches kv (the backward passes the gradients in the caches' places)
inline RopeAppendParams rope_append_params(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *proj, void *Q_out, int S, int t0) {
    RopeAppendParams P{};
    P.proj = proj;
    P.Q_out = Q_out;
    P.cache[0] = kv->K_sel; P.cache[1] = kv->V_sel; P.cache[2] = kv->K_win; P.cache[3] = kv->V_win; P.cache[4] = kv->K_raw; P.cache[5] = kv->V_raw;
    P.B = kv->B; P.S = S; P.G = L->G; P.h = L->h; P.Dk = L->Dk; P.Dv = L->Dv; P.S_max = kv->S_max; P.t0 = t0;
    P.rope_base = L->rope_base > 0.f ? L->rope_base : 10000.0f;
    P.inv_scale = 1.0f / (L->rope_scale > 0.f ? L->rope_scale : 1.0f);
    return P;
}

// pooling of the compressed tokens of B sequences: raw caches [B G, S_max, D] -> compressed caches [B G, n_cmp_max, D] (the backward passes
// no caches: its gradients go beside the block).  The caller adds the tokens: j0 / j1, or the position array of the ragged forms
inline CmpPoolParams cmp_pool_params(const nsa_layer_desc *L, int B, const void *K_raw, const void *V_raw, void *K_cmp, void *V_cmp, int S_max, int n_cmp_max) {
    CmpPoolParams P{};
    P.K_raw = K_raw; P.V_raw = V_raw; P.K_cmp = K_cmp; P.V_cmp = V_cmp;
    P.nbg = B * L->G; P.S_max = S_max; P.n_cmp_max = n_cmp_max; P.Dk = L->Dk; P.Dv = L->Dv; P.l = L->l; P.d = L->d;
    P.rope_base = L->rope_base > 0.f ? L->rope_base : 10000.0f;
    P.inv_scale = 1.0f;  // the reference pools apply_rope(K_raw, pos) WITHOUT the NSA_ROPE_SCALE position scaling (compress_pool.py:20)
    return P;
}

// columns of the fused QKV projection: Q | K_sel | V_sel | K_win | V_win | K_raw | V_raw
inline int qkv_cols(const nsa_layer_desc *L) { return L->G * L->h * L->Dk + 3 * L->G * L->Dk + 3 * L->G * L->Dv; }
// that projection of `rows` rows of x as the projection family's block (no out: the launch's RopeAppendParams say where each column goes).
// The block step reads fold_norm from this call's route and the launcher decides on the same call: the two cannot disagree
inline LinearCall qkv_call(const nsa_layer_desc *L, const void *x, int rows, const void *norm_w, float eps, void *stream) {
    return LinearCall{x, L->W_qkv, nullptr, rows, qkv_cols(L), L->dim, L->dtype, 0, nullptr, (hipStream_t)stream, norm_w, eps};
}

// What the attention family (nsa_sel_attn_* / nsa_band_attn_* / nsa_sel_select_attn_fwd and everything below them) passes around: the
// arguments of the C ABI, once.  ranges / n: selection attention only; ws: the call's scratch (split-KV or key-split records)
struct AttnCall {
    const void *Q, *K, *V;
    const int32_t *ranges;
    void *O;
    float *lse;
    int B, S, G, h, Dk, Dv, S_kv, n;
    int64_t ksb, ksg, kss, vsb, vsg, vss;
    int dtype;
    float scale;
    int variant;
    void *ws;
    size_t ws_bytes;
    hipStream_t st;
    int64_t rows() const { return (int64_t)B * S * G; }
};
// the band of a band-attention call (BandAttnParams): the sliding window of w tokens, and the compressed tokens on their emission schedule
struct Band {
    int t0, a, dd, c, w;
};
inline Band sliding_band(int t0, int w) { return Band{t0, 0, 1, 0, w}; }
inline Band compressed_band(int t0, int l, int d) { return Band{t0, l, d, 1, 1 << 30}; }
struct AttnGrads {
    const void *dO;
    void *dQ;
    float *dK, *dV;
};
// the branches of a layer call over the S rows of Q (variant 0, no lse; ws: the branch's scratch): selected, sliding, compressed
inline AttnCall selected_call(const nsa_layer_desc *L, const nsa_kv_desc *kv, const CacheStrides &C, const void *Q, const int32_t *ranges, void *O, int S,
                              int S_kv, int n, void *ws, size_t ws_bytes, void *stream) {
    return AttnCall{Q, kv->K_sel, kv->V_sel, ranges, O, nullptr, kv->B, S, L->G, L->h, L->Dk, L->Dv, S_kv, n, C.ksb, C.ksg, L->Dk, C.vsb, C.vsg, L->Dv,
                    L->dtype, C.scale, 0, ws, ws_bytes, (hipStream_t)stream};
}
inline AttnCall sliding_call(const nsa_layer_desc *L, const nsa_kv_desc *kv, const CacheStrides &C, const void *Q, void *O, int S, int S_kv, void *ws,
                             size_t ws_bytes, void *stream) {
    return AttnCall{Q, kv->K_win, kv->V_win, nullptr, O, nullptr, kv->B, S, L->G, L->h, L->Dk, L->Dv, S_kv, 0, C.ksb, C.ksg, L->Dk, C.vsb, C.vsg, L->Dv,
                    L->dtype, C.scale, 0, ws, ws_bytes, (hipStream_t)stream};
}
inline AttnCall compressed_call(const nsa_layer_desc *L, const nsa_kv_desc *kv, const CacheStrides &C, const void *Q, void *O, int S, int n_cmp, void *ws,
                                size_t ws_bytes, void *stream) {
    return AttnCall{Q, kv->K_cmp, kv->V_cmp, nullptr, O, nullptr, kv->B, S, L->G, L->h, L->Dk, L->Dv, n_cmp, 0, C.kcb, C.kcg, L->Dk, C.vcb, C.vcg, L->Dv,
                    L->dtype, C.scale, 0, ws, ws_bytes, (hipStream_t)stream};
}
// the attention of a decode-family call's rows over the ranges it selected
inline AttnCall attn_call(const SelDecodeCall &c, void *ws, size_t ws_bytes, void *stream) {
    return AttnCall{c.Q, c.K, c.V, c.ranges_out, c.O, nullptr, c.B, c.S, c.G, c.h, c.Dk, c.Dv, c.S_kv, c.n_top, c.ksb, c.ksg, c.kss, c.vsb, c.vsg, c.vss,
                    c.dtype, c.scale, 0, ws, ws_bytes, (hipStream_t)stream};
}

// ---- the kernel blocks of a call.  What the three share (P: SelAttnParams, SelAttnBwdParams or BandAttnParams); everything a fill does not
// name (split-KV, mapping, fused selector) stays zero: the caller sets what its route needs
template <class P>
inline P attn_operands(const AttnCall &c) {
    P p{};
    p.Q = c.Q; p.K = c.K; p.V = c.V; p.O = c.O; p.lse = c.lse;
    p.S = c.S; p.G = c.G; p.h = c.h; p.Dk = c.Dk; p.Dv = c.Dv; p.S_kv = c.S_kv;
    p.ksb = c.ksb; p.ksg = c.ksg; p.kss = c.kss; p.vsb = c.vsb; p.vsg = c.vsg; p.vss = c.vss;
    p.scale = default_scale(c.scale, c.Dk);
    return p;
}
inline SelAttnParams sel_attn_params(const AttnCall &c) {
    SelAttnParams P = attn_operands<SelAttnParams>(c);
    P.ranges = c.ranges; P.R = c.rows(); P.n = c.n;
    return P;
}
inline SelAttnBwdParams sel_attn_bwd_params(const AttnCall &c, const AttnGrads &g) {
    SelAttnBwdParams P = attn_operands<SelAttnBwdParams>(c);
    P.ranges = c.ranges; P.R = c.rows(); P.n = c.n;
    P.dO = g.dO; P.dQ = g.dQ; P.dK = g.dK; P.dV = g.dV;
    return P;
}
inline BandAttnParams band_attn_params(const AttnCall &c, const Band &b) {
    BandAttnParams P = attn_operands<BandAttnParams>(c);
    P.B = c.B;
    P.t0 = b.t0; P.a = b.a; P.dd = b.dd; P.c = b.c; P.w = b.w;
    return P;
}

}  // namespace nsa
