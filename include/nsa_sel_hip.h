/*
 * nsa_sel_hip.h -- C ABI of libnsa_sel_hip.so: the MI355X (gfx950) implementation of
 * nsa-vibe's selected-branch attention hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only (no torch types).  Every
 * pointer is a DEVICE pointer unless its comment says "host".  All kernels are enqueued
 * on `stream` (a hipStream_t passed as void*; NULL = the default stream) and never
 * synchronise.  Inputs are borrowed and never written; outputs are caller allocated.
 *
 * Error convention (replaces the Python exceptions of the reference's plugin slot,
 * nsa/kernels/cuda_sel_kernel/__init__.py:60-68 and nsa/core/nsa_attention.py:764-782):
 * every entry point returns 0 on success, a negative NSA_ERR_* code otherwise, and
 * nsa_hip_last_error() returns a thread-local message.  The Python shim raises
 * RuntimeError on non-zero, which is what the reference's router catches.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   nsa_sel_attn_fwd           sel_forward(Q,K,V,ranges)            nsa/kernels/cuda_sel_kernel/sel_cuda.cpp:28-73
 *                              selection_attention_cuda             nsa/kernels/cuda_sel_kernel/__init__.py:47-68
 *                              grouped_selection_attention_masked   nsa/core/attention_kernels.py:705-772 (semantics)
 *   nsa_sel_attn_first_key_parity  grouped_selection_attention_packed / grouped_selection_attention (parity mode)
 *                                                                   nsa/core/attention_kernels.py:273-388, 181-226
 *   nsa_sel_attn_head_causal_parity  NSAAttention._sdpa_over_ranges (parity mode)   nsa/core/nsa_attention.py:1779-1855
 *   nsa_sel_attn_bwd           analytic backward / autograd of the masked SDPA
 *                                                                   nsa/kernels/triton_sel_kernel/__init__.py:125-231
 *   nsa_sel_scores             compute_pcmp_all + map_pcmp_to_pslc_batched + .sum(dim=3)
 *                                                                   nsa/core/selection_scorer.py:42-61, 89-116; nsa_attention.py:1073-1091
 *   nsa_pcmp_all               compute_pcmp_all                     nsa/core/selection_scorer.py:42-61
 *   nsa_map_pcmp_to_pgrp       map_pcmp_to_pslc_batched + group sum nsa/core/selection_scorer.py:89-121
 *   nsa_select_topn_ranges     select_topn_ranges / _batched (+v2)  nsa/core/selection_scorer.py:124-249, 255-362, 434-605
 *   nsa_indices_to_ranges_v2   convert_indices_to_ranges_batched_v2 nsa/core/selection_scorer.py:434-605
 *   nsa_batched_ranges_width   forced-column rule of the batched selector  selection_scorer.py:283-308,339-354
 *   nsa_build_block_meta_host  build_block_meta                     nsa/core/block_index.py:74-99
 */
#ifndef NSA_SEL_HIP_H
#define NSA_SEL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSA_HIP_ABI_VERSION 1

#if defined(__GNUC__)
#define NSA_API __attribute__((visibility("default")))
#else
#define NSA_API
#endif

/* element types of Q/K/V/O */
#define NSA_DT_F32 0
#define NSA_DT_BF16 1
#define NSA_DT_F16 2

/* selector semantics */
#define NSA_SEL_SEQUENTIAL 0 /* select_topn_ranges        (decode, sequential prefill) */
#define NSA_SEL_BATCHED 1    /* select_topn_ranges_batched (batched prefill, training)  */

/* error codes */
#define NSA_OK 0
#define NSA_ERR_INVALID (-1)     /* bad argument / unsupported shape */
#define NSA_ERR_HIP (-2)         /* a HIP runtime call failed        */
#define NSA_ERR_WORKSPACE (-3)   /* workspace too small              */
#define NSA_ERR_NO_DEVICE (-4)   /* no gfx950 device                 */

NSA_API int nsa_hip_abi_version(void);
NSA_API const char *nsa_hip_last_error(void);
/* Measurement / A-B switches (kernel form, staging, mapping).  Each switch is seeded once per process from the environment
 * variable NSA_HIP_<NAME> and can be changed afterwards only through this call (nothing reads the environment on the launch
 * path).  name: "SEL_ROWS", "ATTN_MAP", "ATTN_STAGE", "BAND_STAGE", "DECODE_UNFUSED", "SEL_BLOCKS", "DECODE_WG", "SEL_ROWSUM", "DECODE_STENCIL", "SEL_FUSE", "SCORES_FORM", "SEL_FLAT", "SEL_KSPLIT", "DECODE_STOP" (TIMELINE builds
 * only), "DECODE_WAVES", "DECODE_SPLIT", "DECODE_STEP", "DECODE_TEAM_SPIN", "DECODE_WIDE", "SEL_KSPLIT_T1", "SEL_KSPLIT_T2", "SCORES_SELECT", "DECODE_BAND", "DECODE_LONG" (with or without the NSA_HIP_ prefix); value -1 = automatic where the switch has an automatic setting.  Results never depend on a switch beyond the
 * tolerances stated for the entry point. */
NSA_API int nsa_hip_set_tuning(const char *name, int value);
NSA_API int nsa_hip_get_tuning(const char *name, int *value);
/* 0 if device `dev` is a gfx950 part; fills cu_count / total memory (host pointers, nullable). */
NSA_API int nsa_hip_device_check(int dev, int *cu_count, size_t *hbm_bytes);

/* ---------------------------------------------------------------------------------------
 * Selection attention forward.
 *   Q [B,S,G,h,Dk]  O [B,S,G,h,Dv]   contiguous
 *   K [B,G,S_kv,Dk] V [B,G,S_kv,Dv]  innermost dim contiguous; the b/g/token strides are given in
 *                                    ELEMENTS so a preallocated cache [B,G,S_max,D] can be passed
 *                                    without a copy (NSA_KV layout, nsa/cache/kv_cache.py:8-30)
 *   ranges [B,S,G,n,2] int32 [start,end) token ranges.  Semantics = union of the ranges after
 *          clamping to [0,S_kv] (attention_kernels.py:721-732); end<=start entries are ignored;
 *          a row with no allowed token yields zeros (attention_kernels.py:734-749,769-771).
 *   lse    [B,S,G,h] fp32, nullable: log-sum-exp of the scaled logits (needed by the backward).
 *   scale  softmax scale; pass <=0 for the default Dk^-1/2.
 *   variant 0 = auto, 1 = generic VALU kernel, 2 = MFMA kernels (bf16/f16, Dk=Dv in {64,128}, h<=16): with many rows the block form
 *           (8 consecutive rows of one (b,g) per wave walk the union of their 64-key blocks; from 64k keys on as two key halves on
 *           different XCDs plus a merge launch) or the query-tile form, with few rows (decode) one workgroup per row or one row per
 *           wave with its tiles split over several waves.
 *   workspace: nsa_sel_attn_fwd_workspace() bytes, 16-byte aligned (may be 0).  Holds the partial records when few rows are split
 *           over KV and when a long context is split into key halves (288 B per (row, head): sized for S_kv = S); with a smaller or
 *           no workspace the call falls back to the forms that need none.
 * ------------------------------------------------------------------------------------- */
NSA_API size_t nsa_sel_attn_fwd_workspace(int B, int S, int G, int h, int Dk, int Dv, int n_ranges, int dtype);
/* the same for query rows that are the LAST S positions of a longer context (S_kv > S: a chunk of a chunked prefill): the key-split form splits
 * rows by their position S_kv - S + row, so it may need records where the S_kv = S query above sees none.  A launch whose workspace is too
 * small for the split form runs the unsplit walk (same results within one ulp of the output dtype, slower at long contexts). */
NSA_API size_t nsa_sel_attn_fwd_workspace_kv(int B, int S, int G, int h, int Dk, int Dv, int S_kv, int n_ranges, int dtype);
NSA_API int nsa_sel_attn_fwd(const void *Q, const void *K, const void *V, const int32_t *ranges, void *O,
                     float *lse, int B, int S, int G, int h, int Dk, int Dv, int S_kv, int n_ranges,
                     int64_t k_stride_b, int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_b,
                     int64_t v_stride_g, int64_t v_stride_s, int dtype, float scale, int variant,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Opt-in PARITY MODE of the reference's default packed / gather executors (grouped_selection_attention_packed,
 * nsa/core/attention_kernels.py:273-388; grouped_selection_attention, :181-226): they call SDPA with is_causal=True and a single
 * query, so the query sees only the first gathered key and every head's output is V[b,g,start of the first non-empty range]
 * (slot order; ranges clamped to [0,S_kv] as everywhere here), zeros for a row without a range.  Not the semantics of the
 * selected branch -- kept so that outputs of the reference's default routing can be reproduced bit for bit. */
NSA_API int nsa_sel_attn_first_key_parity(const void *V, const int32_t *ranges, void *O, int B, int S, int G, int h, int Dv,
                                  int S_kv, int n_ranges, int64_t v_stride_b, int64_t v_stride_g, int64_t v_stride_s,
                                  int dtype, void *stream);

/* Opt-in PARITY MODE of NSAAttention._sdpa_over_ranges (nsa/core/nsa_attention.py:1779-1855), the reference's gather route of the
 * decode and sequential-prefill paths (what NSA_FORCE_PARITY=1 leaves them on, :704-708, :830, :1687): the union of the clamped ranges
 * is gathered in ascending token order and SDPA(is_causal=True) is called with the h heads in the query-length position, so head i
 * attends the first i+1 gathered tokens (top-left aligned causal mask).  Rows without a token give zeros.  h <= 16.  Not the
 * semantics of the selected branch -- kept so that outputs of the reference's forced-parity routing can be reproduced. */
NSA_API int nsa_sel_attn_head_causal_parity(const void *Q, const void *K, const void *V, const int32_t *ranges, void *O, int B, int S, int G,
                                    int h, int Dk, int Dv, int S_kv, int n_ranges, int64_t k_stride_b, int64_t k_stride_g,
                                    int64_t k_stride_s, int64_t v_stride_b, int64_t v_stride_g, int64_t v_stride_s, int dtype,
                                    float scale, void *stream);

/* Backward.  dO like O; dQ like Q (dtype); dK/dV are fp32 [B,G,S_kv,D] contiguous, fully written by the callee.
 * O and lse come from the forward.
 *   variant 0 auto, 1 generic (any dtype/shape: one wave per query row, dK/dV by fp32 atomics),
 *   2 MFMA (bf16/f16, Dk = Dv in {64, 128}, h <= 16): dQ query-major + dK/dV key-block-major, no atomics, reproducible.
 *   workspace: nsa_sel_attn_bwd_workspace() bytes (MFMA route: B*S*G*h floats for rowsum(dO*O) plus, when the query
 *   rows are split over workgroups, the per-split dK/dV partial sums that are added in fixed order; else 0). */
NSA_API size_t nsa_sel_attn_bwd_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_kv, int dtype, int variant);
NSA_API int nsa_sel_attn_bwd(const void *Q, const void *K, const void *V, const int32_t *ranges, const void *O,
                     const float *lse, const void *dO, void *dQ, float *dK, float *dV, int B, int S,
                     int G, int h, int Dk, int Dv, int S_kv, int n_ranges, int64_t k_stride_b,
                     int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_b, int64_t v_stride_g,
                     int64_t v_stride_s, int dtype, float scale, int variant, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Band attention forward: the sliding-window and the compressed branch (next row of the scope table after the selected
 * branch).  Query row t (absolute position t0 + t) attends the contiguous key interval [max(0, hi - w), hi) with
 *     hi(t) = (t0 + t + 1 >= a) ? min(S_kv, (t0 + t + 1 - a) / dd + c) : 0 ;
 *   sliding window (sliding_window_attention, nsa/core/attention_kernels.py:146-178): a = 0, dd = 1, c = 0, w = window;
 *   compressed (emission schedule num_cmp(t), attention_kernels.py:118-121): a = l, dd = d, c = 1, w = INT_MAX (K/V = K_cmp/V_cmp).
 * Layouts, strides, scale, lse and the empty-row rule (zeros, lse = -inf) as in nsa_sel_attn_fwd.  Prefill passes t0 = 0 and
 * all S rows; a decode step passes S = 1 and t0 = position of the new token.
 *   variant 0 = auto, 1 = generic VALU kernel (any dtype, D <= 256), 2 = MFMA kernel (bf16/f16, Dk = Dv in {64, 128}, h <= 16).
 * ------------------------------------------------------------------------------------- */
NSA_API size_t nsa_band_attn_fwd_workspace(int B, int S, int G, int h, int Dk, int Dv, int dtype);
NSA_API int nsa_band_attn_fwd(const void *Q, const void *K, const void *V, void *O, float *lse, int B, int S, int G, int h,
                      int Dk, int Dv, int S_kv, int64_t k_stride_b, int64_t k_stride_g, int64_t k_stride_s,
                      int64_t v_stride_b, int64_t v_stride_g, int64_t v_stride_s, int t0, int a, int dd, int c, int w,
                      int dtype, float scale, int variant, void *workspace, size_t workspace_bytes, void *stream);

/* Band attention backward (same interval rule and layouts as nsa_band_attn_fwd; O and lse from the forward; dQ in the activation
 * dtype, dK/dV fp32 [B,G,S_kv,D] fully written).  MFMA route (bf16/f16, Dk = Dv in {64, 128}): dQ by a dense query-major kernel (48
 * slots per wave at D = 64, 16 at D = 128), dK/dV by
 * the key-block-major kernels of nsa_sel_attn_bwd fed with one [lo,hi) range per row; otherwise the generic selection backward. */
NSA_API size_t nsa_band_attn_bwd_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_kv, int dtype, int variant);
NSA_API int nsa_band_attn_bwd(const void *Q, const void *K, const void *V, const void *O, const float *lse, const void *dO, void *dQ,
                      float *dK, float *dV, int B, int S, int G, int h, int Dk, int Dv, int S_kv, int64_t k_stride_b,
                      int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_b, int64_t v_stride_g, int64_t v_stride_s, int t0,
                      int a, int dd, int c, int w, int dtype, float scale, int variant, void *workspace, size_t workspace_bytes,
                      void *stream);

/* ---------------------------------------------------------------------------------------
 * Layer-level entry points: NSAAttention around the three branches (nsa/core/nsa_attention.py).  Plain-C descriptors:
 *   nsa_layer_desc  geometry + weights of one NSAAttention module (state-dict tensors, row-major [out,in] like nn.Linear;
 *                   W_qkv is the row-wise concatenation W_Q | W_K_sel | W_V_sel | W_K_win | W_V_win | W_K_cmp | W_V_cmp)
 *   nsa_kv_desc     the preallocated NSA_KV buffers (nsa/cache/kv_cache.py:8-26), each [B,G,S_max,D] contiguous,
 *                   K_cmp/V_cmp [B,G,n_cmp_max,D]
 * All tensors of one call share `dtype`.
 * ------------------------------------------------------------------------------------- */
typedef struct nsa_layer_desc {
    int dim, G, h, Dk, Dv, l, d, l_sel, n_sel, w, gate_hidden, dtype;
    float rope_base, rope_scale, gate_tau;
    const void *W_qkv;   /* [G*h*Dk + 3*G*Dk + 3*G*Dv, dim] */
    const void *W_out;   /* [dim, G*h*Dv] */
    const void *gate_w1; /* [gate_hidden, Dk] */
    const void *gate_b1; /* [gate_hidden] */
    const void *gate_w2; /* [3, gate_hidden] */
    const void *gate_b2; /* [3] */
} nsa_layer_desc;

typedef struct nsa_kv_desc {
    void *K_sel, *V_sel, *K_win, *V_win, *K_raw, *V_raw;
    void *K_cmp, *V_cmp;
    int B, S_max, n_cmp_max;
} nsa_kv_desc;

/* out[M,N] = epilogue(A[M,K] . W[N,K]^T) for few rows (decode projections).  epilogue 0: none, 1: silu, 2: + residual[M,N]. */
NSA_API int nsa_linear_small(const void *A, const void *W, void *out, int M, int N, int K, int dtype, int epilogue, const void *residual,
                     void *stream);
/* y[M,dim] = RMSNorm(x) * w, one wave per row, rounded where the reference's eager chain rounds (llama_block_nsa.py:10-19). */
NSA_API int nsa_rmsnorm_rows(const void *x, const void *w, void *y, int M, int dim, float eps, int dtype, void *stream);
/* Backward of nsa_rmsnorm_rows (training): dx[M,dim] and dw[dim] (activation dtype) from x, w, dy.  dim % 8 == 0, dim <= 4096, 16-byte
 * aligned tensors; dw is a fixed-order sum over workgroup partials (no atomics).  workspace: nsa_rmsnorm_rows_bwd_workspace bytes. */
NSA_API size_t nsa_rmsnorm_rows_bwd_workspace(int M, int dim);
NSA_API int nsa_rmsnorm_rows_bwd(const void *x, const void *w, const void *dy, void *dx, void *dw, int M, int dim, float eps, int dtype,
                         void *workspace, size_t workspace_bytes, void *stream);
/* RoPE (Q over the flattened head axis, K_sel/K_win per group; nsa_attention.py:552-572, 1002-1024) on a fused projection
 * proj [B,S,NQ+3GDk+3GDv] and append of the S tokens at cache position t0: Q_out [B,S,G,h,Dk]. */
NSA_API int nsa_rope_cache_append(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *proj, void *Q_out, int S, int t0,
                          void *stream);
/* Emit compressed tokens j0 <= j < j1: K_cmp[j] = mean_{i<l} RoPE(K_raw[j d + i]), V_cmp[j] = mean V_raw (compress_pool.py:9-38). */
NSA_API int nsa_cmp_pool_append(const nsa_layer_desc *L, const nsa_kv_desc *kv, int j0, int j1, void *stream);
/* Gate MLP + combine (nsa_attention.py:32-82, 85-124): O_out = sum_i gate_i O_i; gates_out [R,3] fp32 nullable; R = B*S*G rows. */
NSA_API int nsa_gate_combine(const nsa_layer_desc *L, const void *Q, const void *O_cmp, const void *O_sel, const void *O_win,
                     void *O_out, float *gates_out, int64_t R, void *stream);
/* Backward of the three layer kernels (training path; the attention branches have their own backward entry points).
 *   rope_cache_append_bwd: dQ [B,S,G,h,Dk] and the gradients of the S appended rows of each cache, [B,G,S,D] contiguous
 *                          (NULL = zero), -> dproj [B,S,NQ+3GDk+3GDv] (the rotation is undone on the gradient).
 *   cmp_pool_bwd:          dK_cmp/dV_cmp [B,G,n_cmp,D] -> dK_raw/dV_raw [B,G,S,D]  (raw rows 0..S-1, windows j d .. j d + l).
 *   gate_combine_bwd:      dO [R,h,Dv] -> dO_cmp/dO_sel/dO_win = gate_i dO and dgates [R,3] fp32 = sum O_i dO;
 *                          the gradient through the gate MLP (a [R,Dk] -> [R,3] network) is left to the caller. */
NSA_API int nsa_rope_cache_append_bwd(const nsa_layer_desc *L, int B, int S, int t0, const void *dQ, const void *dK_sel,
                              const void *dV_sel, const void *dK_win, const void *dV_win, const void *dK_raw,
                              const void *dV_raw, void *dproj, void *stream);
NSA_API int nsa_cmp_pool_bwd(const nsa_layer_desc *L, int B, int S, int n_cmp, const void *dK_cmp, const void *dV_cmp, void *dK_raw,
                     void *dV_raw, void *stream);
NSA_API int nsa_gate_combine_bwd(const nsa_layer_desc *L, const void *dO, const void *O_cmp, const void *O_sel, const void *O_win,
                         const float *gates, void *dO_cmp, void *dO_sel, void *dO_win, float *dgates, int64_t R, void *stream);
/* One decode step of a whole LlamaBlockNSA (nsa/model/llama_block_nsa.py:33-106: x + attn(norm1(x)), then + mlp(norm2(.))) in one
 * call: RMSNorm -> nsa_layer_decode_step with the residual added in the output projection's epilogue -> RMSNorm -> fc1 + silu ->
 * fc2 + residual.  x, y [B,dim]; the MLP weights are row-major [out,in] like nn.Linear. */
typedef struct nsa_block_desc {
    nsa_layer_desc attn;
    const void *norm1_w, *norm2_w; /* [dim] */
    const void *mlp_w1;            /* [mlp_hidden, dim] */
    const void *mlp_w2;            /* [dim, mlp_hidden] */
    int mlp_hidden;
    float norm_eps;
} nsa_block_desc;
NSA_API size_t nsa_block_decode_step_workspace(const nsa_block_desc *Bk, int B, int S_max);
NSA_API int nsa_block_decode_step(const nsa_block_desc *Bk, const nsa_kv_desc *kv, const void *x, void *y, int t, const int32_t *csc_ptr,
                          const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out,
                          void *workspace, size_t workspace_bytes, void *stream);

/* One decode step of a whole TinyLM-style stack (scripts/train_showcase.py:30-110) in one call: embedding rows of tokens[B] ->
 * n_blocks x nsa_block_decode_step (all at position t, each with its own cache) -> final RMSNorm -> LM head -> logits [B,vocab]
 * (activation dtype) and, when next_tokens != NULL, their argmax.  blocks / kvs are host arrays of n_blocks descriptors. */
NSA_API size_t nsa_model_decode_step_workspace(const nsa_block_desc *blocks, int n_blocks, int B, int S_max);
NSA_API int nsa_model_decode_step(const nsa_block_desc *blocks, const nsa_kv_desc *kvs, int n_blocks, const int32_t *tokens,
                          const void *embed, const void *norm_f_w, const void *lm_head, int vocab, void *logits,
                          int32_t *next_tokens, int t, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals,
                          int S_sel, void *workspace, size_t workspace_bytes, void *stream);

/* Prefill of the whole layer between the two big GEMMs, in one call (nsa_attention.py:978-1448 / 1521-1723): proj [B,S,NQ+3GDk+3GDv]
 * (= x @ W_qkv^T) -> RoPE + append of the S tokens into the EMPTY caches -> compressed-token pooling -> selection scores ->
 * top-n + selection attention -> sliding and compressed branches -> gates + combine -> O_mix [B,S,G*h*Dv] (input of the output
 * projection).  selector = NSA_SEL_BATCHED or NSA_SEL_SEQUENTIAL; ranges_out [B,S,G,W,2] with W = nsa_batched_ranges_width(S, ...)
 * resp. n_sel; gates_out [B,S,G,3] fp32 nullable.  csc_* / S_sel: Eq.9 map of the metadata for S tokens. */
NSA_API size_t nsa_layer_prefill_workspace(const nsa_layer_desc *L, int B, int S, int S_sel);
NSA_API int nsa_layer_prefill(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *proj, int S, int selector,
                      const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out,
                      int out_width, void *O_mix, float *gates_out, void *workspace, size_t workspace_bytes, void *stream);
/* Extend: S new tokens at positions t0 .. t0 + S - 1 onto caches that hold t0 tokens (t0 = 0: an empty cache), between the two big GEMMs in
 * one call, with the semantics of S decode steps (the next turn of a chat, a chunk of a chunked prefill, k draft tokens to verify): proj
 * [B,S,NQ+3GDk+3GDv] -> RoPE + append at t0 -> compressed tokens n_cmp(t0 - 1) <= j < n_cmp(t0 + S - 1) on the absolute schedule ->
 * DECODE-normalised scores (nsa_sel_scores_rows, q0 = t0, norm = 1) + sequential top-n at t (forced init and local blocks) -> selection
 * attention over K_sel[:t + 1] -> sliding and compressed branches at t -> gates + combine -> O_mix [B,S,G*h*Dv].  Caches, ranges and outputs
 * are those of S nsa_layer_decode_step calls up to the rounding of the different kernel forms; unlike nsa_layer_prefill (whose rows normalise
 * over every compressed token of the prompt) the result does not depend on how a prompt is split into chunks.  ranges_out [B,S,G,n_sel,2],
 * gates_out [B,S,G,3] fp32 nullable.  csc_* / S_sel: Eq.9 map of the metadata covering t0 + S tokens.  The workspace grows with the chunk
 * (p_grp is B*S*G*S_sel floats), not with the context. */
NSA_API size_t nsa_layer_extend_workspace(const nsa_layer_desc *L, int B, int S, int t0, int S_sel);
NSA_API int nsa_layer_extend(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *proj, int t0, int S, const int32_t *csc_ptr,
                     const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, void *O_mix, float *gates_out,
                     void *workspace, size_t workspace_bytes, void *stream);
/* One decode step of the whole layer in one call (nsa_attention.py:509-830, decode branch): x [B,dim] is the new token at
 * position t (= tokens already cached); appends it to the caches, emits a compressed token when due, runs the three branches,
 * the gate and the output projection -> y [B,dim].  csc_* / S_sel: the Eq.9 map of the block metadata covering t
 * (nsa_build_block_meta_host).  ranges_out [B,G,n_sel,2] int32 and gates_out [B,G,3] fp32 are nullable monitors.
 * The selected branch runs as the one-launch decode step (nsa_sel_decode_step) at Dk = Dv = 64 and 128.  The tuning switch
 * "DECODE_BAND" >= 1 (sliding + compressed branches on that launch, their splits merged there, the mix in the output projection)
 * applies to Dk = Dv = 64 only: at 128 the two branches are their own launches (mode 0) and gate + mix run as the gate kernel,
 * whatever the switch says.  The workspace size follows Dk / Dv. */
NSA_API size_t nsa_layer_decode_step_workspace(const nsa_layer_desc *L, int B, int S_max);
NSA_API int nsa_layer_decode_step(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *x, void *y, int t,
                          const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel,
                          int32_t *ranges_out, float *gates_out, void *workspace, size_t workspace_bytes, void *stream);
/* The decode step of the whole layer for S CONSECUTIVE tokens per sequence in one call (k draft tokens to verify, the tail of a chunked
 * prefill), 1 <= S <= 16: x [B,S,dim] holds the tokens of positions t0 .. t0 + S - 1 (t0 = tokens already cached, t0 + S <= S_max) and the call
 * does what S nsa_layer_decode_step calls at t = t0 .. t0 + S - 1 do -- the same caches, ranges, gates and y rows [B,S,dim]:
 *   1. the fused QKV projection of the B S rows with RoPE + cache append in its epilogue, row (b, s) rotated at and appended to position
 *      t0 + s (the MFMA form from B S >= 3 rows of bf16 / f16 on, else the chunk loop: where the single step at t0 + s projects on the same
 *      form, the cached bits are the single step's);
 *   2. the compressed tokens n_cmp(t0 - 1) <= j < n_cmp(t0 + S - 1) whose windows complete inside the call;
 *   3. the selected branch as nsa_sel_decode_rows (one launch, or its separate launches where that form declines);
 *   4. the sliding and the compressed branch of the S rows (one launch in split form where Dk = Dv = 64 allows, else one each);
 *   5. split combine + gates + mix (Dv = 64; the gate kernel otherwise), 6. the output projection of the B S rows.
 * Six launches at the m7c shape when a compressed token is due, five otherwise.  y is within the rounding of the band kernels' split
 * count of the single steps' rows; ranges are theirs wherever both project on the same form (B >= 3).
 * csc_* / S_sel: the Eq.9 map of block metadata covering t0 + S tokens.  ranges_out [B,S,G,n_sel,2] int32 and gates_out [B,S,G,3] fp32 are
 * nullable monitors.  workspace: nsa_layer_decode_rows_workspace() bytes, 256-byte aligned (0 for a null descriptor, B < 1 or S outside
 * [1,16]; at S = 1 not smaller than nsa_layer_decode_step_workspace).
 * nsa_layer_decode_rows_plan makes no HIP call and reports, for aligned caches of capacity S_max, *launches and *route = 1 (the selected
 * branch in its one-launch rows form) / 0 (its separate launches) / -1 with *launches = 0: DECLINED -- the caller should run S single steps.
 * Tuning switch "LAYER_DECODE_ROWS": 1 = never declined, 0 = always, -1 (default) = declined where the call was measured slower than S
 * single steps (S = 1).  nsa_layer_decode_rows itself runs whatever the switch says. */
NSA_API size_t nsa_layer_decode_rows_workspace(const nsa_layer_desc *L, int B, int S, int S_max);
NSA_API int nsa_layer_decode_rows(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *x, void *y, int t0, int S,
                          const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel,
                          int32_t *ranges_out, float *gates_out, void *workspace, size_t workspace_bytes, void *stream);
NSA_API int nsa_layer_decode_rows_plan(const nsa_layer_desc *L, int B, int S, int S_max, int t0, int S_sel, int *launches /* host */,
                               int *route /* host */);
/* The same for a RAGGED batch: every sequence at its own position, read on the device.  x / y [B,S,dim], 1 <= S <= 16; row (b, s) is the token
 * at position t_pos[b] + s of sequence b, whose slab of the caches already holds t_pos[b] tokens.  For every live sequence the call does
 * what nsa_layer_decode_rows(t0 = t_pos[b]) does to that sequence: the same appended cache rows, pooled tokens, ranges, gates and y rows.
 * t_pos: DEVICE int32 [B], 4-byte aligned.  t_max: the caller's HOST bound of t_pos[b] + S - 1.  With te = min(t_max, kv->S_max - 1) the host
 * checks that S_sel and kv->n_cmp_max cover te + 1 tokens and plans every launch from te, B and S alone; it never reads t_pos (no copy, no
 * synchronisation), so the arguments of the call do not change from token to token: advance t_pos on the device and call again.
 * A sequence with t_pos[b] < 0 or t_pos[b] + S - 1 > te is INACTIVE -- the padding slot of a batch, and the guard that keeps a wrong
 * position inside the buffers (nothing is clamped silently): NOTHING is written to any of its eight cache tensors, its y and ranges_out
 * rows are zero, its gates_out rows are UNSPECIFIED (the gate is evaluated from whatever Q the projection left in the workspace; x rows
 * of an inactive sequence must still be finite for its y rows to be zero).  Rows of a slab beyond its own sequence are never read:
 * every kernel bounds its loads by the sequence's own last token, so what an allocator left there (NaN patterns included) is harmless.
 * Six launches at Dk = Dv = 64, always: 1. the fused QKV projection with RoPE + append at t_pos[b] + s, 2. pooling (launched every call,
 * since the host cannot know whether a window completes: ceil(S / d) blocks per (b, g), which exit where none does), 3. the selected
 * branch as the rows form of nsa_sel_decode_ragged, 4. the sliding and the compressed branch in one launch, 5. split combine + gates +
 * mix, 6. the output projection.  At Dk = Dv = 128 the band branches are one ragged launch each and the gate kernel stands in for 5.
 * There is no scalar route to stand in, so the call DECLINES with NSA_ERR_INVALID and a message naming the limit wherever
 * nsa_sel_decode_ragged does: a dtype other than bf16 / f16, anything but Dk = Dv in {64, 128} and the default block geometry, te beyond the
 * unsplit forms (with the tuning switch DECODE_LONG = 1: te beyond 131,071, the limit of the long-row form the selected branch then runs --
 * same launch count, same workspace), DECODE_STEP = 0 or DECODE_UNFUSED = 1, a null or misaligned operand, S outside [1,16].
 * nsa_layer_decode_ragged_plan makes no HIP call: NSA_OK with *launches = n and *route = 1, or *launches = 0 and *route = -1 for a declined
 * shape; an error status for bad arguments.  workspace: nsa_layer_decode_ragged_workspace() bytes, 256-byte aligned -- not less than
 * nsa_layer_decode_rows_workspace(L, B, S, S_max), and 0 for the arguments that call answers 0 for. */
NSA_API size_t nsa_layer_decode_ragged_workspace(const nsa_layer_desc *L, int B, int S, int S_max);
NSA_API int nsa_layer_decode_ragged(const nsa_layer_desc *L, const nsa_kv_desc *kv, const void *x, void *y,
                            const int32_t *t_pos /* device [B] */, int t_max /* host */, int S, const int32_t *csc_ptr,
                            const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out,
                            void *workspace, size_t workspace_bytes, void *stream);
NSA_API int nsa_layer_decode_ragged_plan(const nsa_layer_desc *L, int B, int S, int S_max, int t_max, int S_sel, int *launches /* host */,
                                 int *route /* host */);

/* The ragged layer decode over PAGED caches: nsa_layer_decode_ragged with all eight cache tensors held in pools of fixed-size pages and
 * found through a device block table -- the layer around nsa_sel_decode_paged and nsa_band_attn_fwd_paged, and the one place that WRITES
 * a token into a page.
 *   nsa_paged_kv_desc   K_sel, V_sel, K_win, V_win, K_raw, V_raw  [n_pages, G, 1024, D] and K_cmp, V_cmp [n_pages, G, 64, D], each contiguous
 *                 (as nsa_kv_desc requires of its slabs) and 16-byte aligned.  block_table: device int32 [B, max_pages], table_stride
 *                 elements between its rows (>= max_pages).  ONE page id serves all eight pools: entry [b, j] holds tokens
 *                 [1024 j, 1024 j + 1024) and compressed rows [64 j, 64 j + 64) of sequence b.  The capacity that stands for S_max is
 *                 max_pages * 1024 (max_pages <= 2^20).  Page bases are formed in 64 bits, so a pool may exceed 2 GiB.
 *                 OWNERSHIP: the page a live sequence appends to -- the page(s) of positions t_pos[b] .. t_pos[b] + S - 1 and of the
 *                 compressed rows emitted there -- must belong to that sequence ALONE.  A page may be shared between sequences (a common
 *                 prefix) only once it is CLOSED: page j of a sequence of t tokens is closed when t >= 1024 (j + 1) + 16, equivalently
 *                 n_cmp(t) >= 64 (j + 1).  Until then its last compressed row, 64 j + 63 -- pooled from raw rows 1024 j + 1008 ..
 *                 1024 j + 1039 -- is still to be written, so two sequences that share the page and diverge at a position in
 *                 [1024 (j + 1), 1024 (j + 1) + 16) would both write it.  The kernels check none of this: two sequences appending to one
 *                 page overwrite each other.  The allocator does: NSA_PagedKV.fork / own_tail / truncate (nsa_vibe_amd/kv_cache.py) share
 *                 closed pages only, by reference count, and give a sequence private copies of the others (nsa_paged_kv_copy_pages).
 *   x, y, t_pos, t_max, S, csc_*, S_sel, ranges_out, gates_out   as in nsa_layer_decode_ragged; te = min(t_max, max_pages * 1024 - 1).  The
 *                 host reads neither t_pos nor the table, and the arguments do not change from token to token.
 * One verdict per sequence: the call's first launch, one wave per sequence, writes t_live[b] into the workspace -- t_pos[b] where the
 * sequence is live under the ragged rule (0 <= t_pos[b], t_pos[b] + S - 1 <= te) AND every table entry j = 0 .. (t_pos[b] + S - 1) >> 10
 * lies in [0, n_pages); -1 otherwise.  Every later launch takes t_live as its position array, so writers and readers agree: an inactive
 * sequence appends NOTHING to any pool and gets zero y and ranges_out rows (gates_out rows unspecified, as in the ragged call).  Beyond the
 * verdict every kernel forms an address only from a table entry it has itself tested against [0, n_pages): the two writers re-test the
 * one or two entries they use, the readers test as nsa_sel_decode_paged / nsa_band_attn_fwd_paged do.  No table value can send a load or
 * a store outside the pools; nothing is clamped silently.
 * Launches: 0. the verdicts, 1. the fused QKV projection with RoPE + append (row (b, s) at pos = t_live[b] + s goes to row pos & 1023 of
 * page table[b][pos >> 10] of the six token pools; the S rows of a sequence may lie in two pages), 2. pooling (compressed row j =
 * n_cmp(t_live[b]) + k from raw rows [16 j, 16 j + 32), every one found through its own page -- j = 63 reads rows 1008 .. 1039 -- into row
 * j & 63 of page table[b][j >> 6]), 3. nsa_sel_decode_paged's launch, 4. the sliding and the compressed branch as one
 * nsa_band_attn_fwd_paged launch each (page_rows 1024 / 64; in split form each is followed by its combine), 5. gates + mix (the finish
 * kernel at Dv = 64, the gate kernel at 128), 6. the output projection.  Ten launches at the m7c shape.
 * Bits: for a table that scatters contiguous slabs into pages, in any order, the appended rows, the pooled rows and the ranges are those of
 * nsa_layer_decode_ragged on the slabs bit for bit; at Dv = 128 y and the gates too.  At Dv = 64 the ragged call merges the band splits in
 * its finish kernel while this call combines per branch: y is within the rounding of that.
 * DECLINES with NSA_ERR_INVALID and a message naming the limit, no fallback, wherever nsa_layer_decode_ragged and the two paged operators
 * do: a dtype other than bf16 / f16, anything but Dk = Dv in {64, 128} and the default block geometry, h > 16, w < 1, te beyond the unsplit
 * forms (with the tuning switch DECODE_LONG = 1: te beyond 131,071, the limit of the long-row form the selected branch then runs -- same
 * launch count, same workspace), DECODE_STEP = 0 or DECODE_UNFUSED = 1, S outside [1,16], a null or misaligned operand, max_pages outside
 * [1, 2^20], n_pages < 1, a table stride below max_pages.
 * nsa_layer_decode_paged_plan makes no HIP call: NSA_OK with *launches = n and *route = 1, or *launches = 0 and *route = -1 for a declined
 * shape; an error status for bad arguments.  workspace: nsa_layer_decode_paged_workspace() bytes, 256-byte aligned (0 for a null descriptor,
 * B < 1, S outside [1,16] or max_pages outside [1, 2^20]); it does not grow with max_pages beyond 2^17 tokens, the contexts the forms reach. */
typedef struct nsa_paged_kv_desc {
    void *K_sel, *V_sel, *K_win, *V_win, *K_raw, *V_raw; /* [n_pages, G, 1024, D] */
    void *K_cmp, *V_cmp;                                 /* [n_pages, G, 64, D] */
    const int32_t *block_table;                          /* device, [B, max_pages] */
    int64_t table_stride;
    int n_pages, B, max_pages;
} nsa_paged_kv_desc;
NSA_API size_t nsa_layer_decode_paged_workspace(const nsa_layer_desc *L, int B, int S, int max_pages);
NSA_API int nsa_layer_decode_paged(const nsa_layer_desc *L, const nsa_paged_kv_desc *pkv, const void *x, void *y,
                           const int32_t *t_pos /* device [B] */, int t_max /* host */, int S, const int32_t *csc_ptr,
                           const int32_t *csc_rows, const float *csc_vals, int S_sel, int32_t *ranges_out, float *gates_out,
                           void *workspace, size_t workspace_bytes, void *stream);
NSA_API int nsa_layer_decode_paged_plan(const nsa_layer_desc *L, int B, int S, int max_pages, int t_max, int S_sel, int *launches /* host */,
                                int *route /* host */);

/* Copies between a contiguous cache and the pages of a paged one, and between pages: how a prefilled sequence ENTERS the pools (admission),
 * leaves them, and how a sequence gets a private copy of a page it shares.  Plain streaming copies, ONE launch per call, 16-byte loads and
 * stores.  G, Dk, Dv, dtype: the geometry of the pools and the cache (the descriptors hold pointers and extents only); bf16 / f16,
 * Dk and Dv in {64, 128}.  Every address is formed in 64 bits: pools and caches may exceed 2 GiB.
 *   nsa_paged_kv_store   token rows [t0, t1) of the six token tensors of slab b_src of `kv` ([B, G, S_max, D], contiguous) go to the pages of table
 *                  row `slot`: row r to row r & 1023 of page table[slot][r >> 10].  The same launch copies compressed rows
 *                  [n_cmp(t0), n_cmp(t1)) of K_cmp / V_cmp ([B, G, n_cmp_max, D]): row c to row c & 63 of page table[slot][c >> 6]
 *                  (n_cmp(t) = 0 below t = 32, else (t - 32) / 16 + 1: the default block geometry).
 *   nsa_paged_kv_load    the same arguments, the other way: pages -> slab.
 *   nsa_paged_kv_copy_pages   jobs: DEVICE int32 [n_jobs, 4] of (src_page, dst_page, n_tokens, n_cmp_rows).  For every job, token rows
 *                  [0, n_tokens) of the six token pools and compressed rows [0, n_cmp_rows) of the two compressed pools go from page src
 *                  to page dst.  The jobs of one launch must not write a page that another of them reads or writes.
 * The host reads neither the table nor the jobs.  A kernel forms an address only from a page id it has itself tested against [0, n_pages):
 * the rows of a table entry outside that range are SKIPPED (nothing is read or written for them), and so is a whole job with a page id
 * outside it, n_tokens outside [0, 1024] or n_cmp_rows outside [0, 64].  Nothing is clamped silently; no table or job value can send a load
 * or a store outside the pools or the slab; rows outside the ranges, and every other page, are left untouched.
 * NSA_ERR_INVALID with a message naming the limit, and no launch, for: a null pointer; a pool, cache or table that is misaligned (16 / 16 /
 * 4 bytes; the job array 4); a table stride below max_pages; t0 < 0, t1 < t0; t1 beyond kv->S_max or max_pages * 1024; n_cmp(t1) beyond
 * kv->n_cmp_max; a dtype other than bf16 / f16; Dk or Dv outside {64, 128}; slot outside [0, pkv->B); b_src outside [0, kv->B); G < 1;
 * n_pages < 1; max_pages outside [1, 2^20]; n_jobs < 0.  t0 == t1 and n_jobs == 0: NSA_OK, no launch. */
NSA_API int nsa_paged_kv_store(const nsa_paged_kv_desc *pkv, const nsa_kv_desc *kv, int b_src, int slot, int t0, int t1, int G, int Dk, int Dv,
                       int dtype, void *stream);
NSA_API int nsa_paged_kv_load(const nsa_paged_kv_desc *pkv, const nsa_kv_desc *kv, int b_src, int slot, int t0, int t1, int G, int Dk, int Dv,
                      int dtype, void *stream);
NSA_API int nsa_paged_kv_copy_pages(const nsa_paged_kv_desc *pkv, const int32_t *jobs /* device [n_jobs, 4] */, int n_jobs, int G, int Dk, int Dv,
                            int dtype, void *stream);

/* ---------------------------------------------------------------------------------------
 * Eq.9 map in gather (CSC) form.  For selection block j the entries csc_ptr[j]..csc_ptr[j+1]
 * list (cmp row, weight) in ASCENDING cmp row -- the order the reference's CPU scatter_add
 * accumulates in -- so p_slc is bit-identical to the reference given an identical fp32 p_cmp.
 * nsa_build_block_meta_host fills both the reference's CSR/COO arrays and this CSC (host
 * pointers; call with NULL arrays to get the sizes).
 * ------------------------------------------------------------------------------------- */
NSA_API int nsa_block_counts(int seq_len, int l, int d, int l_sel, int *S_cmp, int *S_sel, int *nnz);
NSA_API int nsa_build_block_meta_host(int seq_len, int l, int d, int l_sel, int32_t *csr_indptr /*S_cmp+1*/,
                              int32_t *csr_indices /*nnz*/, float *csr_values /*nnz*/,
                              int32_t *csc_ptr /*S_sel+1*/, int32_t *csc_rows /*nnz*/,
                              float *csc_vals /*nnz*/);

/* p_cmp [R,h,S_cmp_cur] fp32 -> p_slc [R,h,S_sel] (nullable) and p_grp [R,S_sel] (Eq.10, heads
 * summed in ascending h).  CSC rows >= S_cmp_cur are dropped (selection_scorer.py:103-108). */
NSA_API int nsa_map_pcmp_to_pgrp(const float *p_cmp, int64_t R, int h, int S_cmp_cur, const int32_t *csc_ptr,
                         const int32_t *csc_rows, const float *csc_vals, int S_sel, float *p_slc,
                         float *p_grp, void *stream);

/* p_cmp = softmax over ALL S_cmp columns of Q K_cmp^T * scale, fp32 out [B,S,G,h,S_cmp].
 * Q [B,S,G,h,Dk] contiguous; K_cmp [B,G,S_cmp,Dk] with element strides. */
NSA_API int nsa_pcmp_all(const void *Q, const void *K_cmp, float *p_cmp, int B, int S, int G, int h, int Dk,
                 int S_cmp, int64_t kc_stride_b, int64_t kc_stride_g, int64_t kc_stride_s, int dtype,
                 float scale, void *stream);

/* Fused scorer: Q,K_cmp -> p_grp [B,S,G,S_sel] fp32 without materialising p_cmp / p_slc.
 *   l, d, l_sel: the block geometry the CSC was built for.  For l = 2d, l' = 4d (the reference default
 *   32/16/64) and bf16/f16 inputs with Dk in {64,128}, h <= 16, a single MFMA kernel evaluates Eq.9 in
 *   closed form; every other case runs the query-chunked generic path and needs the workspace.
 *   causal_skip != 0: entries p_grp[b,t,g,j] of blocks the selector can never pick at t
 *   ((j+1) l' > t+1, masked to -inf by both selectors) need not be computed: such an entry is returned as 0 -- or, on the MFMA route, as
 *   its full computed value where the workgroup of the query (64 / 32 consecutive queries share a sweep that stops at the LAST block any
 *   of them can read) computed the block for a later query of the group.  causal_skip == 2 additionally leaves the entries no query of the
 *   workgroup can read UNWRITTEN (saves the zero fill of p_grp -- 512 MiB at S = 64k).  Either way only entries with (j+1) l' <= t+1 are
 *   defined values of the reference: a caller that sums or ranks p_grp itself must apply that mask (both selectors here do).
 *   Few query rows (B*S*G <= 1024: decode) run a decode-shaped pair of kernels that spreads the K_cmp sweep of a
 *   row over many workgroups (any dtype / geometry); it needs B*S*G*h*S_cmp floats of workspace.
 *   variant: 0 auto, 1 generic, 2 MFMA (prefill), 3 decode-shaped.
 *   workspace: nsa_sel_scores_workspace(same shape/geometry/dtype/variant) bytes (0 for the MFMA route). */
NSA_API size_t nsa_sel_scores_workspace(int B, int S, int G, int h, int Dk, int S_cmp, int S_sel, int l, int d, int l_sel,
                                int dtype, int variant);
NSA_API int nsa_sel_scores(const void *Q, const void *K_cmp, float *p_grp, int B, int S, int G, int h, int Dk,
                   int S_cmp, int64_t kc_stride_b, int64_t kc_stride_g, int64_t kc_stride_s,
                   const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel,
                   int l, int d, int l_sel, int causal_skip, int variant /* 0 auto, 1 generic, 2 MFMA, 3 decode */,
                   int dtype, float scale, void *workspace, size_t workspace_bytes, void *stream);
/* The same scorer for query rows at absolute positions (a chunk of a chunked prefill, an extend of a filled cache, speculative-verify rows):
 *   q0   absolute position of query row 0: row (b,s,g) sits at token t = q0 + s; causal_skip counts blocks from t.
 *   norm 0 = softmax over all S_cmp columns (nsa_sel_scores, q0 = 0: the same kernels and bits);
 *        1 = DECODE normalisation: row t normalises over its own n_cmp(t) = (t + 1 < l) ? 0 : (t + 1 - l) / d + 1 columns (clamped to
 *            S_cmp), the compressed tokens a decode step at t sees (nsa/core/nsa_attention.py:651); columns c >= n_cmp(t) contribute nothing to
 *            Eq.9 / 10.  This deliberately differs from the one-shot prefill, whose rows normalise over every compressed token of the prompt.
 *   With norm = 1 every route bounds its sweeps by the rows it holds (the first sweep becomes triangular), the decode-shaped pair is taken only
 *   for chunks of fewer than 64 rows, and a row's p_grp bits do not depend on the chunk it sits in when chunk boundaries are multiples of 64.
 *   Results are bitwise reproducible run to run.  workspace: nsa_sel_scores_rows_workspace(same shape, variant, norm) bytes.
 * Note for nsa_sel_scores / nsa_sel_scores_select: their causal_skip counts blocks from row 0, so rows that are not at tokens 0 .. S - 1 need
 * causal_skip = 0 there (or these entry points). */
NSA_API size_t nsa_sel_scores_rows_workspace(int B, int S, int G, int h, int Dk, int S_cmp, int S_sel, int l, int d, int l_sel, int dtype,
                                     int variant, int norm);
NSA_API int nsa_sel_scores_rows(const void *Q, const void *K_cmp, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp,
                        int64_t kc_stride_b, int64_t kc_stride_g, int64_t kc_stride_s, const int32_t *csc_ptr, const int32_t *csc_rows,
                        const float *csc_vals, int S_sel, int l, int d, int l_sel, int causal_skip, int variant, int dtype, float scale,
                        int q0, int norm, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Deterministic top-n + forced blocks + range merge.
 *   p_grp [R,S_sel] fp32 with R = B*S*G rows ordered (b,s,g); row r sits at token
 *   t = t0 + (r / G) % S  (decode: S = 1, t0 = current position), or t_rows[r] if non-NULL.
 *   mode NSA_SEL_SEQUENTIAL: out [R,n_top,2]; mode NSA_SEL_BATCHED: out [R,K,2] with
 *   K = nsa_batched_ranges_width(...); out_width must equal that width.
 *   Ranking key = fp32(p) - fp32(idx)*1e-8f (unfused), descending, index ascending on ties.
 *   Sequential-mode note: where the reference's topk would have to pick -inf entries (fewer valid
 *   candidates than n_top - 3) it emits inverted garbage ranges; this ABI emits [0,0] instead.
 * ------------------------------------------------------------------------------------- */
NSA_API int nsa_batched_ranges_width(int S, int S_sel, int l_sel, int n_top, int force_init, int force_local);
NSA_API int nsa_select_topn_ranges(const float *p_grp, int64_t R, int S, int G, int t0, const int32_t *t_rows,
                           int S_sel, int l_sel, int n_top, int force_init, int force_local, int mode,
                           int S_total /* batched: the S the forced-column rule is evaluated for */,
                           int32_t *ranges_out, int out_width, void *stream);

/* ---------------------------------------------------------------------------------------
 * Scores + top-n selection in one call (prefill; round 4): the arguments of nsa_sel_scores (variant 0) followed by those of
 * nsa_select_topn_ranges (rows in the [B,S,G] order of Q, token of row (b,s,g) = t0 + s).  Replaces compute_pcmp_all ->
 * map_pcmp_to_pslc_batched -> sum(dim=3) -> select_topn_ranges[_batched] (nsa/core/nsa_attention.py:1088-1108, 1566-1576;
 * nsa/core/selection_scorer.py:42-61, 89-116, 124-249, 255-362).  Where the 32x32x16 MFMA scorer applies (h = 6, Dk = 64, default block
 * geometry, bf16 / f16, S_sel <= 1024) and the context is long enough for it to pay (S_cmp >= 3072; tuning switch "SCORES_SELECT") a workgroup
 * selects the ranges of its 64 query rows right behind its second sweep, with the select kernel's own row function: ONE launch, the scores are read back out of L2 (no HBM read of p_grp), the selector's scalar work runs beside
 * the scorer's matrix / vector work.  Everywhere else the scorer and the select kernel are launched back to back.  p_grp is still written
 * (same contract as nsa_sel_scores with the given causal_skip); ranges_out is bit-identical to the two separate calls either way.
 * workspace: the larger of nsa_sel_scores_workspace(..., variant 0) and (..., variant 1) bytes (rows that are not 16-byte aligned take the
 * generic scorer).
 * ------------------------------------------------------------------------------------- */
NSA_API int nsa_sel_scores_select(const void *Q, const void *K_cmp, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp,
                          int64_t kc_stride_b, int64_t kc_stride_g, int64_t kc_stride_s, const int32_t *csc_ptr, const int32_t *csc_rows,
                          const float *csc_vals, int S_sel, int l, int d, int l_sel, int causal_skip, int dtype, float scale, int t0,
                          int n_top, int force_init, int force_local, int mode, int S_total, int32_t *ranges_out, int out_width,
                          void *workspace, size_t workspace_bytes, void *stream);
/* nsa_sel_scores_select with the q0 / norm of nsa_sel_scores_rows (scorer rows at q0 + s; t0 stays the selector's token of row 0, normally
 * t0 = q0).  workspace: the larger of nsa_sel_scores_rows_workspace(..., variant 0, norm) and (..., variant 1, norm) bytes. */
NSA_API int nsa_sel_scores_select_rows(const void *Q, const void *K_cmp, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp,
                               int64_t kc_stride_b, int64_t kc_stride_g, int64_t kc_stride_s, const int32_t *csc_ptr, const int32_t *csc_rows,
                               const float *csc_vals, int S_sel, int l, int d, int l_sel, int causal_skip, int dtype, float scale, int t0,
                               int n_top, int force_init, int force_local, int mode, int S_total, int32_t *ranges_out, int out_width, int q0,
                               int norm, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Top-n selection + selection attention in one call (prefill): the arguments of nsa_select_topn_ranges followed by those of
 * nsa_sel_attn_fwd; ranges_out [B,S,G,out_width,2] is produced AND consumed.  The select kernel and the attention kernel are
 * launched back to back on the stream (the default since round 2: the selector is faster as its own launch); with the tuning
 * switch SEL_FUSE = 1 the selection runs inside the attention kernel on the MFMA route (one launch).  Results are those of the
 * two separate calls, bit for bit, either way.
 * ------------------------------------------------------------------------------------- */
NSA_API int nsa_sel_select_attn_fwd(const float *p_grp, int t0, const int32_t *t_rows, int S_sel, int l_sel, int n_top, int force_init,
                            int force_local, int mode, int S_total, int32_t *ranges_out, int out_width, const void *Q, const void *K,
                            const void *V, void *O, float *lse, int B, int S, int G, int h, int Dk, int Dv, int S_kv,
                            int64_t k_stride_b, int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_b, int64_t v_stride_g,
                            int64_t v_stride_s, int dtype, float scale, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * One decode step of the selected branch in ONE call (host launch overhead matters at batch 1):
 *   Q [B,1,G,h,Dk] -> decode-shaped scores -> sequential top-n ranges at token t_token -> selection attention over
 *   K/V[:, :, :S_kv].  Replaces the calls of the decode branch of NSAAttention.forward
 *   (nsa/core/nsa_attention.py:651 compute_pcmp_all, :658 map_pcmp_to_pslc_batched, :670 head sum,
 *   :672 select_topn_ranges, :704-830 selection executor).
 *   ranges_out [B,G,n_top,2] int32, O [B,1,G,h,Dv]; workspace: nsa_sel_decode_step_workspace() bytes, 16-B aligned.
 *   Kernel form (one launch wherever the default block geometry, bf16 / f16 and Dk = Dv in {64, 128} allow): chosen from (B*G, S_cmp) -- logits
 *   in registers for rows of up to 32 chunks of 64 compressed rows, a team of workgroups per row for longer rows while B*G teams fit the
 *   chip, and for more rows than that (B >= 128 at a 64k context) the one-pass form, whose group scores carry one more rounding (<= 2 ulp)
 *   than the other forms': its ranges are theirs wherever the (n_top - 3)-th and the next ranking key differ by more than that (tuning
 *   switch "DECODE_WIDE": 0 = never, 1 = the exact one-workgroup form instead).  Every form is bitwise reproducible run to run.
 *   Dk = Dv = 128: the exact forms with the logits in registers only (eight waves per row, one workgroup per CU; a row of more than 16
 *   chunks as a team of workgroups while B*G teams fit the chip).  Shapes beyond that -- more rows at a long context than teams fit (B*G*4
 *   workgroups > CUs at 64k), DECODE_WIDE forms -- take the separate launches (scores + top-n, then the decode attention), whose
 *   results are the same bits: the decode attention of both routes runs the same row functions.
 *   nsa_sel_decode_step_workspace does not depend on the route: it covers the team form's records (independent of Dk) and the scratch of
 *   the separate launches for the given Dk / Dv.
 *   nsa_sel_decode_step_plan reports what nsa_sel_decode_step does with a shape under the current tuning switches, assuming the default
 *   block geometry (l = 2d, l' = 4d = 64), 16-byte aligned pointers and contiguous rows: *launches = 1 exactly when the call is the
 *   one-launch step; for a declined shape it is an estimate (> 1) of the launches of the separate route -- only "> 1" is contractual there --, *form = 0 logits in registers / 1 four chunks per wave / 2 one-pass (-1 when the step is declined), *nsplit =
 *   workgroups per row (0 when declined).
 * ------------------------------------------------------------------------------------- */
NSA_API size_t nsa_sel_decode_step_workspace(int B, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype);
NSA_API int nsa_sel_decode_step(const void *Q, const void *K_cmp, const void *K, const void *V, const int32_t *csc_ptr,
                        const int32_t *csc_rows, const float *csc_vals, int32_t *ranges_out, void *O, int B, int G, int h,
                        int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int l, int d, int l_sel, int n_top, int t_token,
                        int64_t kc_stride_b, int64_t kc_stride_g, int64_t kc_stride_s, int64_t k_stride_b,
                        int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_b, int64_t v_stride_g,
                        int64_t v_stride_s, int dtype, float scale, void *workspace, size_t workspace_bytes, void *stream);
NSA_API int nsa_sel_decode_step_plan(int B, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int n_top, int dtype,
                             int *launches /* host */, int *form /* host */, int *nsplit /* host */);

/* ---------------------------------------------------------------------------------------
 * The decode step of the selected branch for S CONSECUTIVE tokens per sequence in one call (k draft tokens to verify, the tail of a chunked
 * prefill): the cache already holds the S new tokens, row (b,s,g) sits at token t = t0 + s and computes what nsa_sel_decode_step computes at
 * t on the cache truncated to t + 1 tokens:
 *   it sees the first n_cmp(t) = (t + 1 < l) ? 0 : (t + 1 - l) / d + 1 rows of K_cmp[b,g] (clamped to S_cmp) and normalises its compressed
 *   scores over those columns alone (the decode semantics of nsa_sel_scores_rows(q0 = t0, norm = 1)), selects sequentially at t with the
 *   forced initial and local blocks, and attends K/V[b,g,:t+1].
 *   Q [B,S,G,h,Dk], O [B,S,G,h,Dv], ranges_out [B,S,G,n_top,2] int32; K_cmp / K / V and their strides as in nsa_sel_decode_step.
 *   S_cmp, S_sel, S_kv describe the cache AFTER the S tokens were appended (the block meta of t0 + S tokens); S_kv >= t0 + S.
 * Every sequence of this call sits at the same t0: every row's bounds follow from its index, S and t0.  A batch whose sequences sit at
 * different positions is nsa_sel_decode_ragged (below), the same kernel form with a device array of positions.
 * Kernel form: ONE launch -- the decode step's kernel with one workgroup per row, each deriving its own token, compressed rows and chunks
 * from the row index -- on the unsplit exact forms only: logits in registers (two chunks of 64 compressed rows per wave, 8 or 16 waves by
 * B*S*G) at Dk = Dv in {64, 128}, four chunks per wave at 64 where the LARGEST row (t0 + S - 1) exceeds that, whatever DECODE_WIDE says;
 * no team of workgroups, no one-pass form, no band workgroups.  Ranges and O have the bits of S nsa_sel_decode_step calls that run the
 * same number of waves per row (sel_attn_decode.hpp: 16 up to 256 rows per launch at D = 64, else 8); ranges are theirs bit for bit always.
 * Everywhere else -- another block geometry than l = 2d, l' = 4d = 64, n_cmp(t0) < 1, S > 16, other dtypes, a largest row beyond the unsplit
 * forms (more than 64 / 32 / 16 chunks at 16 waves / 8 waves / D = 128), DECODE_UNFUSED = 1, unaligned inputs -- the call runs the separate
 * launches: nsa_sel_scores_select_rows(q0 = t0, norm = 1, sequential) then nsa_sel_attn_fwd (same ranges; O within the rounding of the
 * attention kernel forms).  Tuning switch "DECODE_ROWS": 1 = the one-launch form wherever it applies, 0 = never, -1 (default) = in the
 * (S, context) cells where it was measured not slower than both S single steps and the separate launches (DESIGN.md 4.1f has the table: every measured cell except S = 1 on rows of 32 chunks and more; cells
 * where it loses default to the separate launches).
 * nsa_sel_decode_rows_plan reports the route for a cache that holds exactly t0 + S tokens (t0 = S_kv - S), default geometry and aligned
 * inputs assumed: *launches = 1 and *form = 0 / 1 for the one-launch form, else *launches > 1 (an estimate) and *form = -1.
 * workspace: nsa_sel_decode_rows_workspace() bytes, 16-byte aligned (the scratch of the separate launches; the one-launch form uses none).
 * ------------------------------------------------------------------------------------- */
NSA_API size_t nsa_sel_decode_rows_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype);
NSA_API int nsa_sel_decode_rows(const void *Q, const void *K_cmp, const void *K, const void *V, const int32_t *csc_ptr,
                        const int32_t *csc_rows, const float *csc_vals, int32_t *ranges_out, void *O, int B, int S, int G, int h,
                        int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int l, int d, int l_sel, int n_top, int t0,
                        int64_t kc_stride_b, int64_t kc_stride_g, int64_t kc_stride_s, int64_t k_stride_b,
                        int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_b, int64_t v_stride_g,
                        int64_t v_stride_s, int dtype, float scale, void *workspace, size_t workspace_bytes, void *stream);
NSA_API int nsa_sel_decode_rows_plan(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int n_top, int dtype,
                             int *launches /* host */, int *form /* host */);

/* ---------------------------------------------------------------------------------------
 * Ragged-batch decode step of the selected branch: nsa_sel_decode_rows with the position of every sequence read from a DEVICE array.
 * Shapes as there (Q [B,S,G,h,Dk], O [B,S,G,h,Dv], ranges_out [B,S,G,n_top,2], 1 <= S <= 16); row (b,s,g) sits at token
 * t = t_pos[b] + s and computes what nsa_sel_decode_step computes at t on sequence b's cache truncated to t + 1 tokens: its own n_cmp(t)
 * compressed rows, normalised over those alone, sequential selection at t, attention over K/V[b,g,:t+1].
 *   t_pos  device int32 [B].  The host never reads it: no copy, no synchronisation, and the call's arguments need not change from token
 *          to token (a captured graph can advance the array on the device).
 *   t_max  host upper bound of t_pos[b] + S - 1 over the batch.  Form and waves per row are planned from t_max and B*S*G exactly as the
 *          rows form plans from t0 + S - 1: logits in registers (form 0) or, at D = 64, four chunks per wave (form 1); 8 or 16 waves.
 *   S_cmp, S_sel, S_kv describe the caches' CAPACITY bound: the block metadata of at least min(t_max, S_kv - 1) + 1 tokens, and the rows
 *          the buffers may be read up to.
 * Inactive sequences: t_pos[b] < 0, or t_pos[b] + S - 1 > min(t_max, S_kv - 1).  Such a sequence reads nothing from the caches and gets
 * zeros in all of its O and ranges_out rows -- the padding slot of a serving batch, and the guard that keeps a wrong position inside the
 * buffers.  Nothing is clamped silently.
 * A row without a compressed token (t < l - 1) is handled inside the kernel: no compressed row is read, its group scores are zero, the
 * selector and the attention run as for any row -- the ranges of nsa_sel_decode_step at that token.
 * ONE launch or none.  Declined with NSA_ERR_INVALID and a message naming the limit: anything but bf16 / f16, Dk = Dv in {64, 128},
 * h <= 16, the default block geometry (l = 32, d = 16, l' = 64), 16-byte aligned operands, S <= 16, or a t_max beyond the unsplit forms
 * (more than 64 / 32 / 16 chunks of 64 compressed tokens at 16 waves / 8 waves / D = 128) -- the separate launches take a scalar
 * position only and cannot stand in.  DECODE_STEP = 0 and DECODE_UNFUSED = 1 decline as well; DECODE_ROWS does not apply.
 * Tuning switch "DECODE_LONG" (default 0): with 1 a t_max beyond the unsplit forms is not declined but runs the LONG-ROW form (form 3):
 * still one workgroup per row and one launch, no workspace; a wave keeps the logits of its first two chunks in registers and sweeps every
 * further chunk twice (records first, then -- with the row's log-sum-exp -- the same MFMAs on the same operands again), so ranges and O
 * are the bits of the other exact forms.  It holds rows of up to 128 chunks of 64 compressed tokens and 2048 selection blocks:
 * t_max <= 131,071.  Beyond that the call declines with a message naming that limit.  A shape inside the unsplit forms keeps form 0 / 1
 * whatever the switch says.
 * nsa_sel_decode_ragged_plan: *launches = 1 and *form = 0 / 1 (/ 3 with DECODE_LONG = 1), or *launches = 0 and *form = -1 for a declined
 * shape (status NSA_OK).
 * workspace: nsa_sel_decode_ragged_workspace() bytes (0 today: the launch keeps everything on chip); may be null.
 * Bits: with t_pos[b] = t0 for every b, ranges and O are those of nsa_sel_decode_rows(t0); the existing entry points are unchanged.
 * ------------------------------------------------------------------------------------- */
NSA_API size_t nsa_sel_decode_ragged_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype);
NSA_API int nsa_sel_decode_ragged(const void *Q, const void *K_cmp, const void *K, const void *V, const int32_t *csc_ptr,
                          const int32_t *csc_rows, const float *csc_vals, int32_t *ranges_out, void *O,
                          const int32_t *t_pos /* device, [B] */, int t_max /* host */, int B, int S, int G, int h, int Dk, int Dv,
                          int S_cmp, int S_sel, int S_kv, int l, int d, int l_sel, int n_top, int64_t kc_stride_b, int64_t kc_stride_g,
                          int64_t kc_stride_s, int64_t k_stride_b, int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_b,
                          int64_t v_stride_g, int64_t v_stride_s, int dtype, float scale, void *workspace, size_t workspace_bytes,
                          void *stream);
NSA_API int nsa_sel_decode_ragged_plan(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int S_kv, int n_top, int dtype,
                               int t_max, int *launches /* host */, int *form /* host */);

/* ---------------------------------------------------------------------------------------
 * The ragged-batch decode step of the selected branch over PAGED caches: nsa_sel_decode_ragged in every respect except where row (b,s,g)
 * finds its cache rows.  The caches are pools of fixed-size pages that a serving layer hands out as sequences grow and takes back when
 * they finish; a block table says which pool page holds which 1024 tokens of which sequence.
 *   page_tokens   tokens per page.  Only 1024 is built -- one scorer chunk (64 compressed rows at d = 16) and 16 selection blocks of
 *                 l' = 64, so a chunk of K_cmp, a gathered K/V block and a forced block each lie inside exactly one page and the table
 *                 costs one wave-uniform lookup per chunk.  Every other value is declined with a message that names it.
 *   K_pool, V_pool [n_pages, G, 1024, D]; Kc_pool [n_pages, G, 64, D].  Each with a page stride (k_stride_p ...), a group stride and a row
 *                 stride in elements.  Rules as for the ragged call's caches: strides in multiples of 8 elements, 16-byte aligned bases, V
 *                 rows contiguous (v_stride_s = Dv), K rows contiguous (k_stride_s = Dk) for the forced-block prefetch, else no prefetch.
 *                 A pool may be of any size (beyond 2 GiB too): page bases are formed in 64 bits, and the only 32-bit byte offsets are
 *                 those of a row inside one (page, group) plane -- 1024 rows of K / V, 64 of K_cmp -- which must stay under 2 GiB
 *                 (1024 * stride_s * 2 bytes; declined otherwise).
 *   block_table   device int32 [B, max_pages], table_stride elements between its rows (>= max_pages).  Entry j of sequence b is the pool
 *                 page that holds tokens [1024 j, 1024 j + 1024) of its K and V and compressed rows [64 j, 64 j + 64) of its K_cmp: one
 *                 page id indexes all three pools.  The host never reads the table, as it never reads t_pos.
 *   t_pos, t_max, S   as in nsa_sel_decode_ragged.  The capacity that call takes from S_kv is max_pages * 1024 here; S_cmp and S_sel are
 *                 the metadata bounds of min(t_max, capacity - 1) + 1 tokens.  max_pages <= 2^20.
 * Inactive sequences: the ragged call's rule -- t_pos[b] < 0, or t_pos[b] + S - 1 > min(t_max, capacity - 1) -- plus one case: any table
 * entry the sequence NEEDS lies outside [0, n_pages).  The entries it needs are j = 0 .. (t_pos[b] + S - 1) >> 10; entries behind them are
 * never read.  An inactive sequence gets zeros in all of its O and ranges_out rows and reads nothing from the pools: its workgroups check
 * the needed entries once, before their first cache read, and leave.  Nothing is clamped silently, and no table value can send an access
 * outside the pools: only entries inside [0, n_pages) are ever turned into an address.
 * ONE launch or none: the form and the waves per row are planned from t_max and B*S*G exactly as nsa_sel_decode_ragged plans them, with
 * the same declines and messages (dtype, Dk = Dv in {64, 128}, h <= 16, the default block geometry, S <= 16, a t_max beyond the unsplit
 * forms, DECODE_STEP = 0, DECODE_UNFUSED = 1), and in addition NSA_ERR_INVALID for page_tokens != 1024, a null table, max_pages < 1,
 * n_pages < 1, a table stride below max_pages, misaligned pools or strides, and row strides that leave the 32-bit in-plane offsets.
 * With the tuning switch DECODE_LONG = 1 a t_max beyond the unsplit forms runs the long-row form (form 3) as in nsa_sel_decode_ragged: rows
 * of up to 128 chunks (t_max <= 131,071: table entries 0 .. 127), the same bits as that call on contiguous caches.
 * nsa_sel_decode_paged_plan: *launches = 1 and *form = 0 / 1 (/ 3 with DECODE_LONG = 1), or *launches = 0 and *form = -1 for a declined shape or page size (status
 * NSA_OK).  workspace: nsa_sel_decode_paged_workspace() bytes (0 today); may be null.
 * Bits: for a table that scatters contiguous caches into pages, in any order, ranges and O are those of nsa_sel_decode_ragged on the
 * contiguous caches bit for bit -- the same form and waves, the same arithmetic on the same values in the same order.  The existing entry
 * points are unchanged: the paged form is a kernel instantiation of its own.
 * ------------------------------------------------------------------------------------- */
NSA_API size_t nsa_sel_decode_paged_workspace(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int n_top, int dtype);
NSA_API int nsa_sel_decode_paged(const void *Q, const void *Kc_pool, const void *K_pool, const void *V_pool,
                         const int32_t *block_table /* device, [B,max_pages] */, int64_t table_stride, int n_pages, int max_pages,
                         int page_tokens, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int32_t *ranges_out,
                         void *O, const int32_t *t_pos /* device, [B] */, int t_max /* host */, int B, int S, int G, int h, int Dk, int Dv,
                         int S_cmp, int S_sel, int l, int d, int l_sel, int n_top, int64_t kc_stride_p, int64_t kc_stride_g,
                         int64_t kc_stride_s, int64_t k_stride_p, int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_p,
                         int64_t v_stride_g, int64_t v_stride_s, int dtype, float scale, void *workspace, size_t workspace_bytes,
                         void *stream);
NSA_API int nsa_sel_decode_paged_plan(int B, int S, int G, int h, int Dk, int Dv, int S_cmp, int S_sel, int max_pages, int page_tokens,
                              int n_top, int dtype, int t_max, int *launches /* host */, int *form /* host */);

/* Band attention forward with per-sequence positions (the sliding and the compressed branch of a ragged decode step): nsa_band_attn_fwd
 * with t0 replaced by a device array.  Query row (b, t) sits at absolute position t_pos[b] + t; hi and lo follow from it by the formula
 * above.  t_max: host upper bound of t_pos[b] + S - 1 (the host never reads t_pos).  Route, split count and workspace are those of the
 * scalar call (they depend on B, S, G, h, D alone).  Inactive sequences -- t_pos[b] < 0, t_pos[b] + S - 1 > t_max, or a last row whose
 * unclamped hi exceeds S_kv (sliding: t_pos[b] + S - 1 > S_kv - 1) -- give zero rows and lse = -inf.  Both kernels take the array: MFMA
 * (bf16 / f16) and generic (fp32 and everything else it covers).  Forward only. */
NSA_API size_t nsa_band_attn_fwd_ragged_workspace(int B, int S, int G, int h, int Dk, int Dv, int dtype);
NSA_API int nsa_band_attn_fwd_ragged(const void *Q, const void *K, const void *V, void *O, float *lse,
                             const int32_t *t_pos /* device, [B] */, int t_max /* host */, int B, int S, int G, int h, int Dk, int Dv,
                             int S_kv, int64_t k_stride_b, int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_b,
                             int64_t v_stride_g, int64_t v_stride_s, int a, int dd, int c, int w, int dtype, float scale, int variant,
                             void *workspace, size_t workspace_bytes, void *stream);

/* nsa_band_attn_fwd_ragged over PAGED caches (the sliding and the compressed branch of a ragged decode step whose K_win / V_win or K_cmp /
 * V_cmp live in pools of pages): that call in every respect except where a key row is found.
 *   K_pool, V_pool  [n_pages, G, page_rows, D], each with a page, a group and a row stride in elements.  Page bases are formed in 64 bits,
 *                   so a pool may exceed 2 GiB; the only 32-bit byte offsets are inside one (page, group) plane: page_rows * stride_s * 2
 *                   bytes must stay under 2 GiB (declined otherwise).
 *   block_table     device int32 [B, max_pages], table_stride elements between its rows (>= max_pages).  Key row r of sequence b is row
 *                   r & (page_rows - 1) of pool page block_table[b, r >> log2(page_rows)].  The host never reads it.
 *   page_rows       a power of two in [32, 65536] (32 = the key tile: a tile touches at most two pages).  1024 for the sliding branch and
 *                   64 for the compressed one (d = 16) are the sizes at which one table -- nsa_sel_decode_paged's -- serves all five pools.
 *   Q, O, lse, t_pos, t_max, B, S, G, h, Dk, Dv, a, dd, c, w, dtype, scale   as in nsa_band_attn_fwd_ragged.  The capacity that call takes
 *                   from S_kv is max_pages * page_rows here.  max_pages <= 2^20.  There is no variant: one route.
 * Inactive sequences: the ragged call's rule with the capacity in the place of S_kv, plus one case: a table entry the sequence NEEDS lies
 * outside [0, n_pages).  The needed entries are those that cover key rows [lo_b, hi_b): hi_b the unclamped hi of the sequence's last query
 * row, lo_b = max(0, hi(first row) - w).  Entries below the sliding window and entries behind hi_b are never read and may hold anything.
 * The set is the sequence's, not a wave's: every wave of a sequence and every split of a row reaches the same verdict.  An inactive
 * sequence gives zero rows and lse = -inf and reads nothing from the pools.  Only entries that passed the test are turned into addresses;
 * nothing is clamped silently.
 * Route, split count and workspace are those of the scalar and the ragged call, planned from (B, S, G, h, D) alone; a missing or too small
 * workspace runs the unsplit form.  NSA_ERR_INVALID, with a message that names the limit and no fallback, for: anything outside the MFMA
 * kernels (fp32, Dk != Dv, D not 64 or 128, h > 16), w < 1, a null table or t_pos, max_pages outside [1, 2^20], n_pages < 1, a table stride
 * below max_pages, a page_rows that is not built, misaligned pools or strides (16-byte pools and Q, strides in multiples of 8 elements, O
 * 8-byte aligned), and row strides that leave the 32-bit in-plane offsets.
 * Bits: for a table that scatters contiguous caches into pages, in any order, O and lse are those of nsa_band_attn_fwd_ragged on the
 * contiguous caches bit for bit -- the same tiles of 32 keys, masks, split shares and epilogue.  Forward only. */
NSA_API size_t nsa_band_attn_fwd_paged_workspace(int B, int S, int G, int h, int Dk, int Dv, int dtype);
NSA_API int nsa_band_attn_fwd_paged(const void *Q, const void *K_pool, const void *V_pool,
                            const int32_t *block_table /* device, [B,max_pages] */, int64_t table_stride, int n_pages, int max_pages,
                            int page_rows, void *O, float *lse, const int32_t *t_pos /* device, [B] */, int t_max /* host */, int B, int S,
                            int G, int h, int Dk, int Dv, int64_t k_stride_p, int64_t k_stride_g, int64_t k_stride_s, int64_t v_stride_p,
                            int64_t v_stride_g, int64_t v_stride_s, int a, int dd, int c, int w, int dtype, float scale, void *workspace,
                            size_t workspace_bytes, void *stream);

/* indices [R,K] int32 ascending with -1 padding -> ranges [R,K,2]; clamp end to t+1. */
NSA_API int nsa_indices_to_ranges_v2(const int32_t *indices, int64_t R, int S, int G, int t0, int K, int S_sel,
                             int l_sel, int32_t *ranges_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NSA_SEL_HIP_H */
