// Internal forms of a few C-ABI entry points: same arguments plus the split-KV hand-over used by the fused decode step
// (defer != 0: the partial records stay in the workspace, *ns_used tells how many splits were written; 1 = O is final).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace nsa {

int sel_attn_fwd_impl(const void *Q, const void *K, const void *V, const int32_t *ranges, void *O, float *lse, int B, int S, int G, int h,
                      int Dk, int Dv, int S_kv, int n_ranges, int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb, int64_t vsg, int64_t vss,
                      int dtype, float scale, int variant, void *workspace, size_t workspace_bytes, void *stream, int defer, int *ns_used);
int band_attn_fwd_impl(const void *Q, const void *K, const void *V, void *O, float *lse, int B, int S, int G, int h, int Dk, int Dv, int S_kv,
                       int64_t ksb, int64_t ksg, int64_t kss, int64_t vsb, int64_t vsg, int64_t vss, int t0, int a, int dd, int c, int w,
                       int dtype, float scale, int variant, void *workspace, size_t workspace_bytes, void *stream, int defer, int *ns_used);
struct DecBandPair;    // sel_attn_params.hpp
struct SelDecodeCall;  // nsa_host.hpp: the arguments of nsa_sel_decode_step / nsa_sel_decode_rows (S tokens per sequence from t0 on; the step: S = 1)
// band / band_taken: the layer step's sliding + compressed branches (split form, deferred combine); *band_taken = 1 when the selected branch ran
// as the one-launch decode step and carried them on its launch (otherwise the caller launches them itself)
int sel_decode_step_impl(const SelDecodeCall &c, void *workspace, size_t workspace_bytes, void *stream, int defer, int *ns_used, float **part_used,
                         const DecBandPair *band = nullptr, int *band_taken = nullptr);
int sel_decode_rows_impl(const SelDecodeCall &c, void *workspace, size_t workspace_bytes, void *stream);

bool decode_score_select_supported(int dtype, int h, int Dk, int S_cmp, int S_sel, int64_t csb, int64_t csg, int64_t css, const void *Q,
                                   const void *Kc, int64_t rows);
struct DecAttnArgs;  // sel_attn_params.hpp: non-null = the row's selection attention runs in the same launch
int launch_decode_score_select(const void *Q, const void *Kc, int B, int G, int h, int Dk, int S_cmp, int64_t csb, int64_t csg, int64_t css,
                               const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int l_sel, int n_top,
                               int t_token, int dtype, float scale, int32_t *ranges_out, hipStream_t st, const DecAttnArgs *attend,
                               int stencil);
// the one-launch decode step (sel_decode_fused.hip): default block geometry, bf16 / f16, Dk = Dv = 64 or 128
bool decode_step_supported(const SelDecodeCall &c);
size_t decode_step_workspace(int64_t R, int h, int S_cmp);
int launch_decode_step(const SelDecodeCall &c, void *ws, size_t ws_bytes, hipStream_t st, const DecBandPair *band = nullptr);
// shape / tuning part of decode_step_supported (default block geometry; the tensors are not read): false = declined (form -1, nsplit 0)
bool decode_step_shape_plan(const SelDecodeCall &c, int *form, int *nsplit);
// rows form of the one-launch step (nsa_sel_decode_rows): S consecutive tokens per sequence at t0 .. t0 + S - 1, one workgroup per row
bool decode_rows_shape_plan(const SelDecodeCall &c, int *form, int *nw_out);
bool decode_rows_supported(const SelDecodeCall &c);
int launch_decode_rows(const SelDecodeCall &c, hipStream_t st);
// shape / tuning part of decode_score_select_supported
bool decode_score_select_shape_ok(int dtype, int h, int Dk, int S_cmp, int S_sel, int64_t rows);

// ---- launchers the C ABI dispatches to; every translation unit that defines one includes this header, so a definition whose return type or
// default arguments disagree does not compile (a changed parameter list still declares an overload and fails at link time).
// The default arguments (q0 / norm / l / d: prefill rows, normalised over all S_cmp columns) live here only.
// sel_select.hip
int launch_select_topn(const float *p_grp, int64_t R, int S, int G, int t0, const int32_t *t_rows, int S_sel, int l_sel, int n_top,
                       int force_init, int force_local, int mode, int S_total, int32_t *out, int W, hipStream_t st);
int launch_indices_to_ranges(const int32_t *idx, int64_t R, int S, int G, int t0, int K, int S_sel, int l_sel, int32_t *out, hipStream_t st);
int batched_width(int S, int S_sel, int l_sel, int n_top, int force_init, int force_local);
// sel_scores.hip
int launch_map_pcmp(const float *p_cmp, int64_t R, int h, int S_cmp_cur, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals,
                    int S_sel, float *p_slc, float *p_grp, hipStream_t st);
int launch_pcmp(const void *Q, const void *Kc, float *p_cmp, int64_t row0, int64_t nrows, int S, int G, int h, int Dk, int S_cmp, int64_t csb,
                int64_t csg, int64_t css, int dtype, float scale, hipStream_t st, int q0 = 0, int norm = 0, int l = 1, int d = 1);
size_t scores_workspace(int64_t R, int h, int S_cmp);
int launch_sel_scores(const void *Q, const void *Kc, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp, int64_t csb, int64_t csg,
                      int64_t css, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int dtype, float scale,
                      void *ws, size_t ws_bytes, hipStream_t st, int q0 = 0, int norm = 0, int l = 1, int d = 1);
constexpr int64_t DECODE_MAX_ROWS = 1024;  // rows (B*S*G) up to which the decode-shaped scorer is used
size_t decode_scores_workspace(int64_t R, int h, int S_cmp);
int launch_decode_scores(const void *Q, const void *Kc, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp, int64_t csb, int64_t csg,
                         int64_t css, const int32_t *csc_ptr, const int32_t *csc_rows, const float *csc_vals, int S_sel, int dtype, float scale,
                         void *ws, size_t ws_bytes, hipStream_t st, int q0 = 0, int norm = 0, int l = 1, int d = 1);
// sel_scores_mfma.hip
struct SelectParams;  // sel_select_row.hpp
bool scores_mfma_supported(int dtype, int h, int Dk, int l, int d, int l_sel);
int launch_sel_scores_mfma(const void *Q, const void *Kc, float *p_grp, int B, int S, int G, int h, int Dk, int S_cmp, int64_t csb, int64_t csg,
                           int64_t css, int S_sel, int d_stride, int dtype, float scale, int causal_skip, hipStream_t st, const SelectParams *sel,
                           int *sel_done, int q0 = 0, int norm = 0, int l = 1);
// sel_attn_generic.hip
int launch_sel_first_key(const void *V, const int32_t *ranges, void *O, int64_t R, int S, int G, int h, int Dv, int n, int S_kv, int64_t vsb,
                         int64_t vsg, int64_t vss, int esz, hipStream_t st);

}  // namespace nsa
