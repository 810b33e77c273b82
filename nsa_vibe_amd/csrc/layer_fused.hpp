// Argument blocks + launchers of the layer-level kernels (layer_fused.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nsa {

struct RopeAppendParams {
    const void *proj;  // [B*S, NQ + 3 G Dk + 3 G Dv]: Q | K_sel | V_sel | K_win | V_win | K_raw | V_raw
    void *Q_out;       // [B*S, NQ]
    void *cache[6];    // K_sel, V_sel, K_win, V_win, K_raw, V_raw: [B,G,S_max,D] contiguous
    int B, S, G, h, Dk, Dv, S_max, t0;
    float rope_base, inv_scale;
    // ragged form of the rows epilogue (nsa_layer_decode_ragged): device [B] positions or null; with it row (b, s) is rotated at and
    // appended to position t_pos[b] + s (t0 = 0), and a sequence with t_pos[b] < 0 or t_pos[b] + S - 1 > min(t_max, S_max - 1) writes
    // NO cache row (rope_seq); Q_out is written for every row
    const int32_t *t_pos;
    int t_max;
};
struct CmpPoolParams {
    const void *K_raw, *V_raw;  // [nbg, S_max, D]
    void *K_cmp, *V_cmp;        // [nbg, n_cmp_max, D]
    int nbg, S_max, n_cmp_max, Dk, Dv, l, d, j0, j1;
    float rope_base, inv_scale;
    // ragged form (launch_cmp_pool_ragged): device [nbg / G] positions; sequence b emits the tokens whose windows complete inside its S
    // rows t_pos[b] .. t_pos[b] + S - 1 (j0 / j1 unused), a sequence that is not live (as above) none
    const int32_t *t_pos;
    int t_max, S, G;
};
// ---- paged caches (nsa_layer_decode_paged): the eight cache tensors are pools [n_pages, G, 1024 | 64, D] found through a device block table.
// One table block, and the two writers' argument blocks with it at their end -- the PAGED instantiations alone take these; RopeAppendParams,
// CmpPoolParams and every other instantiation keep their layout.  Entry [b, j] of the table is the pool page of tokens [1024 j, 1024 j + 1024)
// and compressed rows [64 j, 64 j + 64) of sequence b.  A kernel forms an address only from an entry it has itself tested against [0, n_pages).
constexpr int LAYER_PAGE_TOKENS = 1024, LAYER_PAGE_CMP = 64;
struct LayerPageTable {
    const int32_t *table;  // device [B, max_pages] int32
    int64_t stride;        // elements between its rows
    int n_pages, max_pages;
};
// cache[]: the six token pools; S_max: the capacity max_pages * 1024; t_pos: the verdicts t_live of the pre-pass; t0 = 0
struct RopePagedParams : RopeAppendParams {
    LayerPageTable pg;
};
// K_raw / V_raw / K_cmp / V_cmp: the pools; S_max: the capacity; n_cmp_max = max_pages * 64; t_pos: t_live
struct CmpPoolPagedParams : CmpPoolParams {
    LayerPageTable pg;
};
// the pre-pass: one wave per sequence writes its verdict t_live[b] = t_pos[b] where the sequence is live -- 0 <= t_pos[b],
// t_pos[b] + S - 1 <= te, every table entry j = 0 .. (t_pos[b] + S - 1) >> 10 inside [0, n_pages) -- and -1 otherwise
struct PagedLiveParams {
    const int32_t *t_pos;
    int32_t *t_live;
    LayerPageTable pg;
    int B, S, te;
};
struct GateCombineParams {
    const void *Q, *O_cmp, *O_sel, *O_win;
    void *O_out;
    float *gates_out;  // [R,3] or null
    const void *w1, *b1, *w2, *b2;
    int64_t R;
    int h, Dk, Dv, Hd;
    float tau;
};
struct DecodeFinishParams {
    const void *Q;
    const float *part[3];  // cmp, sel, win: split-KV partial records (ns > 1) ...
    const void *O[3];      // ... or the final branch output (ns == 1)
    int ns[3];
    void *O_out;
    float *gates_out;
    const void *w1, *b1, *w2, *b2;
    int64_t R;
    int h, Dk, Dv, Hd;
    float tau;
};
// One few-row projection out [M,N] = A [M,K] . W [N,K]^T: what nsa_linear_small and the layer calls hand to every launcher of the family
// (layer_fused.hip).  Filled once by aggregate initialisation: the fields after `st` are optional groups and stay zero when left out.
struct LinearCall {
    const void *A, *W;
    void *out;
    int M, N, K, dtype;
    int epi;  // 0 none, 1 silu, 2 + res[M,N]
    const void *res;
    hipStream_t st;
    const void *norm_w;  // RMSNorm(A) with these weights and eps folded into the projection (a route with fold_norm only)
    float eps;
    const void *Os, *Ow;  // the mix (launch_linear_small_mix): A = O_cmp, these O_sel and O_win, the row gates [M G][3]
    const float *gates;
    int G;
};
// What runs a LinearCall under an epilogue kind -- the family's one route decision (proj_route): the MFMA kernel with 4 or 8 waves, the
// all-loads-first VALU form with nc chunks in flight, or the chunk loop; cw = weight rows per wave of the VALU forms.
enum ProjKind { PROJ_PLAIN, PROJ_ROPE, PROJ_ROPE_ROWS, PROJ_MIX };
enum ProjForm { PROJ_NONE, PROJ_MFMA, PROJ_FAST, PROJ_LOOP };  // PROJ_NONE: a mix the projection does not take
struct ProjRoute {
    ProjForm form;
    int waves, nc, cw;
    dim3 grid;
    bool fold_norm;  // the form takes c.norm_w (the MFMA kernel reads normalised rows)
};
ProjRoute proj_route(const LinearCall &c, ProjKind kind);
// epilogue of the fused QKV projection: every column pair rotated and appended at its row's position.  rows: P.S (1 to 16) consecutive
// tokens per sequence, row b P.S + s of c.A at position P.t0 + s (the layer's rows call; false: P.S = 1, the single step); with P.t_pos the
// rows form's ragged instantiations (position P.t_pos[b] + s, cache stores predicated on the sequence being live)
int launch_qkv_rope_append(const RopeAppendParams &P, const LinearCall &c, bool rows);
int launch_linear_small_epi(const LinearCall &c);
// c.norm_w set: one launch where the route folds the norm, else RMSNorm(A) into scratch [M,K] and the projection from there
int launch_linear_normed(const LinearCall &c, void *scratch);
int launch_decode_finish(const DecodeFinishParams &P, int dtype, hipStream_t st);
// output projection of a decode step fed by the three branch outputs and the row gates: out = mix(O_cmp, O_sel, O_win) . W^T
inline bool linear_small_mix_supported(const LinearCall &c) { return proj_route(c, PROJ_MIX).form != PROJ_NONE; }
int launch_linear_small_mix(const LinearCall &c);
int launch_embed_rows(const int32_t *tokens, const void *embed, void *x, int B, int dim, int vocab, int dtype, hipStream_t st);
size_t argmax_rows_workspace(int B, int vocab);
int launch_argmax_rows(const void *logits, int32_t *next, int B, int vocab, int dtype, void *ws, hipStream_t st);
int launch_rmsnorm_rows(const void *x, const void *w, void *y, int M, int dim, float eps, int dtype, hipStream_t st);
size_t rmsnorm_rows_bwd_workspace(int M, int dim);
int launch_rmsnorm_rows_bwd(const void *x, const void *w, const void *dy, void *dx, void *dw, int M, int dim, float eps, int dtype,
                            void *workspace, size_t workspace_bytes, hipStream_t st);
int launch_rope_cache_append(const RopeAppendParams &P, int dtype, hipStream_t st);
int launch_cmp_pool(const CmpPoolParams &P, int dtype, hipStream_t st);
// per-sequence positions (P.t_pos): nbg ceil(S / d) blocks of the wide form, launched whether or not a window completes (the host never
// reads the positions); block (bg, k) takes token n_cmp(t_pos[b]) + k and leaves where its sequence does not emit it
int launch_cmp_pool_ragged(const CmpPoolParams &P, int dtype, hipStream_t st);
// the paged call's three launches of this file: the verdicts, the rows epilogue's PAGED instantiations (row (b, s) at pos = t_live[b] + s
// goes to row pos & 1023 of page table[b][pos >> 10] of each token pool) and the wide pooling kernel's (window rows and the compressed
// row each found through their own page)
int launch_paged_live(const PagedLiveParams &P, hipStream_t st);
int launch_qkv_rope_append_paged(const RopePagedParams &P, const LinearCall &c);
int launch_cmp_pool_paged(const CmpPoolPagedParams &P, int dtype, hipStream_t st);
int launch_rope_cache_append_bwd(const RopeAppendParams &P, int dtype, hipStream_t st);
int launch_cmp_pool_bwd(const CmpPoolParams &P, const void *dKc, const void *dVc, void *dKr, void *dVr, int S, int n_cmp, int dtype,
                        hipStream_t st);
int launch_gate_combine(const GateCombineParams &P, int dtype, hipStream_t st);
int launch_gate_combine_bwd(const GateCombineParams &P, const void *dO, const float *gates, void *dOc, void *dOs, void *dOw, float *dgates,
                            int dtype, hipStream_t st);

}  // namespace nsa
