// Kernel argument blocks of the scorer and selector kernels (sel_scores.hip, sel_scores_mfma.hip, sel_scores_mfma32.hip, sel_select.hip and
// the decode kernels that select in their launch).  No device code: dispatch_check.cpp reads the blocks of a refused launch through them.
#pragma once
#include <stdint.h>

namespace nsa {

// Eq.9 + Eq.10 (map_pcmp_kernel): p_cmp [R,h,S_cmp_cur] -> p_slc [R,h,S_sel] (or null), p_grp [R,S_sel]
struct MapParams {
    const float *p_cmp;
    const int32_t *csc_ptr, *csc_rows;
    const float *csc_vals;
    float *p_slc, *p_grp;
    int64_t R;
    int h, S_cmp_cur, S_sel;
};

struct PcmpParams {
    const void *Q;   // [R,h,Dk]
    const void *Kc;  // [B,G,S_cmp,Dk] strided
    float *p_cmp;    // [Rchunk,h,S_cmp]
    int64_t row0, nrows;  // rows [row0,row0+nrows) of the full R = B*S*G
    int S, G, h, Dk, S_cmp;
    int64_t csb, csg, css;
    float scale;
    int q0, norm, l, d;  // norm = 1: row (b,s,g) at token q0 + s normalises over its own n_cmp(q0 + s) columns, the rest are written as 0
};

struct DecodeParams {
    const void *Q;   // [R,h,Dk]
    const void *Kc;  // strided
    float *x;        // [R,h,S_cmp] logits * scale * log2(e)
    float *part;     // [R,h,nchunk,2] per 64-row chunk: max, sum exp2(x - max)
    float *p_grp;    // [R,S_sel]
    const int32_t *csc_ptr, *csc_rows;
    const float *csc_vals;
    int64_t R;
    int S, G, h, Dk, S_cmp, S_sel;
    int64_t csb, csg, css;
    float c2;
    int stencil;  // fused decode kernel: l = 2d and l' = 4d, Eq.9 is the closed-form 5-tap stencil (no CSC loads)
    int q0, norm, l, d;  // norm = 1 (two-kernel route only): row (b,s,g) at token q0 + s sees its own n_cmp(q0 + s) columns
};

// the fused MFMA scorers (sel_scores_mfma.hip: 16x16x32 tiles, every group size; sel_scores_mfma32.hip: 32x32x16 tiles, h = 6 and D = 64)
struct ScoresMfmaParams {
    const void *Q;   // [B,S,G,h,D]
    const void *Kc;  // [B,G,S_cmp,D] strided
    float *p_grp;    // [B,S,G,S_sel]
    int B, S, G, h, S_cmp, S_sel;
    int64_t csb, csg, css;
    float scale;
    int causal_skip;
    int d_stride;  // the compression stride d (tokens); l' = 4d
    int big_out;   // S G S_sel >= 2^31 elements per sequence: 64-bit output offsets
    int q0;        // absolute position of query row 0 (a chunk of a chunked prefill starts at q0 > 0)
    int norm;      // 1: row t = q0 + s normalises over its own n_cmp(t) columns (decode semantics); 0: over all S_cmp
    int l;         // compression window (tokens): n_cmp(t) = (t + 1 < l) ? 0 : (t + 1 - l) / d + 1
};

struct SelectParams {
    const float *p_grp;     // [R,S_sel]
    const int32_t *t_rows;  // [R] or null
    int32_t *out;           // [R,W,2]
    int64_t R;
    int S, G, t0, S_sel, l_sel, n_top, force_init, force_local, mode, W;
    int k_actual;      // picks per row
    int n_forced;      // forced entries used (sequential: all; batched: kept columns, maybe truncated)
    unsigned keepmask; // batched: bit i = sorted forced column i is kept
    int all_valid;     // batched with n_top >= S_sel: select every valid block
    int l_sel_shift;   // log2(l_sel) when l_sel is a power of two, else -1 (the block of a token without an integer division)
    int forced_plain;  // batched: every forced column is kept and used (S > 2 l'), the forced set is {0} + (cblk - force_local, cblk]
};

}  // namespace nsa
