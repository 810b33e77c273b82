/*
 * nsa_oracle.c -- CPU restatement of nsa-vibe's selected-branch attention hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under nsa_vibe_amd/ (the product) may import,
 * link or call this file.  Allowed users: tests/, __graft_entry__.smoke(), and the
 * `cpu_baseline` leg of bench.py -- and there only as the checker / reported CPU
 * baseline, never as the thing shipped.
 *
 * Parity status: PINNED.  oracle/make_goldens.py imports the reference
 * (/root/reference, Python) in the build container, runs the reference functions
 * cited below on seeded inputs and stores inputs+outputs under tests/golden/;
 * tests/test_oracle_golden.py checks this file against those vectors
 * (bit-exact for integer ranges and for the Eq.9/Eq.10 fp32 chain, 1e-6 for the
 * softmax scores, 1e-5 for attention outputs).
 *
 * All arithmetic is IEEE fp32 with separate multiply/add (compile with
 * -ffp-contract=off); every function cites the reference file:line it follows.
 * Paths are relative to the reference repo root.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define NSA_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------- */
/* A1: block starts + fractional-overlap CSR  (nsa/core/block_index.py:25-71) */
/* ------------------------------------------------------------------------- */

/* nsa/core/block_index.py:25-36 */
NSA_API int nsa_oracle_block_counts(int seq_len, int l, int d, int l_sel, int *S_cmp, int *S_sel) {
    if (d <= 0 || l <= 0 || l_sel <= 0) return -1;
    *S_cmp = (seq_len < l) ? 0 : (seq_len - l) / d + 1;
    *S_sel = (seq_len <= 0) ? 0 : (seq_len + l_sel - 1) / l_sel;
    return 0;
}

static int overlap_len(int a0, int a1, int b0, int b1) { /* block_index.py:39-40 */
    int lo = a0 > b0 ? a0 : b0;
    int hi = a1 < b1 ? a1 : b1;
    return hi > lo ? hi - lo : 0;
}

/*
 * nsa/core/block_index.py:43-71 (build_M_csl_csr).  indptr has S_cmp+1 entries,
 * indices/values must hold at least nsa_oracle_csr_nnz() entries.  Weights are
 * ov/total computed in double and rounded once to fp32, as torch.tensor(list of
 * python floats, dtype=float32) does.  Returns nnz.
 */
NSA_API int nsa_oracle_build_csr(int seq_len, int l, int d, int l_sel, int32_t *indptr,
                                 int32_t *indices, float *values) {
    int S_cmp, S_sel;
    if (nsa_oracle_block_counts(seq_len, l, d, l_sel, &S_cmp, &S_sel)) return -1;
    int nnz = 0;
    indptr[0] = 0;
    for (int i = 0; i < S_cmp; ++i) {
        int a0 = i * d, a1 = i * d + l;
        int total = 0;
        /* only selection blocks that can overlap [a0,a1) */
        int j0 = a0 / l_sel, j1 = (a1 - 1) / l_sel;
        if (j1 >= S_sel) j1 = S_sel - 1;
        for (int j = j0; j <= j1; ++j) total += overlap_len(a0, a1, j * l_sel, j * l_sel + l_sel);
        if (total > 0) {
            for (int j = j0; j <= j1; ++j) {
                int ov = overlap_len(a0, a1, j * l_sel, j * l_sel + l_sel);
                if (ov > 0) {
                    if (indices) {
                        indices[nnz] = j;
                        values[nnz] = (float)((double)ov / (double)total);
                    }
                    ++nnz;
                }
            }
        }
        indptr[i + 1] = nnz;
    }
    return nnz;
}

/* ------------------------------------------------------------------------- */
/* A2: p_cmp = softmax_c(Q K_cmp^T * scale)  (nsa/core/selection_scorer.py:42-61) */
/*   Q [B,S,G,h,Dk] contiguous; K_cmp [B,G,S_cmp,Dk]; out [B,S,G,h,S_cmp].      */
/*   Softmax over ALL S_cmp columns (no causal mask), as the reference does.     */
/* ------------------------------------------------------------------------- */
NSA_API int nsa_oracle_pcmp_all(const float *Q, const float *Kc, float *P, int B, int S, int G,
                                int h, int Dk, int S_cmp, float scale) {
    if (S_cmp == 0) return 0;
    long rows = (long)B * S * G * h;
#pragma omp parallel for schedule(static)
    for (long r = 0; r < rows; ++r) {
        long hh = r % h;
        long g = (r / h) % G;
        long s = (r / ((long)h * G)) % S;
        long b = r / ((long)h * G * S);
        (void)hh;
        (void)s;
        const float *q = Q + r * Dk;
        const float *k = Kc + ((b * G + g) * (long)S_cmp) * Dk;
        float *p = P + r * (long)S_cmp;
        float m = -INFINITY;
        for (int c = 0; c < S_cmp; ++c) {
            float acc = 0.f;
            for (int e = 0; e < Dk; ++e) acc += q[e] * k[(long)c * Dk + e];
            acc = acc * scale;
            p[c] = acc;
            if (acc > m) m = acc;
        }
        float sum = 0.f;
        for (int c = 0; c < S_cmp; ++c) {
            p[c] = expf(p[c] - m);
            sum += p[c];
        }
        for (int c = 0; c < S_cmp; ++c) p[c] = p[c] / sum;
    }
    return 0;
}

/* ------------------------------------------------------------------------- */
/* A3+A4: Eq.9 COO scatter-add + Eq.10 head sum                               */
/*   (nsa/core/selection_scorer.py:89-116; nsa/core/nsa_attention.py:670,1091) */
/*   p_cmp [R,h,S_cmp_cur] -> p_slc [R,h,S_sel] (optional) -> p_grp [R,S_sel]   */
/*   COO entries in CSR order (ascending cmp row); rows >= S_cmp_cur dropped    */
/*   (selection_scorer.py:103-108).  Accumulation order = the CPU scatter_add   */
/*   order: ascending nnz; product rounded before the add; head sum ascending h.*/
/* ------------------------------------------------------------------------- */
NSA_API int nsa_oracle_map_pcmp_to_pgrp(const float *p_cmp, long R, int h, int S_cmp_cur,
                                        const int32_t *indptr, const int32_t *indices,
                                        const float *values, int S_cmp_meta, int S_sel,
                                        float *p_slc /* nullable */, float *p_grp) {
    int rmax = S_cmp_cur < S_cmp_meta ? S_cmp_cur : S_cmp_meta;
#pragma omp parallel
    {
        float *tmp = (float *)malloc(sizeof(float) * (size_t)S_sel);
#pragma omp for schedule(static)
        for (long r = 0; r < R; ++r) {
            float *grp = p_grp + r * (long)S_sel;
            for (int j = 0; j < S_sel; ++j) grp[j] = 0.f;
            for (int hh = 0; hh < h; ++hh) {
                const float *pc = p_cmp + (r * h + hh) * (long)S_cmp_cur;
                float *dst = p_slc ? p_slc + (r * h + hh) * (long)S_sel : tmp;
                for (int j = 0; j < S_sel; ++j) dst[j] = 0.f;
                for (int i = 0; i < rmax; ++i) {
                    for (int k = indptr[i]; k < indptr[i + 1]; ++k) {
                        volatile float prod = pc[i] * values[k];
                        dst[indices[k]] = dst[indices[k]] + prod;
                    }
                }
                for (int j = 0; j < S_sel; ++j) grp[j] = grp[j] + dst[j];
            }
        }
        free(tmp);
    }
    return 0;
}

/* ------------------------------------------------------------------------- */
/* top-k helper: composite key (selection_scorer.py:182-187, 312-321)          */
/*   composite = fp32(masked) - fp32(idx) * 1e-8f (unfused);                    */
/*   order = composite descending, index ascending on exact ties (PRD.md:46,    */
/*   the documented intent; torch.topk leaves exact ties unspecified).          */
/* ------------------------------------------------------------------------- */
static inline float composite_key(float masked, int idx) {
    volatile float bias = (float)idx * 1e-8f;
    volatile float c = masked - bias;
    return c;
}

/* pick k best of n by (key desc, idx asc); -inf keys are never picked.  out_idx
 * receives the picks in rank order; returns how many were picked (<= k).      */
static int topk_pick(const float *key, int n, int k, int *out_idx) {
    int got = 0;
    char *used = (char *)calloc((size_t)n, 1);
    for (int r = 0; r < k; ++r) {
        int best = -1;
        float bk = -INFINITY;
        for (int i = 0; i < n; ++i) {
            if (used[i]) continue;
            if (key[i] > bk) {
                bk = key[i];
                best = i;
            }
        }
        if (best < 0) break; /* only -inf left */
        used[best] = 1;
        out_idx[got++] = best;
    }
    free(used);
    return got;
}

static int cmp_int(const void *a, const void *b) {
    int x = *(const int *)a, y = *(const int *)b;
    return (x > y) - (x < y);
}

/* ------------------------------------------------------------------------- */
/* A5: select_topn_ranges -- decode / sequential mode                          */
/*   (nsa/core/selection_scorer.py:124-249)                                     */
/*   p_grp [R,S_sel] (R = B*G rows at one token position t, or any list of rows */
/*   with per-row t in t_tokens).  Output [R,n_top,2] int32, zero padded.       */
/*   Normalisation (SURVEY 7 hard part (c)): when fewer than k_rest valid       */
/*   non-forced candidates exist the reference's topk picks -inf entries in an  */
/*   unspecified order and emits inverted ranges (start > end) for them; this   */
/*   restatement emits nothing for such picks.  Compare on {(s,e): e > s}.      */
/* ------------------------------------------------------------------------- */
NSA_API int nsa_oracle_select_topn_seq(const float *p_grp, long R, int S_sel, int l_sel,
                                       int n_top, const int32_t *t_tokens, int force_init,
                                       int force_local, int32_t *ranges) {
#pragma omp parallel
    {
        float *key = (float *)malloc(sizeof(float) * (size_t)(S_sel > 0 ? S_sel : 1));
        int *sel = (int *)malloc(sizeof(int) * (size_t)(n_top + force_local + 2 + S_sel));
#pragma omp for schedule(static)
        for (long r = 0; r < R; ++r) {
            int t = t_tokens[r];
            int32_t *out = ranges + r * (long)n_top * 2;
            memset(out, 0, sizeof(int32_t) * (size_t)n_top * 2);
            const float *p = p_grp + r * (long)S_sel;
            /* :156 valid_j <=> start_j + l_sel - 1 <= t */
            for (int j = 0; j < S_sel; ++j) {
                int valid = (j * l_sel + l_sel - 1) <= t;
                key[j] = valid ? composite_key(p[j], j) : -INFINITY;
            }
            /* :159-170 forced list, NOT deduplicated */
            int nf = 0;
            if (force_init) sel[nf++] = 0;
            int last_block = t / l_sel;
            if (last_block < 0) last_block = 0;
            for (int i = 0; i < force_local; ++i) {
                int f = last_block - i;
                if (f < 0) f = 0;
                sel[nf++] = f;
            }
            /* :172-175 forced -> -inf (scatter_ requires the index in range) */
            for (int i = 0; i < nf; ++i)
                if (sel[i] < S_sel) key[sel[i]] = -INFINITY;
            int k_rest = n_top - nf;
            if (k_rest < 0) k_rest = 0;
            int ns = nf;
            if (k_rest > 0) {
                int k_actual = k_rest < S_sel ? k_rest : S_sel; /* :186 */
                ns += topk_pick(key, S_sel, k_actual, sel + nf);
            }
            qsort(sel, (size_t)ns, sizeof(int), cmp_int); /* :211 */
            /* :221-248 unique_consecutive on block starts, merge adjacent, clamp */
            int m = 0;
            int have = 0, cur_s = 0, cur_e = 0, prev = -1;
            for (int i = 0; i < ns; ++i) {
                int blk = sel[i];
                if (have && blk == prev) continue;
                prev = blk;
                int x = blk * l_sel;
                if (!have) {
                    cur_s = x;
                    cur_e = x + l_sel;
                    have = 1;
                } else if (x == cur_e) {
                    cur_e += l_sel;
                } else {
                    if (m < n_top) {
                        int e = cur_e < t + 1 ? cur_e : t + 1;
                        out[2 * m] = cur_s;
                        out[2 * m + 1] = e;
                    }
                    ++m;
                    cur_s = x;
                    cur_e = x + l_sel;
                }
            }
            if (have && m < n_top) {
                int e = cur_e < t + 1 ? cur_e : t + 1;
                out[2 * m] = cur_s;
                out[2 * m + 1] = e;
            }
        }
        free(key);
        free(sel);
    }
    return 0;
}

/* ------------------------------------------------------------------------- */
/* A6: number of forced columns the batched selector keeps                     */
/*   (selection_scorer.py:283-300): forced = sort([0, c, c-1,...]) per row then  */
/*   unique_consecutive(dim=-1) over WHOLE columns [B,S,G]: a column is dropped  */
/*   only if it equals the previous column for every row t in [0,S).            */
/*   Writes the kept column ids (into the sorted per-row forced list) to keep[]. */
/* ------------------------------------------------------------------------- */
static void forced_row_sorted(int t, int l_sel, int force_init, int force_local, int *f, int *nf) {
    int n = 0;
    if (force_init) f[n++] = 0;
    int last_block = t / l_sel;
    for (int k = 0; k < force_local; ++k) {
        int v = last_block - k;
        if (v < 0) v = 0;
        f[n++] = v;
    }
    qsort(f, (size_t)n, sizeof(int), cmp_int);
    *nf = n;
}

NSA_API int nsa_oracle_batched_forced_columns(int S, int l_sel, int force_init, int force_local,
                                              int *keep /* size force_init+force_local */) {
    int nfmax = (force_init ? 1 : 0) + (force_local > 0 ? force_local : 0);
    if (nfmax == 0) return 0;
    int nk = 0;
    int *fa = (int *)malloc(sizeof(int) * (size_t)nfmax);
    for (int c = 0; c < nfmax; ++c) {
        if (c == 0) {
            keep[nk++] = 0;
            continue;
        }
        int same = 1;
        for (int t = 0; t < S && same; ++t) {
            int nf;
            forced_row_sorted(t, l_sel, force_init, force_local, fa, &nf);
            if (fa[c] != fa[c - 1]) same = 0;
        }
        if (!same) keep[nk++] = c;
    }
    free(fa);
    return nk;
}

/* ------------------------------------------------------------------------- */
/* A6+A7: select_topn_ranges_batched + convert_indices_to_ranges_batched_v2     */
/*   (nsa/core/selection_scorer.py:255-362, 434-605)                            */
/*   p_grp_all [B,S,G,S_sel] -> ranges [B,S,G,K,2]; K returned via *K_out.      */
/*   If ranges == NULL only K is computed.                                      */
/* ------------------------------------------------------------------------- */
NSA_API int nsa_oracle_select_topn_batched(const float *p_grp_all, int B, int S, int G, int S_sel,
                                           int l_sel, int n_top, int force_init, int force_local,
                                           int32_t *ranges, int *K_out) {
    int nfmax = (force_init ? 1 : 0) + (force_local > 0 ? force_local : 0);
    int *keep = (int *)malloc(sizeof(int) * (size_t)(nfmax + 1));
    int nfc = nsa_oracle_batched_forced_columns(S, l_sel, force_init, force_local, keep);
    int k_rest = n_top - nfc;
    if (k_rest < 0) k_rest = 0;
    int k_actual = k_rest < S_sel ? k_rest : S_sel;
    int K;
    if (n_top >= S_sel) K = S_sel;                 /* :353-354 replaces selected by all_idx */
    else if (k_rest > 0) K = nfc + k_actual;       /* :339 */
    else K = nfc < n_top ? nfc : n_top;            /* :341 */
    *K_out = K;
    if (!ranges) {
        free(keep);
        return 0;
    }
    long R = (long)B * S * G;
#pragma omp parallel
    {
        float *key = (float *)malloc(sizeof(float) * (size_t)(S_sel > 0 ? S_sel : 1));
        int *sel = (int *)malloc(sizeof(int) * (size_t)(K + nfmax + 2));
        int *fa = (int *)malloc(sizeof(int) * (size_t)(nfmax + 1));
#pragma omp for schedule(static)
        for (long r = 0; r < R; ++r) {
            int t = (int)((r / G) % S);
            const float *p = p_grp_all + r * (long)S_sel;
            int32_t *out = ranges + r * (long)K * 2;
            memset(out, 0, sizeof(int32_t) * (size_t)K * 2);
            int ns = 0;
            if (n_top >= S_sel) {
                /* :349-354 all valid blocks: prefix of length num_valid(t) */
                for (int j = 0; j < S_sel; ++j)
                    if ((j + 1) * l_sel <= t + 1) sel[ns++] = j;
            } else {
                int nf;
                forced_row_sorted(t, l_sel, force_init, force_local, fa, &nf);
                /* :276-280 valid <=> block end <= t+1 */
                for (int j = 0; j < S_sel; ++j) {
                    int valid = (j + 1) * l_sel <= t + 1;
                    key[j] = valid ? composite_key(p[j], j) : -INFINITY;
                }
                int nfk = 0;
                for (int c = 0; c < nfc; ++c) {
                    int f = fa[keep[c]];
                    if (f < S_sel) key[f] = -INFINITY; /* :302-305 */
                    sel[nfk++] = f;
                }
                ns = nfk;
                if (k_rest > 0) {
                    ns += topk_pick(key, S_sel, k_actual, sel + nfk);
                } else if (ns > n_top) {
                    ns = n_top; /* :341 */
                }
                /* :344-347 keep only valid picks (forced current partial block dropped) */
                int w = 0;
                for (int i = 0; i < ns; ++i)
                    if (sel[i] >= 0 && sel[i] < S_sel && (sel[i] + 1) * l_sel <= t + 1)
                        sel[w++] = sel[i];
                ns = w;
            }
            qsort(sel, (size_t)ns, sizeof(int), cmp_int); /* :355 */
            /* v2 converter :466-474 runs where diff in {0,1}; :534-539 end = max id;
             * :569-573 clamp end to t+1; packed to the front */
            int m = 0;
            int i = 0;
            while (i < ns) {
                int first = sel[i], last = sel[i];
                int j = i + 1;
                while (j < ns && (sel[j] - sel[j - 1] == 0 || sel[j] - sel[j - 1] == 1)) {
                    last = sel[j];
                    ++j;
                }
                int s0 = first * l_sel;
                int e0 = last * l_sel + l_sel;
                if (e0 > t + 1) e0 = t + 1;
                if (m < K) {
                    out[2 * m] = s0;
                    out[2 * m + 1] = e0;
                }
                ++m;
                i = j;
            }
        }
        free(key);
        free(sel);
        free(fa);
    }
    free(keep);
    return 0;
}

/* ------------------------------------------------------------------------- */
/* A8: grouped_selection_attention_masked -- the semantic oracle               */
/*   (nsa/core/attention_kernels.py:705-772)                                    */
/*   allowed = union of clamp([s,e), 0, S_kv); softmax over allowed keys with   */
/*   scale Dk^-1/2; rows without any allowed key -> zeros (:734-749, 769-771).  */
/*   Q [B,S,G,h,Dk], K [B,G,S_kv,Dk], V [B,G,S_kv,Dv], ranges [B,S,G,n,2].      */
/*   O [B,S,G,h,Dv]; lse (nullable) [B,S,G,h] = log sum exp of scaled logits.   */
/* ------------------------------------------------------------------------- */
NSA_API int nsa_oracle_sel_attention_masked(const float *Q, const float *K, const float *V,
                                            const int32_t *ranges, float *O, float *lse, int B,
                                            int S, int G, int h, int Dk, int Dv, int S_kv, int n,
                                            float scale) {
    long R = (long)B * S * G;
#pragma omp parallel
    {
        int *diff = (int *)malloc(sizeof(int) * (size_t)(S_kv + 2));
        int *idx = (int *)malloc(sizeof(int) * (size_t)(S_kv + 1));
        float *sc = (float *)malloc(sizeof(float) * (size_t)(S_kv + 1));
#pragma omp for schedule(dynamic, 4)
        for (long r = 0; r < R; ++r) {
            long g = r % G;
            long b = r / ((long)G * S);
            const int32_t *rg = ranges + r * (long)n * 2;
            /* difference array (:721-732) restricted to the touched span */
            int lo = S_kv, hi = 0;
            for (int i = 0; i < n; ++i) {
                long s0 = rg[2 * i], e0 = rg[2 * i + 1];
                if (s0 < 0) s0 = 0;
                if (s0 > S_kv) s0 = S_kv;
                if (e0 < 0) e0 = 0;
                if (e0 > S_kv) e0 = S_kv;
                if (e0 > s0) {
                    if (s0 < lo) lo = (int)s0;
                    if (e0 > hi) hi = (int)e0;
                }
            }
            int L = 0;
            if (hi > lo) {
                memset(diff + lo, 0, sizeof(int) * (size_t)(hi - lo + 1));
                for (int i = 0; i < n; ++i) {
                    long s0 = rg[2 * i], e0 = rg[2 * i + 1];
                    if (s0 < 0) s0 = 0;
                    if (s0 > S_kv) s0 = S_kv;
                    if (e0 < 0) e0 = 0;
                    if (e0 > S_kv) e0 = S_kv;
                    if (e0 > s0) {
                        diff[s0] += 1;
                        diff[e0] -= 1;
                    }
                }
                int run = 0;
                for (int c = lo; c < hi; ++c) {
                    run += diff[c];
                    if (run > 0) idx[L++] = c;
                }
            }
            const float *Kb = K + ((b * G + g) * (long)S_kv) * Dk;
            const float *Vb = V + ((b * G + g) * (long)S_kv) * Dv;
            for (int hh = 0; hh < h; ++hh) {
                const float *q = Q + (r * h + hh) * (long)Dk;
                float *o = O + (r * h + hh) * (long)Dv;
                for (int e = 0; e < Dv; ++e) o[e] = 0.f;
                if (L == 0) {
                    if (lse) lse[r * h + hh] = -INFINITY;
                    continue;
                }
                float m = -INFINITY;
                for (int i = 0; i < L; ++i) {
                    const float *k = Kb + (long)idx[i] * Dk;
                    float acc = 0.f;
                    for (int e = 0; e < Dk; ++e) acc += q[e] * k[e];
                    acc *= scale;
                    sc[i] = acc;
                    if (acc > m) m = acc;
                }
                double sum = 0.0;
                for (int i = 0; i < L; ++i) {
                    sc[i] = expf(sc[i] - m);
                    sum += (double)sc[i];
                }
                float inv = (float)(1.0 / sum);
                for (int i = 0; i < L; ++i) {
                    float pw = sc[i] * inv;
                    const float *v = Vb + (long)idx[i] * Dv;
                    for (int e = 0; e < Dv; ++e) o[e] += pw * v[e];
                }
                if (lse) lse[r * h + hh] = m + (float)log(sum);
            }
        }
        free(diff);
        free(idx);
        free(sc);
    }
    return 0;
}

/* ------------------------------------------------------------------------- */
/* A8 backward (autograd of the masked SDPA, used to check the HIP backward).   */
/*   dO [B,S,G,h,Dv] -> dQ [B,S,G,h,Dk], dK [B,G,S_kv,Dk], dV [B,G,S_kv,Dv]      */
/*   Serial over rows (accumulates into dK/dV); small test sizes only.           */
/* ------------------------------------------------------------------------- */
NSA_API int nsa_oracle_sel_attention_masked_bwd(const float *Q, const float *K, const float *V,
                                                const int32_t *ranges, const float *dO, float *dQ,
                                                float *dK, float *dV, int B, int S, int G, int h,
                                                int Dk, int Dv, int S_kv, int n, float scale) {
    long R = (long)B * S * G;
    memset(dQ, 0, sizeof(float) * (size_t)(R * h * Dk));
    memset(dK, 0, sizeof(float) * (size_t)((long)B * G * S_kv * Dk));
    memset(dV, 0, sizeof(float) * (size_t)((long)B * G * S_kv * Dv));
    char *allowed = (char *)malloc((size_t)S_kv + 1);
    double *p = (double *)malloc(sizeof(double) * (size_t)(S_kv + 1));
    double *dp = (double *)malloc(sizeof(double) * (size_t)(S_kv + 1));
    for (long r = 0; r < R; ++r) {
        long g = r % G;
        long b = r / ((long)G * S);
        const int32_t *rg = ranges + r * (long)n * 2;
        memset(allowed, 0, (size_t)S_kv + 1);
        int any = 0;
        for (int i = 0; i < n; ++i) {
            long s0 = rg[2 * i], e0 = rg[2 * i + 1];
            if (s0 < 0) s0 = 0;
            if (s0 > S_kv) s0 = S_kv;
            if (e0 < 0) e0 = 0;
            if (e0 > S_kv) e0 = S_kv;
            for (long c = s0; c < e0; ++c) {
                allowed[c] = 1;
                any = 1;
            }
        }
        if (!any) continue;
        const float *Kb = K + ((b * G + g) * (long)S_kv) * Dk;
        const float *Vb = V + ((b * G + g) * (long)S_kv) * Dv;
        float *dKb = dK + ((b * G + g) * (long)S_kv) * Dk;
        float *dVb = dV + ((b * G + g) * (long)S_kv) * Dv;
        for (int hh = 0; hh < h; ++hh) {
            const float *q = Q + (r * h + hh) * (long)Dk;
            const float *go = dO + (r * h + hh) * (long)Dv;
            float *gq = dQ + (r * h + hh) * (long)Dk;
            double m = -INFINITY, sum = 0.0;
            for (int c = 0; c < S_kv; ++c) {
                if (!allowed[c]) continue;
                double acc = 0.0;
                for (int e = 0; e < Dk; ++e) acc += (double)q[e] * Kb[(long)c * Dk + e];
                p[c] = acc * scale;
                if (p[c] > m) m = p[c];
            }
            for (int c = 0; c < S_kv; ++c)
                if (allowed[c]) {
                    p[c] = exp(p[c] - m);
                    sum += p[c];
                }
            double delta = 0.0;
            for (int c = 0; c < S_kv; ++c)
                if (allowed[c]) {
                    p[c] /= sum;
                    double a = 0.0;
                    for (int e = 0; e < Dv; ++e) a += (double)go[e] * Vb[(long)c * Dv + e];
                    dp[c] = a;
                    delta += p[c] * a;
                }
            for (int c = 0; c < S_kv; ++c)
                if (allowed[c]) {
                    double ds = p[c] * (dp[c] - delta) * scale;
                    for (int e = 0; e < Dk; ++e) {
                        gq[e] += (float)(ds * Kb[(long)c * Dk + e]);
                        dKb[(long)c * Dk + e] += (float)(ds * q[e]);
                    }
                    for (int e = 0; e < Dv; ++e) dVb[(long)c * Dv + e] += (float)(p[c] * go[e]);
                }
        }
    }
    free(allowed);
    free(p);
    free(dp);
    return 0;
}

/* ------------------------------------------------------------------------- */
/* A7 alone: convert_indices_to_ranges_batched_v2                              */
/*   (nsa/core/selection_scorer.py:434-605).  indices [R,K] sorted ascending,   */
/*   -1 padded; per-row clamp t_rows[r]+1; out [R,K,2] zero padded.  Ids outside */
/*   [0,S_sel) make the run invalid -> [0,0] (:554-565).                         */
/* ------------------------------------------------------------------------- */
NSA_API int nsa_oracle_indices_to_ranges_v2(const int32_t *indices, long R, int K, int S_sel,
                                            int l_sel, const int32_t *t_rows, int32_t *ranges) {
#pragma omp parallel for schedule(static)
    for (long r = 0; r < R; ++r) {
        const int32_t *x = indices + r * (long)K;
        int32_t *out = ranges + r * (long)K * 2;
        memset(out, 0, sizeof(int32_t) * (size_t)K * 2);
        int t = t_rows[r];
        int m = 0;
        int i = 0;
        while (i < K) {
            if (x[i] < 0) {
                ++i;
                continue;
            }
            int first = x[i], last = x[i];
            int j = i + 1;
            /* :470-474 a run continues while the previous element is valid and diff in {0,1} */
            while (j < K && x[j] >= 0 && (x[j] - x[j - 1] == 0 || x[j] - x[j - 1] == 1)) {
                if (x[j] > last) last = x[j];
                ++j;
            }
            if (first < S_sel && last >= 0 && last < S_sel) {
                int s0 = first * l_sel;
                int e0 = last * l_sel + l_sel;
                if (e0 > t + 1) e0 = t + 1;
                out[2 * m] = s0;
                out[2 * m + 1] = e0;
            }
            ++m;
            i = j;
        }
    }
    return 0;
}

NSA_API int nsa_oracle_num_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

NSA_API void nsa_oracle_set_num_threads(int n) {
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

/* ------------------------------------------------------------------------- */
/* Gate MLP + three-branch mix  (nsa/core/nsa_attention.py:32-82, 1380-1395)  */
/* ------------------------------------------------------------------------- */

/*
 * One row: the fp32 logits and gates of GateMLP.forward (nsa/core/nsa_attention.py:71-81) on the pooled query q_gp = Q.mean(dim=3)
 * (:1381).  Dot products and the head mean accumulate in double and round once to fp32, at the points where the fp32 PyTorch ops round
 * (mean, fc1 + bias, silu, fc2 + bias, / max(tau, 1e-6), softmax).  qp [Dk], act [Hd] and pre [Hd] (fc1 output) are written for the
 * backward.  Returns 1 when the row is "peaked" (top-2 logit gap > 50, :77-81: one-hot of the argmax, first index on ties).
 */
static int gate_row(const float *Q, int h, int Dk, int Hd, const float *w1, const float *b1, const float *w2, const float *b2,
                    float tau, float *qp, float *pre, float *act, float *lg, float *p) {
    for (int k = 0; k < Dk; ++k) { /* :1381 Q.mean(dim=3) */
        double a = 0.0;
        for (int i = 0; i < h; ++i) a += (double)Q[(int64_t)i * Dk + k];
        qp[k] = (float)(a / (double)h);
    }
    for (int j = 0; j < Hd; ++j) { /* :71 silu(fc1(q)) */
        double a = 0.0;
        for (int k = 0; k < Dk; ++k) a += (double)w1[(int64_t)j * Dk + k] * (double)qp[k];
        pre[j] = (float)(a + (double)b1[j]);
        act[j] = (float)((double)pre[j] / (1.0 + exp(-(double)pre[j])));
    }
    const float td = tau > 1e-6f ? tau : 1e-6f; /* :72 / max(tau, 1e-6) */
    for (int c = 0; c < 3; ++c) {
        double a = 0.0;
        for (int j = 0; j < Hd; ++j) a += (double)w2[c * Hd + j] * (double)act[j];
        const float z = (float)(a + (double)b2[c]);
        lg[c] = z / td;
    }
    float mx = lg[0];
    int arg = 0;
    for (int c = 1; c < 3; ++c)
        if (lg[c] > mx) { mx = lg[c]; arg = c; }
    double e[3], den = 0.0; /* :73 softmax */
    for (int c = 0; c < 3; ++c) { e[c] = exp((double)lg[c] - (double)mx); den += e[c]; }
    float second = -INFINITY;
    for (int c = 0; c < 3; ++c)
        if (c != arg && lg[c] > second) second = lg[c];
    const int peaked = (lg[arg] - second) > 50.0f; /* :76-78 */
    for (int c = 0; c < 3; ++c) p[c] = peaked ? (c == arg ? 1.0f : 0.0f) : (float)(e[c] / den);
    return peaked;
}

/*
 * nsa/core/nsa_attention.py:1380-1395 (prefill; the decode form :931-950 is the same expression per [B,G] row): gates [R,3] of
 * GateMLP.forward and O = w_cmp * O_cmp + w_sel * O_sel + w_win * O_win in fp32, left to right, one rounding per op.
 * Q [R,h,Dk]; O_cmp, O_sel, O_win, O [R,h,Dv]; w1 [Hd,Dk], b1 [Hd], w2 [3,Hd], b2 [3].  logits [R,3] may be NULL.
 */
NSA_API void nsa_oracle_gate_combine(const float *Q, const float *Oc, const float *Os, const float *Ow, const float *w1, const float *b1,
                                     const float *w2, const float *b2, long R, int h, int Dk, int Dv, int Hd, float tau, float *gates,
                                     float *O, float *logits) {
#pragma omp parallel for schedule(static)
    for (long r = 0; r < R; ++r) {
        float *qp = (float *)malloc(sizeof(float) * (size_t)(Dk + 2 * Hd));
        float *pre = qp + Dk, *act = pre + Hd;
        float lg[3], p[3];
        gate_row(Q + (int64_t)r * h * Dk, h, Dk, Hd, w1, b1, w2, b2, tau, qp, pre, act, lg, p);
        for (int c = 0; c < 3; ++c) {
            gates[r * 3 + c] = p[c];
            if (logits) logits[r * 3 + c] = lg[c];
        }
        const int64_t base = (int64_t)r * h * Dv;
        for (int e = 0; e < h * Dv; ++e) {
            const float t1 = p[0] * Oc[base + e], t2 = p[1] * Os[base + e];
            const float t3 = t1 + t2, t4 = p[2] * Ow[base + e];
            O[base + e] = t3 + t4;
        }
        free(qp);
    }
}

/*
 * Gradient of nsa_oracle_gate_combine (the autograd of nsa/core/nsa_attention.py:70-81 + 1392-1395) for the upstream gradient dO [R,h,Dv]:
 *   dO_i = gate_i dO (fp32 products), dgates [R,3] = sum_{h,d} O_i dO;
 *   peaked rows: the gates are the one-hot (torch.where of :81 passes no gradient to the softmax) -> no gradient into the MLP;
 *   else dlogit = p (dgates - <p, dgates>) / max(tau, 1e-6), then fc2, silu'(x) = s(x)(1 + x (1 - s(x))), fc1, and dQ = dq_gp / h
 *   on every head (the mean).  dW1 [Hd,Dk], db1 [Hd], dW2 [3,Hd], db2 [3] are summed over the R rows.  Inner math in double.
 */
NSA_API void nsa_oracle_gate_combine_bwd(const float *Q, const float *Oc, const float *Os, const float *Ow, const float *w1, const float *b1,
                                         const float *w2, const float *b2, const float *dO, long R, int h, int Dk, int Dv, int Hd, float tau,
                                         float *dOc, float *dOs, float *dOw, float *dgates, float *dQ, float *dW1, float *db1, float *dW2,
                                         float *db2) {
    double *aW1 = (double *)calloc((size_t)Hd * Dk + Hd + 3 * (size_t)Hd + 3, sizeof(double));
    double *ab1 = aW1 + (size_t)Hd * Dk, *aW2 = ab1 + Hd, *ab2 = aW2 + 3 * Hd;
    float *qp = (float *)malloc(sizeof(float) * (size_t)(Dk + 2 * Hd));
    float *pre = qp + Dk, *act = pre + Hd;
    double *da = (double *)malloc(sizeof(double) * (size_t)(Hd + Dk));
    double *dq = da + Hd;
    const double td = tau > 1e-6f ? (double)tau : (double)1e-6f;
    for (long r = 0; r < R; ++r) {
        float lg[3], p[3];
        const int peaked = gate_row(Q + (int64_t)r * h * Dk, h, Dk, Hd, w1, b1, w2, b2, tau, qp, pre, act, lg, p);
        const int64_t base = (int64_t)r * h * Dv;
        double dg[3] = {0.0, 0.0, 0.0};
        for (int e = 0; e < h * Dv; ++e) {
            const float d = dO[base + e];
            dOc[base + e] = p[0] * d;
            dOs[base + e] = p[1] * d;
            dOw[base + e] = p[2] * d;
            dg[0] += (double)Oc[base + e] * d;
            dg[1] += (double)Os[base + e] * d;
            dg[2] += (double)Ow[base + e] * d;
        }
        for (int c = 0; c < 3; ++c) dgates[r * 3 + c] = (float)dg[c];
        float *dQr = dQ + (int64_t)r * h * Dk;
        if (peaked) {
            memset(dQr, 0, sizeof(float) * (size_t)h * Dk);
            continue;
        }
        const double dot = (double)p[0] * dg[0] + (double)p[1] * dg[1] + (double)p[2] * dg[2];
        double dl[3];
        for (int c = 0; c < 3; ++c) {
            dl[c] = (double)p[c] * (dg[c] - dot) / td;
            ab2[c] += dl[c];
            for (int j = 0; j < Hd; ++j) aW2[c * Hd + j] += dl[c] * (double)act[j];
        }
        for (int j = 0; j < Hd; ++j) {
            const double x = (double)pre[j], s = 1.0 / (1.0 + exp(-x));
            const double dact = dl[0] * w2[j] + dl[1] * w2[Hd + j] + dl[2] * w2[2 * Hd + j];
            da[j] = dact * s * (1.0 + x * (1.0 - s));
            ab1[j] += da[j];
            for (int k = 0; k < Dk; ++k) aW1[(int64_t)j * Dk + k] += da[j] * (double)qp[k];
        }
        for (int k = 0; k < Dk; ++k) {
            double a = 0.0;
            for (int j = 0; j < Hd; ++j) a += da[j] * (double)w1[(int64_t)j * Dk + k];
            dq[k] = a / (double)h;
        }
        for (int i = 0; i < h; ++i)
            for (int k = 0; k < Dk; ++k) dQr[(int64_t)i * Dk + k] = (float)dq[k];
    }
    for (int64_t i = 0; i < (int64_t)Hd * Dk; ++i) dW1[i] = (float)aW1[i];
    for (int j = 0; j < Hd; ++j) db1[j] = (float)ab1[j];
    for (int i = 0; i < 3 * Hd; ++i) dW2[i] = (float)aW2[i];
    for (int c = 0; c < 3; ++c) db2[c] = (float)ab2[c];
    free(da);
    free(qp);
    free(aW1);
}

/* ------------------------------------------------------------------------- */
/* RoPE and compressed-token pooling  (nsa/core/rope.py:6-51,                 */
/* nsa/core/compress_pool.py:9-38)                                            */
/* ------------------------------------------------------------------------- */

/*
 * dt: the activation dtype of the reference's chain, coded as the package's NSA_DT_* (0 fp32, 1 bf16, 2 fp16).  rnd_dt rounds a double
 * the way a PyTorch CPU op of that dtype leaves its result: to fp32 first (the op's compute type), then round-to-nearest-even to the dtype.
 */
static float rnd_dt(double x, int dt) {
    float f = (float)x;
    if (dt == 1) { /* bf16: keep the top 16 bits, ties to even */
        uint32_t u;
        memcpy(&u, &f, 4);
        if ((u & 0x7f800000u) != 0x7f800000u) {
            u += 0x7fffu + ((u >> 16) & 1u);
            u &= 0xffff0000u;
            memcpy(&f, &u, 4);
        }
    } else if (dt == 2 && f != 0.0f && isfinite(f)) { /* fp16: 11 significant bits, subnormals below 2^-14 */
        int e;
        frexp((double)f, &e); /* |f| = m 2^e, m in [0.5, 1) */
        const int q = (e - 1 < -14 ? -14 : e - 1) - 10;
        const double r = nearbyint(ldexp((double)f, -q));
        f = (float)ldexp(r, q);
        if (fabsf(f) > 65504.0f) f = copysignf(INFINITY, f);
    }
    return f;
}

/* nsa/core/rope.py:6-13: inv_freq[i] = base ** (-2 i / D), the exponent an fp32 division, the power evaluated in double and rounded once */
static float rope_freq(int i, int D, float base) {
    const float e = (float)((-2.0 * (double)i) / (double)D);
    return (float)pow((double)base, (double)e);
}

NSA_API void nsa_oracle_rope_inv_freq(int D, float base, float *out) {
    for (int i = 0; i < D / 2; ++i) out[i] = rope_freq(i, D, base);
}

/* nsa/core/rope.py:38-44: angle = fl(fl(pos / scale) * inv_freq) in fp32; sin / cos of that angle in double, rounded to the dtype */
static void rope_sc(int p, int i, int D, float base, float scale, int dt, float *sn, float *cs) {
    const float s = scale > 0.0f ? scale : 1.0f; /* :35-36 */
    const float ps = (float)((double)p / (double)s);
    const float a = (float)((double)ps * (double)rope_freq(i, D, base));
    *sn = rnd_dt(sin((double)a), dt);
    *cs = rnd_dt(cos((double)a), dt);
}

/*
 * nsa/core/rope.py:16-51 on rows x [R,D] (adjacent pairs (2i, 2i+1) of the last dim), row r at position pos[r]:
 * y0 = x0 c - x1 s, y1 = x0 s + x1 c with a rounding to the dtype after every product and sum (:45-48).
 */
NSA_API void nsa_oracle_rope(const float *x, const int *pos, long R, int D, float base, float scale, int dt, float *y) {
#pragma omp parallel for schedule(static)
    for (long r = 0; r < R; ++r)
        for (int i = 0; i < D / 2; ++i) {
            float sn, cs;
            rope_sc(pos[r], i, D, base, scale, dt, &sn, &cs);
            const double x0 = x[(int64_t)r * D + 2 * i], x1 = x[(int64_t)r * D + 2 * i + 1];
            y[(int64_t)r * D + 2 * i] = rnd_dt((double)rnd_dt(x0 * cs, dt) - (double)rnd_dt(x1 * sn, dt), dt);
            y[(int64_t)r * D + 2 * i + 1] = rnd_dt((double)rnd_dt(x0 * sn, dt) + (double)rnd_dt(x1 * cs, dt), dt);
        }
}

/* the autograd of nsa/core/rope.py:45-48 for the upstream gradient g [R,D]: dx0 = g0 c + g1 s, dx1 = g1 c - g0 s, each product and the
 * sum of the two paths rounded to the dtype */
static void rope_bwd_pair(double g0, double g1, float sn, float cs, int dt, float *d0, float *d1) {
    *d0 = rnd_dt((double)rnd_dt(g0 * cs, dt) + (double)rnd_dt(g1 * sn, dt), dt);
    *d1 = rnd_dt((double)rnd_dt(g1 * cs, dt) - (double)rnd_dt(g0 * sn, dt), dt);
}

NSA_API void nsa_oracle_rope_bwd(const float *g, const int *pos, long R, int D, float base, float scale, int dt, float *dx) {
#pragma omp parallel for schedule(static)
    for (long r = 0; r < R; ++r)
        for (int i = 0; i < D / 2; ++i) {
            float sn, cs;
            rope_sc(pos[r], i, D, base, scale, dt, &sn, &cs);
            rope_bwd_pair(g[(int64_t)r * D + 2 * i], g[(int64_t)r * D + 2 * i + 1], sn, cs, dt, dx + (int64_t)r * D + 2 * i,
                          dx + (int64_t)r * D + 2 * i + 1);
        }
}

/*
 * nsa/core/compress_pool.py:9-38 (avg_pool_phi_rope_kv with pos given): K_rope = apply_rope(K_raw, pos) WITHOUT position scaling (:20),
 * then the mean over windows of l rows with stride d (avg_pool2d, :31-32) of K_rope and of the raw V.  K_raw [nbg,S,Dk], V_raw [nbg,S,Dv],
 * pos [S] -> K_cmp [nbg,n_cmp,Dk], V_cmp [nbg,n_cmp,Dv] with n_cmp = 0 for S < l (:24-28), else (S - l) / d + 1.  The window sum is exact
 * (double), divided by l and rounded once to the dtype.
 */
NSA_API void nsa_oracle_cmp_pool(const float *K_raw, const float *V_raw, const int *pos, long nbg, int S, int Dk, int Dv, int l, int d,
                                 float base, int dt, float *K_cmp, float *V_cmp) {
    const int n_cmp = S < l ? 0 : (S - l) / d + 1;
#pragma omp parallel for schedule(static)
    for (long bg = 0; bg < nbg; ++bg) {
        float *kr = (float *)malloc(sizeof(float) * (size_t)Dk);
        for (int j = 0; j < n_cmp; ++j) {
            float *kc = K_cmp + ((int64_t)bg * n_cmp + j) * Dk;
            float *vc = V_cmp + ((int64_t)bg * n_cmp + j) * Dv;
            double *ak = (double *)calloc((size_t)(Dk + Dv), sizeof(double));
            for (int i = 0; i < l; ++i) {
                const int r = j * d + i;
                nsa_oracle_rope(K_raw + ((int64_t)bg * S + r) * Dk, pos + r, 1, Dk, base, 1.0f, dt, kr);
                for (int c = 0; c < Dk; ++c) ak[c] += kr[c];
                for (int c = 0; c < Dv; ++c) ak[Dk + c] += V_raw[((int64_t)bg * S + r) * Dv + c];
            }
            for (int c = 0; c < Dk; ++c) kc[c] = rnd_dt(ak[c] / (double)l, dt);
            for (int c = 0; c < Dv; ++c) vc[c] = rnd_dt(ak[Dk + c] / (double)l, dt);
            free(ak);
        }
        free(kr);
    }
}

/*
 * The autograd of nsa_oracle_cmp_pool for the upstream gradients dK_cmp [nbg,n_cmp,Dk], dV_cmp [nbg,n_cmp,Dv] (n_cmp may be smaller than
 * the forward's count, 0 included): raw row r receives 1/l of the gradient of every window j < n_cmp with j d <= r < j d + l (avg_pool2d
 * backward: each window's share rounded to the dtype and added to the row in the dtype, j ascending), and its key gradient is rotated back
 * at pos[r] (rope_bwd_pair).  A row in no window gets exactly 0.
 */
NSA_API void nsa_oracle_cmp_pool_bwd(const float *dK_cmp, const float *dV_cmp, const int *pos, long nbg, int S, int n_cmp, int Dk, int Dv,
                                     int l, int d, float base, int dt, float *dK_raw, float *dV_raw) {
#pragma omp parallel for schedule(static)
    for (long bg = 0; bg < nbg; ++bg) {
        double *a = (double *)malloc(sizeof(double) * (size_t)(Dk + Dv));
        for (int r = 0; r < S; ++r) {
            for (int c = 0; c < Dk + Dv; ++c) a[c] = 0.0;
            for (int j = 0; j < n_cmp; ++j) {
                if (!(j * d <= r && r < j * d + l)) continue;
                for (int c = 0; c < Dk; ++c) a[c] = rnd_dt(a[c] + (double)rnd_dt(dK_cmp[((int64_t)bg * n_cmp + j) * Dk + c] / (double)l, dt), dt);
                for (int c = 0; c < Dv; ++c) a[Dk + c] = rnd_dt(a[Dk + c] + (double)rnd_dt(dV_cmp[((int64_t)bg * n_cmp + j) * Dv + c] / (double)l, dt), dt);
            }
            float *dk = dK_raw + ((int64_t)bg * S + r) * Dk;
            for (int i = 0; i < Dk / 2; ++i) {
                float sn, cs;
                rope_sc(pos[r], i, Dk, base, 1.0f, dt, &sn, &cs);
                rope_bwd_pair(a[2 * i], a[2 * i + 1], sn, cs, dt, dk + 2 * i, dk + 2 * i + 1);
            }
            for (int c = 0; c < Dv; ++c) dV_raw[((int64_t)bg * S + r) * Dv + c] = (float)a[Dk + c];
        }
        free(a);
    }
}
