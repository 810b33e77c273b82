// Host side of the paged caches' copy calls (nsa_paged_kv_store / nsa_paged_kv_load / nsa_paged_kv_copy_pages; paged_kv_copy.hip has the
// kernels): the argument blocks, the argument checks and the grid sizes.  Plain C++ with no HIP in it, so that the checks also build as a
// host program of their own (paged_kv_copy_check.cpp).  A check that fails writes its message into `msg` and answers NSA_ERR_INVALID; the
// entry points hand the message to nsa_hip_last_error().
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/nsa_sel_hip.h"

namespace nsa {

constexpr int PKV_PAGE_TOKENS = 1024, PKV_PAGE_CMP = 64;  // rows of a page: the six token pools, K_cmp / V_cmp (l = 32, d = 16)
constexpr int PKV_MAX_PAGES = 1 << 20;                    // as nsa_layer_decode_paged: max_pages * 1024 stays an int
constexpr int PKV_TILE_TOKENS = 256, PKV_TILE_CMP = 64;   // rows one workgroup copies; both divide their page, so a tile lies in ONE page
constexpr int PKV_MAX_GRID_Y = 65535;

// compressed rows emitted once t tokens are cached (l = 32, d = 16)
inline int pkv_ncmp(int t) { return t < 32 ? 0 : (t - 32) / 16 + 1; }

// tensors 0 .. 5: K_sel, V_sel, K_win, V_win, K_raw, V_raw (rows of 1024-token pages); 6, 7: K_cmp, V_cmp (rows of 64-row pages).  Even: Dk, odd: Dv
struct PagedCopyParams {
    unsigned char *pool[8];
    unsigned char *slab[8];    // slab b_src of the contiguous cache: [G, S_max | n_cmp_max, D]
    const int32_t *table_row;  // row `slot` of the block table
    int n_pages, max_pages, G, Dk, Dv, S_max, n_cmp_max;
    int t0, t1, c0, c1;  // token rows [t0, t1), compressed rows [c0, c1)
};
struct PagedJobsParams {
    unsigned char *pool[8];
    const int32_t *jobs;  // [n_jobs, 4]: src page, dst page, token rows, compressed rows
    int n_pages, G, Dk, Dv;
};
struct PagedCopyGrid {
    unsigned x, y, z;  // all zero: nothing to launch
};

#define PKV_CHECK(cond, ...)                  \
    do {                                      \
        if (!(cond)) {                        \
            snprintf(msg, msg_len, __VA_ARGS__); \
            return NSA_ERR_INVALID;           \
        }                                     \
    } while (0)

// what the three calls ask of the pools and their geometry
inline int paged_pools_check(const char *who, const nsa_paged_kv_desc *pkv, int G, int Dk, int Dv, int dtype, unsigned char *pool[8], char *msg,
                             size_t msg_len) {
    PKV_CHECK(pkv, "%s: null pool descriptor", who);
    void *const p[8] = {pkv->K_sel, pkv->V_sel, pkv->K_win, pkv->V_win, pkv->K_raw, pkv->V_raw, pkv->K_cmp, pkv->V_cmp};
    uintptr_t bits = 0;
    for (int i = 0; i < 8; ++i) {
        PKV_CHECK(p[i], "%s: null pool pointer", who);
        bits |= (uintptr_t)p[i];
        pool[i] = (unsigned char *)p[i];
    }
    PKV_CHECK(bits % 16 == 0, "%s: the eight pools must be 16-byte aligned", who);
    PKV_CHECK(dtype == NSA_DT_BF16 || dtype == NSA_DT_F16, "%s: bf16 / f16 pools only (dtype = %d)", who, dtype);
    PKV_CHECK((Dk == 64 || Dk == 128) && (Dv == 64 || Dv == 128), "%s: Dk and Dv in {64, 128} only (got %d, %d)", who, Dk, Dv);
    PKV_CHECK(G >= 1 && 8 * (int64_t)G <= PKV_MAX_GRID_Y, "%s: G = %d outside [1, %d]", who, G, PKV_MAX_GRID_Y / 8);
    PKV_CHECK(pkv->n_pages >= 1, "%s: bad pool size (n_pages = %d)", who, pkv->n_pages);
    return NSA_OK;
}

// nsa_paged_kv_store / nsa_paged_kv_load: the checks, the argument block and the grid
inline int paged_copy_plan(const char *who, const nsa_paged_kv_desc *pkv, const nsa_kv_desc *kv, int b_src, int slot, int t0, int t1, int G, int Dk,
                           int Dv, int dtype, PagedCopyParams *P, PagedCopyGrid *grid, char *msg, size_t msg_len) {
    *grid = PagedCopyGrid{0, 0, 0};
    if (int rc = paged_pools_check(who, pkv, G, Dk, Dv, dtype, P->pool, msg, msg_len)) return rc;
    PKV_CHECK(kv, "%s: null cache descriptor", who);
    void *const s[8] = {kv->K_sel, kv->V_sel, kv->K_win, kv->V_win, kv->K_raw, kv->V_raw, kv->K_cmp, kv->V_cmp};
    uintptr_t bits = 0;
    for (int i = 0; i < 8; ++i) {
        PKV_CHECK(s[i], "%s: null cache pointer", who);
        bits |= (uintptr_t)s[i];
    }
    PKV_CHECK(bits % 16 == 0, "%s: the eight caches must be 16-byte aligned", who);
    PKV_CHECK(pkv->block_table, "%s: null block table", who);
    PKV_CHECK(pkv->max_pages >= 1 && pkv->max_pages <= PKV_MAX_PAGES, "%s: max_pages = %d outside [1, %d]", who, pkv->max_pages, PKV_MAX_PAGES);
    PKV_CHECK((uintptr_t)pkv->block_table % 4 == 0 && pkv->table_stride >= pkv->max_pages,
              "%s: the block table must be 4-byte aligned with a row stride of at least max_pages = %d (got %lld)", who, pkv->max_pages,
              (long long)pkv->table_stride);
    PKV_CHECK(pkv->B >= 1 && slot >= 0 && slot < pkv->B, "%s: slot = %d outside [0, B = %d)", who, slot, pkv->B);
    PKV_CHECK(kv->B >= 1 && b_src >= 0 && b_src < kv->B, "%s: b_src = %d outside [0, B = %d)", who, b_src, kv->B);
    PKV_CHECK(kv->S_max >= 1 && kv->n_cmp_max >= 1, "%s: bad cache sizes (S_max = %d, n_cmp_max = %d)", who, kv->S_max, kv->n_cmp_max);
    PKV_CHECK(t0 >= 0 && t1 >= t0, "%s: rows [t0, t1) = [%d, %d) need 0 <= t0 <= t1", who, t0, t1);
    PKV_CHECK(t1 <= kv->S_max, "%s: t1 = %d beyond the cache's S_max = %d", who, t1, kv->S_max);
    const int cap = pkv->max_pages * PKV_PAGE_TOKENS;
    PKV_CHECK(t1 <= cap, "%s: t1 = %d beyond the slot's capacity max_pages * 1024 = %d", who, t1, cap);
    const int c0 = pkv_ncmp(t0), c1 = pkv_ncmp(t1);
    PKV_CHECK(c1 <= kv->n_cmp_max, "%s: n_cmp(t1) = %d compressed rows beyond the cache's n_cmp_max = %d", who, c1, kv->n_cmp_max);
    for (int i = 0; i < 8; ++i) {
        const int64_t rows = i < 6 ? kv->S_max : kv->n_cmp_max, D = (i & 1) ? Dv : Dk;
        P->slab[i] = (unsigned char *)s[i] + (int64_t)b_src * G * rows * D * 2;
    }
    P->table_row = pkv->block_table + (int64_t)slot * pkv->table_stride;
    P->n_pages = pkv->n_pages; P->max_pages = pkv->max_pages; P->G = G; P->Dk = Dk; P->Dv = Dv; P->S_max = kv->S_max; P->n_cmp_max = kv->n_cmp_max;
    P->t0 = t0; P->t1 = t1; P->c0 = c0; P->c1 = c1;
    if (t0 == t1) return NSA_OK;  // nothing to copy (no token rows: no compressed rows either)
    // one workgroup per tile of 256 token rows or 64 compressed rows of one (tensor, g); the tiles are aligned, so the first one may begin below
    // t0 / c0.  The compressed tensors have the fewer tiles: their surplus workgroups exit at once
    const unsigned nt = (unsigned)((t1 - 1) / PKV_TILE_TOKENS - t0 / PKV_TILE_TOKENS + 1);
    const unsigned nc = c1 > c0 ? (unsigned)((c1 - 1) / PKV_TILE_CMP - c0 / PKV_TILE_CMP + 1) : 0u;
    *grid = PagedCopyGrid{nt > nc ? nt : nc, 8u * (unsigned)G, 1u};
    return NSA_OK;
}

// nsa_paged_kv_copy_pages
inline int paged_jobs_plan(const char *who, const nsa_paged_kv_desc *pkv, const int32_t *jobs, int n_jobs, int G, int Dk, int Dv, int dtype,
                           PagedJobsParams *P, PagedCopyGrid *grid, char *msg, size_t msg_len) {
    *grid = PagedCopyGrid{0, 0, 0};
    if (int rc = paged_pools_check(who, pkv, G, Dk, Dv, dtype, P->pool, msg, msg_len)) return rc;
    PKV_CHECK(n_jobs >= 0, "%s: n_jobs = %d is negative", who, n_jobs);
    PKV_CHECK(jobs || n_jobs == 0, "%s: null job array", who);
    PKV_CHECK((uintptr_t)jobs % 4 == 0, "%s: the job array must be 4-byte aligned", who);
    P->jobs = jobs; P->n_pages = pkv->n_pages; P->G = G; P->Dk = Dk; P->Dv = Dv;
    if (n_jobs == 0) return NSA_OK;
    // per job and (tensor, g): the four 256-row tiles of a token page; the compressed page is the first of them alone
    *grid = PagedCopyGrid{(unsigned)n_jobs, 8u * (unsigned)G, (unsigned)(PKV_PAGE_TOKENS / PKV_TILE_TOKENS)};
    return NSA_OK;
}

#undef PKV_CHECK

}  // namespace nsa
