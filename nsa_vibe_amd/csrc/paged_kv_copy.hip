// nsa_paged_kv_store / nsa_paged_kv_load / nsa_paged_kv_copy_pages: how a sequence gets into the pages of the paged caches, out of them, and
// from one page into another.  Plain streaming copies, one launch each: a workgroup copies one aligned TILE of rows (256 token rows or 64
// compressed rows, both divisors of their page, so a tile lies in one page) of one (tensor, g) with 16-byte loads and stores, eight in
// flight per lane.  The page id is read once per workgroup from blockIdx-derived, hence wave-uniform, indices and tested against
// [0, n_pages) before any address is formed from it; a failed test ends the workgroup.  paged_kv_copy.hpp has the host checks and the grids.
#include "nsa_common.hpp"
#include "paged_kv_copy.hpp"

namespace nsa {

constexpr int PKV_BATCH = 8;  // 16-byte chunks a lane has in flight

// rows [r_lo, r_hi) of a tile of n_rows rows of 1 << (shift + 4) bytes: src -> dst, chunk k = 16 bytes at offset 16 k of either side
__device__ __forceinline__ void pkv_copy_tile(const unsigned char *src, unsigned char *dst, int n_rows, int shift, int r_lo, int r_hi) {
    const int n_chunks = n_rows << shift;
    for (int base = 0; base < n_chunks; base += 256 * PKV_BATCH) {
        uint4 v[PKV_BATCH];
        const int k0 = base + (int)threadIdx.x;
#pragma unroll
        for (int i = 0; i < PKV_BATCH; ++i) {
            const int k = k0 + i * 256, row = k >> shift;
            v[i] = make_uint4(0u, 0u, 0u, 0u);
            if (k < n_chunks && row >= r_lo && row < r_hi) v[i] = *reinterpret_cast<const uint4 *>(src + (size_t)k * 16);
        }
#pragma unroll
        for (int i = 0; i < PKV_BATCH; ++i) {
            const int k = k0 + i * 256, row = k >> shift;
            if (k < n_chunks && row >= r_lo && row < r_hi) *reinterpret_cast<uint4 *>(dst + (size_t)k * 16) = v[i];
        }
    }
}

// grid (tiles, 8 G): blockIdx.y = tensor * G + g.  TO_PAGES: slab -> pages (store), else pages -> slab (load)
template <bool TO_PAGES>
__global__ __launch_bounds__(256) void paged_kv_copy_kernel(PagedCopyParams P) {
    const int tensor = (int)blockIdx.y / P.G, g = (int)blockIdx.y - tensor * P.G;
    if (tensor >= 8) return;
    const bool cmp = tensor >= 6;
    const int tile_rows = cmp ? PKV_TILE_CMP : PKV_TILE_TOKENS, page_rows = cmp ? PKV_PAGE_CMP : PKV_PAGE_TOKENS;
    const int lo = cmp ? P.c0 : P.t0, hi = cmp ? P.c1 : P.t1, slab_rows = cmp ? P.n_cmp_max : P.S_max;
    const int64_t first = ((int64_t)(lo / tile_rows) + blockIdx.x) * tile_rows;  // the tile's first row (of the sequence)
    if (first >= hi) return;
    const int64_t j = first / page_rows;
    if (j >= P.max_pages) return;
    const int page = P.table_row[j];
    if (page < 0 || page >= P.n_pages) return;  // no page, or a bad id: these rows are skipped
    const int D = (tensor & 1) ? P.Dv : P.Dk, shift = D == 64 ? 3 : 4;  // 16-byte chunks per row: 8 / 16
    const int64_t row_bytes = (int64_t)D * 2;
    unsigned char *pg = P.pool[tensor] + (((int64_t)page * P.G + g) * page_rows + first % page_rows) * row_bytes;
    unsigned char *sl = P.slab[tensor] + ((int64_t)g * slab_rows + first) * row_bytes;
    // rows of the tile inside [lo, hi); hi <= slab_rows (the host's check), so no slab row beyond the slab is touched
    const int r_lo = lo > first ? (int)(lo - first) : 0, r_hi = hi - first < tile_rows ? (int)(hi - first) : tile_rows;
    if (TO_PAGES) pkv_copy_tile(sl, pg, tile_rows, shift, r_lo, r_hi);
    else pkv_copy_tile(pg, sl, tile_rows, shift, r_lo, r_hi);
}

// grid (n_jobs, 8 G, 4): blockIdx.z = the 256-row tile of the token page; the compressed page is tile 0 alone
__global__ __launch_bounds__(256) void paged_kv_copy_pages_kernel(PagedJobsParams P) {
    const int tensor = (int)blockIdx.y / P.G, g = (int)blockIdx.y - tensor * P.G;
    if (tensor >= 8) return;
    const int32_t *J = P.jobs + (int64_t)blockIdx.x * 4;
    const int src = J[0], dst = J[1], n_tok = J[2], n_cmp = J[3];
    // a bad page id or a count beyond the page: the whole job is skipped
    if (src < 0 || src >= P.n_pages || dst < 0 || dst >= P.n_pages || n_tok < 0 || n_tok > PKV_PAGE_TOKENS || n_cmp < 0 || n_cmp > PKV_PAGE_CMP) return;
    const bool cmp = tensor >= 6;
    const int tile_rows = cmp ? PKV_TILE_CMP : PKV_TILE_TOKENS, page_rows = cmp ? PKV_PAGE_CMP : PKV_PAGE_TOKENS;
    const int first = (int)blockIdx.z * tile_rows, hi = cmp ? n_cmp : n_tok;
    if ((cmp && blockIdx.z != 0) || first >= hi) return;
    const int D = (tensor & 1) ? P.Dv : P.Dk, shift = D == 64 ? 3 : 4;
    const int64_t row_bytes = (int64_t)D * 2;
    const unsigned char *s = P.pool[tensor] + (((int64_t)src * P.G + g) * page_rows + first) * row_bytes;
    unsigned char *d = P.pool[tensor] + (((int64_t)dst * P.G + g) * page_rows + first) * row_bytes;
    pkv_copy_tile(s, d, tile_rows, shift, 0, hi - first < tile_rows ? hi - first : tile_rows);
}

template <bool TO_PAGES>
static int paged_kv_copy(const char *who, const nsa_paged_kv_desc *pkv, const nsa_kv_desc *kv, int b_src, int slot, int t0, int t1, int G, int Dk, int Dv,
                         int dtype, void *stream) {
    PagedCopyParams P{};
    PagedCopyGrid grid{};
    char msg[256];
    if (int rc = paged_copy_plan(who, pkv, kv, b_src, slot, t0, t1, G, Dk, Dv, dtype, &P, &grid, msg, sizeof(msg))) {
        set_error("%s", msg);
        return rc;
    }
    if (grid.x == 0) return NSA_OK;
    hipLaunchKernelGGL((paged_kv_copy_kernel<TO_PAGES>), dim3(grid.x, grid.y, grid.z), dim3(256), 0, (hipStream_t)stream, P);
    NSA_LAUNCH_CHECK("paged_kv_copy_kernel");
    return NSA_OK;
}

}  // namespace nsa

using namespace nsa;

extern "C" {

int nsa_paged_kv_store(const nsa_paged_kv_desc *pkv, const nsa_kv_desc *kv, int b_src, int slot, int t0, int t1, int G, int Dk, int Dv, int dtype,
                       void *stream) {
    return paged_kv_copy<true>("paged_kv_store", pkv, kv, b_src, slot, t0, t1, G, Dk, Dv, dtype, stream);
}

int nsa_paged_kv_load(const nsa_paged_kv_desc *pkv, const nsa_kv_desc *kv, int b_src, int slot, int t0, int t1, int G, int Dk, int Dv, int dtype,
                      void *stream) {
    return paged_kv_copy<false>("paged_kv_load", pkv, kv, b_src, slot, t0, t1, G, Dk, Dv, dtype, stream);
}

int nsa_paged_kv_copy_pages(const nsa_paged_kv_desc *pkv, const int32_t *jobs, int n_jobs, int G, int Dk, int Dv, int dtype, void *stream) {
    PagedJobsParams P{};
    PagedCopyGrid grid{};
    char msg[256];
    if (int rc = paged_jobs_plan("paged_kv_copy_pages", pkv, jobs, n_jobs, G, Dk, Dv, dtype, &P, &grid, msg, sizeof(msg))) {
        set_error("%s", msg);
        return rc;
    }
    if (grid.x == 0) return NSA_OK;
    hipLaunchKernelGGL(paged_kv_copy_pages_kernel, dim3(grid.x, grid.y, grid.z), dim3(256), 0, (hipStream_t)stream, P);
    NSA_LAUNCH_CHECK("paged_kv_copy_pages_kernel");
    return NSA_OK;
}

}  // extern "C"
