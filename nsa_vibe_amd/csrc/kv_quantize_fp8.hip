// nsa_kv_quantize_fp8 / nsa_paged_kv_quantize_fp8: rows [t0, t1) of a bf16 K or V tensor -> OCP e4m3 rows plus one fp32 scale per row, the
// cache format of nsa_sel_decode_ragged_fp8 / nsa_sel_decode_paged_fp8.  One launch per appended chunk keeps an fp8 mirror current.
//   scale = amax / 448 (IEEE fp32 division; 1.0f for an all-zero row),  q = e4m3_rne(clamp(x / scale, -448, 448))
// A row that holds a NaN, a +inf or a -inf gets a NaN scale and an e4m3 NaN code (0x7F or 0xFF) in every byte, so the corruption reaches the
// FP8 attention calls as it reaches the bf16 calls through a bf16 cache: NaN output rows from a V row; from a K row what those kernels make of
// a NaN row sum (the clamp alone would turn the element into -448 under a finite scale taken from the row's other elements).
// A row is D / 8 lanes of 16 bytes (8 lanes at D = 64, 16 at D = 128), so a wave takes 8 / 4 rows at once; what the row's lanes do is
// kv_quantize_fp8_row (kv_quantize_fp8_row.hpp, shared with the paged layer call's mirror writer).  Rows outside [t0, t1) are not touched.
// Paged form: source and destination are pools [n_pages, G, page_rows, D] / [n_pages, G, page_rows] under ONE table row; token r lives in row
// r & (page_rows - 1) of page table[r / page_rows] (nsa_paged_kv_quantize_fp8: page_rows = 1024, the selected branch's pages;
// nsa_paged_kv_quantize_fp8_rows: any power of two in [32, 65536], the band branches' -- 64 for K_cmp / V_cmp).  The page id is tested against
// [0, n_pages) before any address is formed from it and a row whose entry fails is skipped, as the paged copy kernels do (paged_kv_copy.hip).
#include "kv_quantize_fp8_row.hpp"
#include "nsa_common.hpp"
#include "nsa_internal.hpp"
#include "sel_attn_params.hpp"

namespace nsa {

struct KvQuantParams {
    const __bf16 *X;
    unsigned char *Q8;
    float *scale;
    int64_t xsb, xsg, xss, qsb, qsg, qss, zsb, zsg;  // element strides: batch (or page), group, row; the scale's rows are contiguous
    int G, t0, t1;
    int64_t planes;               // B G (paged: G)
    const int32_t *table_row;     // paged: device [max_pages]; null: contiguous tensors
    int n_pages, max_pages;
    int page_shift;               // paged: log2(page_rows)
};

template <int D>
__global__ __launch_bounds__(256) void kv_quantize_fp8_kernel(KvQuantParams P) {
    constexpr int LPR = D / 8, RPW = 64 / LPR;  // lanes per row, rows per wave
    const int lane = threadIdx.x & 63, sub = lane % LPR;
    const int64_t rows = (int64_t)P.t1 - P.t0;
    const int64_t idx = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;  // (plane, row) of this lane's row
    if (idx >= P.planes * rows) return;
    const int64_t plane = idx / rows;
    int64_t r = P.t0 + idx % rows;
    int64_t b = plane / P.G;
    const int g = (int)(plane % P.G);
    if (P.table_row) {
        const int64_t j = r >> P.page_shift;
        if (j >= P.max_pages) return;
        const int page = P.table_row[j];
        if (page < 0 || page >= P.n_pages) return;  // no page, or a bad id: the row is skipped
        b = page;
        r &= ((int64_t)1 << P.page_shift) - 1;
    }
    kv_quantize_fp8_row<D>(P.X + b * P.xsb + g * P.xsg + r * P.xss, P.Q8 + b * P.qsb + g * P.qsg + r * P.qss, P.scale + b * P.zsb + g * P.zsg + r, sub);
}

static int kv_quantize_launch(const char *who, const KvQuantParams &P, int D, void *stream) {
    NSA_CHECK_ARG(D == 64 || D == 128, "%s: D = %d, the head dimension must be 64 or 128", who, D);
    NSA_CHECK_ARG(P.G >= 1 && P.planes >= 0, "%s: bad sizes", who);
    NSA_CHECK_ARG(P.t0 >= 0 && P.t1 >= P.t0, "%s: need 0 <= t0 <= t1 (got [%d, %d))", who, P.t0, P.t1);
    const int64_t n = P.planes * ((int64_t)P.t1 - P.t0);
    if (n == 0) return NSA_OK;
    NSA_CHECK_ARG(P.X && P.Q8 && P.scale, "%s: null pointer", who);
    NSA_CHECK_ARG((uintptr_t)P.X % 16 == 0 && P.xsb % 8 == 0 && P.xsg % 8 == 0 && P.xss % 8 == 0 && P.xss >= D,
                  "%s: the bf16 source must be 16-byte aligned with strides in multiples of 8 elements", who);
    NSA_CHECK_ARG((uintptr_t)P.Q8 % 8 == 0 && P.qsb % 8 == 0 && P.qsg % 8 == 0 && P.qss % 8 == 0 && P.qss >= D,
                  "%s: the fp8 destination must be 8-byte aligned with strides in multiples of 8 bytes", who);
    NSA_CHECK_ARG((uintptr_t)P.scale % 4 == 0, "%s: the scale tensor must be 4-byte aligned (fp32, unit row stride)", who);
    const int rpb = 4 * (64 / (D / 8));  // rows of a 256-thread workgroup
    const int64_t grid = (n + rpb - 1) / rpb;
    NSA_CHECK_ARG(grid < ((int64_t)1 << 31), "%s: too many rows", who);
    if (D == 64) hipLaunchKernelGGL(kv_quantize_fp8_kernel<64>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(kv_quantize_fp8_kernel<128>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, P);
    NSA_LAUNCH_CHECK("kv_quantize_fp8_kernel");
    return NSA_OK;
}

}  // namespace nsa

using namespace nsa;

extern "C" {

int nsa_kv_quantize_fp8(const void *X, void *X8, float *scale, int B, int G, int S, int D, int t0, int t1, int64_t xsb, int64_t xsg, int64_t xss, int64_t qsb,
                        int64_t qsg, int64_t qss, int64_t zsb, int64_t zsg, void *stream) {
    NSA_CHECK_ARG(B >= 0 && S >= 0 && t1 <= S, "kv_quantize_fp8: rows [t0, t1) = [%d, %d) must lie inside the S = %d rows of the tensors", t0, t1, S);
    const KvQuantParams P{(const __bf16 *)X, (unsigned char *)X8, scale, xsb, xsg, xss, qsb, qsg, qss, zsb, zsg, G, t0, t1, (int64_t)B * G, nullptr, 0, 0, 0};
    return kv_quantize_launch("kv_quantize_fp8", P, D, stream);
}

int nsa_paged_kv_quantize_fp8_rows(const void *X_pool, void *X8_pool, float *scale_pool, const int32_t *table_row, int n_pages, int max_pages, int page_rows, int G,
                                   int D, int t0, int t1, int64_t xsp, int64_t xsg, int64_t xss, int64_t qsp, int64_t qsg, int64_t qss, int64_t zsp, int64_t zsg,
                                   void *stream) {
    NSA_CHECK_ARG(page_rows >= 32 && page_rows <= 65536 && (page_rows & (page_rows - 1)) == 0,
                  "paged_kv_quantize_fp8: page_rows = %d, must be a power of two in [32, 65536]", page_rows);
    NSA_CHECK_ARG(n_pages >= 1 && max_pages >= 1 && max_pages <= (1 << 20), "paged_kv_quantize_fp8: n_pages >= 1 and max_pages in [1, 2^20] (got %d, %d)", n_pages,
                  max_pages);
    NSA_CHECK_ARG((int64_t)t1 <= (int64_t)max_pages * page_rows, "paged_kv_quantize_fp8: t1 = %d is beyond the table's max_pages * %d = %lld tokens", t1, page_rows,
                  (long long)max_pages * page_rows);
    NSA_CHECK_ARG(table_row && (uintptr_t)table_row % 4 == 0, "paged_kv_quantize_fp8: the table row must be a 4-byte aligned device pointer");
    const KvQuantParams P{(const __bf16 *)X_pool, (unsigned char *)X8_pool, scale_pool, xsp, xsg, xss, qsp, qsg, qss, zsp, zsg, G, t0, t1, (int64_t)G, table_row,
                          n_pages, max_pages, __builtin_ctz((unsigned)page_rows)};
    return kv_quantize_launch("paged_kv_quantize_fp8", P, D, stream);
}

int nsa_paged_kv_quantize_fp8(const void *X_pool, void *X8_pool, float *scale_pool, const int32_t *table_row, int n_pages, int max_pages, int G, int D, int t0,
                              int t1, int64_t xsp, int64_t xsg, int64_t xss, int64_t qsp, int64_t qsg, int64_t qss, int64_t zsp, int64_t zsg, void *stream) {
    return nsa_paged_kv_quantize_fp8_rows(X_pool, X8_pool, scale_pool, table_row, n_pages, max_pages, DEC_PAGE_TOKENS, G, D, t0, t1, xsp, xsg, xss, qsp, qsg, qss, zsp,
                                          zsg, stream);
}

}  // extern "C"
