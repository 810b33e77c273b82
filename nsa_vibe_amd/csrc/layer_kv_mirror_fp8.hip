// layer_kv_mirror_fp8_paged_kernel: the FP8 (e4m3) mirror writer of nsa_layer_decode_paged_fp8.  ONE launch behind the append and the pooling
// of the paged layer call, on their stream: for every live sequence it quantises the rows those two launches have just written --
//   token rows pos = t_live[b] .. t_live[b] + S - 1 of K_sel, V_sel, K_win, V_win   -> row pos & 1023 of page table[b][pos >> 10]
//   compressed rows j in [n_cmp(t_live[b]), n_cmp(t_live[b] + S)) of K_cmp, V_cmp   -> row j & 63 of page table[b][j >> 6]
// -- into six e4m3 pools of the bf16 pools' shape and six fp32 scale pools, so that the FP8 readers behind it (dstep_kernel_fp8, the FP8 band
// kernels) find the mirrors current without the host ever reading a position or the table.  K_raw / V_raw have no mirror (pooling reads bf16).
// Work split.  The host knows B, S and G, not the positions: the grid is 3 B workgroups of four waves, workgroup (b, pair) with pair = sel,
// win or cmp.  The K and the V pool of a pair share rows AND page ids, so the pair's one or two table entries are fetched once; waves 0 / 1
// take the K pool, waves 2 / 3 the V pool.  Inside a pool a row is D / 8 lanes (kv_quantize_fp8_row.hpp: the quantiser's row function, the
// same bits), a wave takes 64 / (D / 8) rows (g, r) at once and the two waves of a pool stride over its (r1 - r0) G rows: at most 16 G token
// rows, 2 G compressed ones.  A workgroup leaves whole, before the barrier, where its sequence is not live or (cmp) no window completes.
// Page ids.  Lanes 0 and 1 of wave 0 fetch the entries of the first and the last row, test each against [0, n_pages) and leave the verdict
// (the id, or -1) in LDS; every address is formed from a verdict, and a row behind a failed entry is skipped -- the rule of the paged kernels.
// Stores: one 8-byte vector store per lane and one fp32 store per row, plain C++.
#include "kv_quantize_fp8_row.hpp"
#include "layer_fused.hpp"
#include "nsa_common.hpp"
#include "nsa_internal.hpp"

namespace nsa {

template <int D>
__global__ __launch_bounds__(256) void layer_kv_mirror_fp8_paged_kernel(KvMirrorFp8PagedParams P) {
    constexpr int LPR = D / 8, RPW = 64 / LPR;  // lanes per row, rows per wave
    __shared__ int page_of[2];                  // the verdicts of the first and the last row's table entries: a page id inside [0, n_pages), or -1
    const int b = (int)(blockIdx.x / 3), pair = (int)(blockIdx.x - 3 * b);
    const int t0 = P.t_pos[b];  // (one scalar load: b is uniform)
    if (t0 < 0 || t0 > P.te - (P.S - 1)) return;  // not live: the whole workgroup, before the barrier
    auto ncmp = [](int n) { return n < 32 ? 0 : (n - 32) / 16 + 1; };  // compressed tokens of n cached ones (l = 32, d = 16: ncmp_of)
    const bool cmp = pair == 2;
    const int shift = cmp ? 6 : 10;  // log2 of the pair's page rows (LAYER_PAGE_CMP / LAYER_PAGE_TOKENS)
    const int r0 = cmp ? ncmp(t0) : t0, r1 = cmp ? ncmp(t0 + P.S) : t0 + P.S;
    if (r1 <= r0) return;  // no window completes inside the call's rows
    const int e0 = r0 >> shift, e1 = (r1 - 1) >> shift;  // r1 - r0 <= 16: at most two pages
    if (threadIdx.x < 2) {
        const int e = threadIdx.x ? e1 : e0;
        int page = -1;
        if (e < P.pg.max_pages) {
            page = P.pg.table[(int64_t)b * P.pg.stride + e];
            if (page < 0 || page >= P.pg.n_pages) page = -1;
        }
        page_of[threadIdx.x] = page;
    }
    __syncthreads();
    const int p0 = page_of[0], p1 = page_of[1];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, sub = lane % LPR;
    const int kv = wave >> 1;  // 0: the K pool, 1: the V pool
    const __bf16 *X = (const __bf16 *)(kv ? P.src[pair][1] : P.src[pair][0]);
    unsigned char *Q8 = kv ? P.q8[pair][1] : P.q8[pair][0];
    float *Z = kv ? P.scale[pair][1] : P.scale[pair][0];
    const int nr = r1 - r0, n = nr * P.G, mask = (1 << shift) - 1;
    for (int base = (wave & 1) * RPW; base < n; base += 2 * RPW) {
        const int idx = base + lane / LPR;  // (g, r) of this lane's row: the D / 8 lanes of a row stay together
        if (idx >= n) continue;
        const int g = idx / nr, r = r0 + idx - g * nr;
        const int page = (r >> shift) == e0 ? p0 : p1;
        if (page < 0) continue;  // a failed entry: the row is skipped
        const int64_t row = ((((int64_t)page * P.G + g) << shift) + (r & mask));  // (formed in 64 bits: a pool may exceed 2 GiB)
        kv_quantize_fp8_row<D>(X + row * D, Q8 + row * D, Z + row, sub);
    }
}

int launch_kv_mirror_fp8_paged(const KvMirrorFp8PagedParams &P, int D, hipStream_t st) {
    const char *who = "kv_mirror_fp8(paged)";
    NSA_CHECK_ARG(D == 64 || D == 128, "%s: D = %d, the head dimension must be 64 or 128", who, D);
    NSA_CHECK_ARG(P.B >= 1 && P.S >= 1 && P.S <= 16 && P.G >= 1 && P.te >= 0, "%s: bad sizes", who);
    NSA_CHECK_ARG(P.t_pos && P.pg.table && P.pg.n_pages >= 1 && P.pg.max_pages >= 1 && P.pg.stride >= P.pg.max_pages,
                  "%s: positions, a block table and n_pages >= 1", who);
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 2; ++k) {
            NSA_CHECK_ARG(P.src[i][k] && P.q8[i][k] && P.scale[i][k], "%s: null pool pointer", who);
            NSA_CHECK_ARG((uintptr_t)P.src[i][k] % 16 == 0 && (uintptr_t)P.q8[i][k] % 16 == 0 && (uintptr_t)P.scale[i][k] % 4 == 0,
                          "%s: the bf16 and the e4m3 pools must be 16-byte aligned, the scale pools 4-byte aligned", who);
        }
    NSA_CHECK_ARG((int64_t)P.B * 3 < ((int64_t)1 << 31), "%s: too many sequences", who);
    const dim3 grid((unsigned)(P.B * 3));
    if (D == 64) hipLaunchKernelGGL(layer_kv_mirror_fp8_paged_kernel<64>, grid, dim3(256), 0, st, P);
    else hipLaunchKernelGGL(layer_kv_mirror_fp8_paged_kernel<128>, grid, dim3(256), 0, st, P);
    NSA_LAUNCH_CHECK("layer_kv_mirror_fp8_paged_kernel");
    return NSA_OK;
}

// layer_kv_mirror_fp8_ragged_kernel: the mirror writer of nsa_layer_decode_ragged_fp8 -- the same rows of contiguous slabs, row r of plane
// (b, g) at (b G + g) rows + r.  No table, so nothing is shared between the rows of a sequence: no LDS, no barrier, and the work is dealt
// out by ROW instead of by (sequence, pair).  A sequence has at most I = G (4 S + 2 CM) rows to quantise -- S token rows of four slabs and
// CM = ceil(S / 16) compressed rows of two (n_cmp advances by at most that over S tokens) -- in that fixed order (slab, g, row), so the rows a
// wave takes together are consecutive rows of one plane wherever S allows: contiguous loads and stores.  A wave takes 64 / (D / 8) of them,
// a sequence ceil(I / rows per wave) waves, and the waves of all sequences are packed four to a workgroup: B = 256, S = 1, G = 4, D = 64 is
// 192 full workgroups where a workgroup per (sequence, pair) would launch 768 mostly idle ones.  A wave belongs to ONE sequence, so the
// position is one scalar load and the liveness test is wave uniform; the slab pointers are indexed per lane from the argument block.
template <int D>
__global__ __launch_bounds__(256) void layer_kv_mirror_fp8_ragged_kernel(KvMirrorFp8RaggedParams P, int wps) {
    constexpr int LPR = D / 8, RPW = 64 / LPR;  // lanes per row, rows per wave
    const int wid = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
    const int b = wid / wps;
    if (b >= P.B) return;
    const int t0 = P.t_pos[b];
    if (t0 < 0 || t0 > P.te - (P.S - 1)) return;  // not live: the whole wave
    auto ncmp = [](int n) { return n < 32 ? 0 : (n - 32) / 16 + 1; };  // compressed tokens of n cached ones (l = 32, d = 16: ncmp_of)
    const int n0 = ncmp(t0), nc = ncmp(t0 + P.S) - n0;
    const int CM = (P.S + 15) / 16, per_tok = P.G * P.S, per_cmp = P.G * CM;
    const int idx = (wid - b * wps) * RPW + lane / LPR;  // the D / 8 lanes of a row stay together
    int slab, g, row, rows;
    if (idx < 4 * per_tok) {
        slab = idx / per_tok;
        const int rem = idx - slab * per_tok;
        g = rem / P.S;
        row = t0 + rem - g * P.S;  // <= te < S_max
        rows = P.S_max;
    } else {
        const int j = idx - 4 * per_tok;
        if (j >= 2 * per_cmp) return;  // behind the sequence's last row
        const int pair = j / per_cmp, rem = j - pair * per_cmp;
        slab = 4 + pair;
        g = rem / CM;
        const int r = rem - g * CM;
        if (r >= nc) return;  // no window completes for this slot
        row = n0 + r;  // < n_cmp(te + 1) <= n_cmp_max
        rows = P.n_cmp_max;
    }
    const int64_t at = ((int64_t)b * P.G + g) * rows + row;  // (formed in 64 bits: a slab may exceed 2 GiB)
    kv_quantize_fp8_row<D>((const __bf16 *)P.src[slab] + at * D, P.q8[slab] + at * D, P.scale[slab] + at, lane % LPR);
}

int launch_kv_mirror_fp8_ragged(const KvMirrorFp8RaggedParams &P, int D, hipStream_t st) {
    const char *who = "kv_mirror_fp8(ragged)";
    NSA_CHECK_ARG(D == 64 || D == 128, "%s: D = %d, the head dimension must be 64 or 128", who, D);
    NSA_CHECK_ARG(P.B >= 1 && P.S >= 1 && P.S <= 16 && P.G >= 1 && P.S_max >= 1 && P.n_cmp_max >= 1 && P.te >= 0 && P.te < P.S_max, "%s: bad sizes", who);
    // (the kernel's row bounds: a live row sits at most at te < S_max, and every compressed row it may emit is held)
    NSA_CHECK_ARG(P.n_cmp_max >= (P.te + 1 < 32 ? 0 : (P.te + 1 - 32) / 16 + 1), "%s: compressed slabs too small for %d tokens", who, P.te + 1);
    NSA_CHECK_ARG(P.t_pos, "%s: null position array", who);
    for (int i = 0; i < 6; ++i) {
        NSA_CHECK_ARG(P.src[i] && P.q8[i] && P.scale[i], "%s: null slab pointer", who);
        NSA_CHECK_ARG((uintptr_t)P.src[i] % 16 == 0 && (uintptr_t)P.q8[i] % 16 == 0 && (uintptr_t)P.scale[i] % 4 == 0,
                      "%s: the bf16 and the e4m3 slabs must be 16-byte aligned, the scale slabs 4-byte aligned", who);
    }
    const int rpw = 64 / (D / 8), items = P.G * (4 * P.S + 2 * ((P.S + 15) / 16));
    const int wps = (items + rpw - 1) / rpw;
    const int64_t waves = (int64_t)P.B * wps;
    NSA_CHECK_ARG(waves < ((int64_t)1 << 31), "%s: too many sequences", who);
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (D == 64) hipLaunchKernelGGL(layer_kv_mirror_fp8_ragged_kernel<64>, grid, dim3(256), 0, st, P, wps);
    else hipLaunchKernelGGL(layer_kv_mirror_fp8_ragged_kernel<128>, grid, dim3(256), 0, st, P, wps);
    NSA_LAUNCH_CHECK("layer_kv_mirror_fp8_ragged_kernel");
    return NSA_OK;
}

}  // namespace nsa
