// The fused MFMA selection scorers (sel_scores_mfma.hip: 16x16x32 tiles, every group size; sel_scores_mfma32.hip: 32x32x16 tiles, h = 6 and
// D = 64): the 32x32 form's host interface, and the device pieces of the two-sweep algorithm that do not depend on the tile shape --
// kcmp_tile_offsets / _load / _store (a 64-row K_cmp tile -> registers -> LDS), wg_first_query, sweep_bounds, sweep2_last_block and
// sweep1_exact (the rare exact online-softmax update).  The tile shape, the fast-path exponent loops, the lane-group merges, the whole second
// sweep and the SEL epilogue stay with each kernel: the two second sweeps are different algorithms.
#pragma once
#include "nsa_common.hpp"
#include "sel_scores_params.hpp"

namespace nsa {

// h = 6, D = 64, 32-bit output offsets: the 32x32x16 form (sel_scores_mfma32.hip)
bool scores_mfma32_supported(const ScoresMfmaParams &P, int Dk);
// sel != null: the workgroup also selects the ranges of its 64 query rows, right behind its second sweep (the scores it reads back are
// the ones it has just written: L2 hits), so the step needs no select launch; needs S_sel <= 1024 and at most 64 ranges per row
bool scores_mfma32_select_supported(const ScoresMfmaParams &P, int Dk, const SelectParams &SP);
int launch_scores_mfma32(const ScoresMfmaParams &P, int dtype, hipStream_t st, const SelectParams *sel = nullptr);

#ifdef __HIPCC__
// ---- K_cmp of one (b,g) as the source of 64-row tiles for a workgroup of 256 threads: thread -> NLD (row, 16-B piece) pairs per tile, pair i =
// (row, piece) of p = tid + 256 i.  The kernel owns the arrays (stg: the tile in flight, toff: the offsets of a full tile).
template <int D>
struct KcmpTile {
    static constexpr int ROWB = D * 2, PIECES = D / 8, TILE_ROWS = 64, TILE_BYTES = TILE_ROWS * ROWB;
    static constexpr int NLD = TILE_ROWS * PIECES / 256;  // 16-B pieces per thread per tile
    static constexpr int LOGP = D == 64 ? 3 : 4;
};
// full tiles: one scalar base per tile + a lane-constant 32-bit offset (the per-lane 64-bit row arithmetic with its clamp was 16 VALU
// instructions per tile and wave in a kernel bound by instruction issue); only the last, padded tile clamps its rows
template <typename T, int D>
__device__ __forceinline__ void kcmp_tile_offsets(const ScoresMfmaParams &P, int tid, unsigned (&toff)[KcmpTile<D>::NLD], bool &small_stride) {
    using K_ = KcmpTile<D>;
#pragma unroll
    for (int i = 0; i < K_::NLD; ++i) {
        const int p = tid + 256 * i;
        toff[i] = (unsigned)((p / K_::PIECES) * (int)P.css + (p % K_::PIECES) * 8) * (unsigned)sizeof(T);
    }
    small_stride = P.css * (int64_t)K_::TILE_ROWS * (int64_t)sizeof(T) < ((int64_t)1 << 31);
}
template <typename T, int D>
__device__ __forceinline__ void kcmp_tile_load(const ScoresMfmaParams &P, const T *Kc, int tid, const unsigned (&toff)[KcmpTile<D>::NLD], bool small_stride,
                                               int tile, u32x4 (&stg)[KcmpTile<D>::NLD]) {
    using K_ = KcmpTile<D>;
    if (small_stride && (tile + 1) * K_::TILE_ROWS <= P.S_cmp) {
        const unsigned char *base = (const unsigned char *)(Kc + (int64_t)tile * K_::TILE_ROWS * P.css);  // wave uniform
#pragma unroll
        for (int i = 0; i < K_::NLD; ++i) stg[i] = *(const u32x4 *)(base + toff[i]);
        return;
    }
#pragma unroll
    for (int i = 0; i < K_::NLD; ++i) {
        const int p = tid + 256 * i;
        const int r = p / K_::PIECES, pc = p % K_::PIECES;
        const int row = min(tile * K_::TILE_ROWS + r, P.S_cmp - 1);
        stg[i] = *(const u32x4 *)(Kc + (int64_t)row * P.css + pc * 8);
    }
}
// into one buffer of the LDS double buffer: piece pc of row r lands at piece pc ^ ((r >> SWZ_SHIFT) & SWZ_MASK) of its LDS row (the form's
// bank swizzle; 0, PIECES - 1 is Geo<D>::row_piece of attn_mfma_tiles.hpp)
template <int D, int SWZ_SHIFT, int SWZ_MASK>
__device__ __forceinline__ void kcmp_tile_store(int tid, const u32x4 (&stg)[KcmpTile<D>::NLD], unsigned char *buf) {
    using K_ = KcmpTile<D>;
#pragma unroll
    for (int i = 0; i < K_::NLD; ++i) {
        const int p = tid + 256 * i;
        const int r = p >> K_::LOGP, pc = (p & (K_::PIECES - 1));
        *(u32x4 *)(buf + r * K_::ROWB + ((pc ^ ((r >> SWZ_SHIFT) & SWZ_MASK)) << 4)) = stg[i];
    }
}

// First query of this workgroup of QW queries.  Late query tiles first: with causal_skip the second sweep of a tile grows with its position (a
// tile at the end of a 64k sequence does 1.5x the work of the first one), and the dispatcher hands out workgroups in index order -- longest
// first keeps the tail short
__device__ __forceinline__ int wg_first_query(const ScoresMfmaParams &P, int QW) {
    return (P.causal_skip ? (int)(gridDim.x - 1 - blockIdx.x) : (int)blockIdx.x) * QW;
}
// What bounds the sweeps of the workgroup whose QW queries start at t0, for the wave whose queries start at tw
struct SweepBounds {
    int ntiles, ntiles1;    // 64-row tiles of K_cmp / of the first sweep
    int nc_wmin, nc_wgmax;  // NORM: visible columns of the wave's first query (its smallest bound) and of the workgroup's last (its largest)
};
template <bool NORM>
__device__ __forceinline__ SweepBounds sweep_bounds(const ScoresMfmaParams &P, int t0, int QW, int tw) {
    SweepBounds s;
    s.ntiles = (P.S_cmp + 63) / 64;
    s.nc_wmin = s.nc_wgmax = P.S_cmp;
    if constexpr (NORM) {
        s.nc_wmin = ncmp_at(P.q0 + min(tw, P.S - 1), P.l, P.d_stride, P.S_cmp);
        s.nc_wgmax = ncmp_at(P.q0 + min(t0 + QW, P.S) - 1, P.l, P.d_stride, P.S_cmp);
    }
    s.ntiles1 = NORM ? (s.nc_wgmax + 63) / 64 : s.ntiles;  // tiles of the first sweep
    return s;
}
// last selection block the workgroup has to produce: with causal_skip the second sweep stops at the last block any of its queries may select
// ((j+1) l' <= t+1); blocks beyond are never read by the selector.  Called where the second sweep begins.
template <bool NORM>
__device__ __forceinline__ int sweep2_last_block(const ScoresMfmaParams &P, int t0, int QW, int nc_wgmax) {
    const int l_sel = 4 * P.d_stride;
    int jlast = P.S_sel - 1;
    if (P.causal_skip) {
        const int t_last = P.q0 + min(t0 + QW, P.S) - 1;  // absolute position of the workgroup's last query
        jlast = min(jlast, (t_last + 1) / l_sel - 1);
    }
    if constexpr (NORM) jlast = min(jlast, nc_wgmax / 4);  // later blocks have no visible tap (block j's first tap is column 4j - 1)
    return jlast;
}

// The exact update of a lane's running max / sum (exp2 domain) by its 16 logits logit(0..15) of one column tile; rows row_of(i) >= rv are
// padding or, under NORM, past the lane column's own bound.  Returns the tile's sum relative to the new max (the caller adds it to lrun).
template <bool NORM, class Logit, class RowOf>
__device__ __forceinline__ float sweep1_exact(const Logit &logit, const RowOf &row_of, int rv, float c2, float &mrun, float &lrun) {
    asm volatile("; sweep-1 slow path" ::: "memory");
    // rv enters through an (empty) asm, as the logits below: the 16 row masks belong to this block
    if constexpr (NORM) asm volatile("" : "+v"(rv));  // per lane column
    else asm volatile("" : "+s"(rv));
    float v[16];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        // the logit enters this block through an (empty) asm: without it the compiler evaluates the masks, products and maxima
        // of this rare path ahead of the branch, on every tile (90 of 255 VALU instructions of the common path)
        float a = logit(i);
        asm volatile("" : "+v"(a));
        const float x = (row_of(i) < rv) ? a * c2 : -INFINITY;
        v[i] = x;
        mx = fmaxf(mx, x);
    }
    const float mnew = fmaxf(mrun, mx);
    float sum = 0.f;
    if (mnew > -INFINITY) {  // a lane (group) may see only padding rows in the last tile
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += __builtin_amdgcn_exp2f(v[i] - mnew);
        lrun = lrun * __builtin_amdgcn_exp2f(mrun - mnew);
        mrun = mnew;
    }
    return sum;
}
#endif  // __HIPCC__

}  // namespace nsa
