// Query-tile schedule of the kernels in which ONE wave owns several consecutive query rows of one (b,g) and walks the UNION of their selected
// 32-key tiles (the forward sel_attn_rows_mfma.hip, the backward's bwd_dq_rows_kernel): a tile is brought into LDS once for all the rows and
// each row masks the keys it did not select.  Per wave: (1) the rows' ranges go to LDS, clamped; (2) two bitmaps per row over 32-key tiles --
// `touch` (some key of the tile selected) and `full` (a single range covers the whole tile) -- are built with LDS atomics, one (row, range)
// pair per lane; their OR over the rows is the tile schedule; (3) tiles are walked in ascending order; per tile the rows that own it in full /
// in part come out as wave-uniform masks, and the 32-key mask of a partially covered row is rebuilt from its ranges.  Union semantics of
// overlapping ranges (attention_kernels.py:721-732) fall out of the bitmaps: no sorting / merging of ranges is needed.
//
// Both kernels are sensitive to code generation, so two steps of (1) stay in the kernels, written against the members: the clear of the
// 2 * tpw * NW + 16 bitmap words from fullw on, and the clamp of a range to 0 <= s <= e <= S_kv with its store to rg[2 * (r * n + i)].  With
// either in a function here, the forward's instances changed their per-loop instruction counts.  For the same reason the methods with
// loops copy the members they use into locals first: a store through unsigned * may alias a member until the struct is in registers.
#pragma once
#include "nsa_common.hpp"

namespace nsa {

__device__ __forceinline__ unsigned bit_span(int lo, int hi) {  // bits lo..hi inclusive, 0 <= lo <= hi <= 31
    const unsigned up = hi >= 31 ? 0xffffffffu : ((1u << (hi + 1)) - 1u);
    return up & ~((1u << lo) - 1u);
}

__device__ __forceinline__ void lds_or(unsigned *p, unsigned v) {  // ds_or_b32: stays in the wave's in-order DS queue
    typedef __attribute__((address_space(3))) unsigned lds_u32;
    __hip_atomic_fetch_or((lds_u32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// bitmap words per row (32 tiles of 32 keys each) and the schedule's LDS bytes per wave: rg | fullw | touchw | kmask, behind the wave's tiles
inline int rows_sched_words(int S_kv) { return ((S_kv + 31) / 32 + 31) / 32; }
inline int rows_sched_bytes(int tpw, int n, int nw) { return 4 * (((2 * tpw * n + 3) & ~3) + ((2 * tpw * nw + 16 + 3) & ~3)); }

struct RowsSched {
    int *rg;           // [tpw][n][2] clamped ranges (written by the kernel)
    unsigned *fullw;   // [tpw][NW]; fullw | touchw | kmask are contiguous and cleared by the kernel
    unsigned *touchw;  // [tpw][NW]
    unsigned *kmask;   // [16]
    int tpw, n, NW, ntok;
    // union over the rows = the tile schedule; kept in registers (lane w holds word w, NW <= 128): walking it costs no LDS round trips
    unsigned u0 = 0u, u1 = 0u;
    unsigned long long nz0 = 0ull, nz1 = 0ull;
    int iw = 0;
    unsigned ibits = 0u;
    int cw = -1;  // lane r < ntok caches row r's bitmap words of the 32-tile group cw
    unsigned fw = 0u, tw = 0u;

    __device__ __forceinline__ RowsSched(unsigned char *lds, int tpw_, int n_, int NW_, int ntok_) : tpw(tpw_), n(n_), NW(NW_), ntok(ntok_) {
        rg = (int *)lds;
        fullw = (unsigned *)(rg + ((2 * tpw * n + 3) & ~3));
        touchw = fullw + tpw * NW;
        kmask = touchw + tpw * NW;
    }
    // the ranges are in LDS: tile bitmaps, one (row, range) pair per lane, and their union
    __device__ __forceinline__ void build(int lane) {
        const int *const rg = this->rg;
        unsigned *const fullw = this->fullw, *const touchw = this->touchw;
        const int n = this->n, NW = this->NW, ntok = this->ntok;
        unsigned u0 = 0u, u1 = 0u;
        wave_lds_fence();
        for (int p = lane; p < ntok * n; p += 64) {
            const int r = p / n;
            const int s = rg[2 * p], e = rg[2 * p + 1];
            if (e > s) {
                const int ta = s >> 5, tb = (e - 1) >> 5;         // tiles touched
                const int fa = (s + 31) >> 5, fb = (e >> 5) - 1;  // tiles covered completely: fa..fb
                for (int w = ta >> 5; w <= (tb >> 5); ++w) {
                    const int base = 32 * w;
                    lds_or(&touchw[r * NW + w], bit_span(max(ta, base) - base, min(tb, base + 31) - base));
                    const int flo = max(fa, base), fhi = min(fb, base + 31);
                    if (flo <= fhi) lds_or(&fullw[r * NW + w], bit_span(flo - base, fhi - base));
                }
            }
        }
        wave_lds_fence();
        for (int r = 0; r < ntok; ++r) {
            if (lane < NW) u0 |= touchw[r * NW + lane];
            if (lane + 64 < NW) u1 |= touchw[r * NW + 64 + lane];
        }
        this->u0 = u0, this->u1 = u1;
        nz0 = __ballot(u0 != 0u);
        nz1 = __ballot(u1 != 0u);
    }
    // next set bit of the union bitmap, ascending (wave-uniform scalars); -1 = done
    __device__ __forceinline__ int next_tile() {
        if (ibits == 0u) {
            if (nz0) {
                iw = __builtin_ctzll(nz0);
                nz0 &= nz0 - 1ull;
                ibits = (unsigned)__builtin_amdgcn_readlane((int)u0, iw);
            } else if (nz1) {
                const int w = __builtin_ctzll(nz1);
                nz1 &= nz1 - 1ull;
                ibits = (unsigned)__builtin_amdgcn_readlane((int)u1, w);
                iw = 64 + w;
            } else {
                return -1;
            }
        }
        const int bit = __builtin_ctz(ibits);
        ibits &= ibits - 1u;
        return 32 * iw + bit;
    }
    // ownership of tile cur, in two steps so that the LDS reads of the first join the fragment reads in front of the caller's lgkmcnt wait:
    // refresh() reloads the cached bitmap words once per 32-tile group, owners() gives bit r of fullm / touchm = row r covers the tile
    // completely / selected at least one of its keys
    __device__ __forceinline__ void refresh(int cur, int lane) {
        if ((cur >> 5) != cw) {
            cw = cur >> 5;
            if (lane < ntok) {
                fw = fullw[lane * NW + cw];
                tw = touchw[lane * NW + cw];
            }
        }
    }
    __device__ __forceinline__ void owners(int cur, unsigned &fullm, unsigned &touchm) const {
        fullm = (unsigned)__ballot((fw >> (cur & 31)) & 1u);
        touchm = (unsigned)__ballot((tw >> (cur & 31)) & 1u);
    }
    // kmask[r] = the 32-key mask of the tile at key tok0 for every row r of partm (rows that cover it in part), from their ranges
    __device__ __forceinline__ void rebuild_kmask(unsigned partm, int tok0, int lane) {
        const int *const rg = this->rg;
        unsigned *const kmask = this->kmask;
        const int n = this->n, ntok = this->ntok;
        if (lane < 16) kmask[lane] = 0u;
        wave_lds_fence();
        for (int p = lane; p < ntok * n; p += 64) {
            const int r = p / n;
            const int lo = max(rg[2 * p], tok0) - tok0, hi = min(rg[2 * p + 1], tok0 + 32) - tok0;
            if (((partm >> r) & 1u) && hi > lo) lds_or(&kmask[r], bit_span(lo, hi - 1));
        }
        wave_lds_fence();
    }
};

}  // namespace nsa
