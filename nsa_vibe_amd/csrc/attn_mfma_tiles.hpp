// Pieces shared by the MFMA attention kernels (selection attention forward and backward, band attention) -- everything between a K/V
// pointer and the MFMA operands; schedule, softmax, masks, epilogue and the LDS carve-up stay with each kernel (the query-tile schedule of
// the two rows-per-wave kernels is attn_rows_schedule.hpp):
//   MfmaT<T>            MFMA / transposing-read wrappers per element type
//   Geo<D>              LDS tile geometry: row image and transposable image with their XOR swizzles (row_piece / tr_piece)
//   frag_read_offsets   a lane's fragment read offsets into the two images
//   load_col_frags      Q^T / dO^T column fragments from global memory, zeros for unused columns
//   read_row_frags, read_tr_frags   K row fragments / V^T fragments (the two 16-row halves paired) from LDS
//   kv_rsrc, KvSrc<D>, kv_src       K/V of one (b,g) as buffer resources + the per-lane and scalar offsets of its 32-key tiles
//   tile_dma            a tile -> LDS by LDS-DMA (full-tile arm with scalar steps, tail arm with the clamped row): the band forward's; the one-row
//                       and the rows kernel of the selection keep a copy each (they say why)
//   kv_plane, kv_page, paged_tile_dma2   paged K/V (the band forward's PAGED form): the 64-bit base of a (page, group) plane, the descriptors
//                       of a KvSrc on it, and a tile whose rows lie in two pages by LDS-DMA with per-lane global addresses
//   wg_pair             workgroup index -> ((b,g) pair, workgroup of the pair) under map_mode 0 / 1 / 2
//   PART_PAD, RESCALE_THR, sel_attn_combine_kernel   split-KV partial record and its combine kernel
#pragma once
#include "nsa_common.hpp"
#include "sel_attn_params.hpp"

namespace nsa {

template <typename T>
struct MfmaT;
template <>
struct MfmaT<__bf16> {
    using x8 = bf16x8;
    using x4 = bf16x4;
    __device__ static f32x4 mma(x8 a, x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    __device__ static x4 tr(const unsigned char *p) {
        return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) x4 *)p);
    }
};
template <>
struct MfmaT<_Float16> {
    using x8 = f16x8;
    using x4 = f16x4;
    __device__ static f32x4 mma(x8 a, x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    __device__ static x4 tr(const unsigned char *p) {
        typedef __attribute__((ext_vector_type(4))) short s16x4;
        const s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)p);
        return __builtin_bit_cast(x4, r);
    }
};

template <int D>
struct Geo {
    static constexpr int ROWB = D * 2;          // bytes per K/V row
    static constexpr int PIECES = D / 8;        // 16-B pieces per row
    static constexpr int RPI = 64 / PIECES;     // rows covered by one wave-wide 16-B load
    static constexpr int NLD = 32 / RPI;        // loads per operand per 32-key tile
    static constexpr int KSTEPS = D / 32;       // MFMA k-steps of the QK product
    static constexpr int MT = D / 16;           // 16-row dv tiles of the PV product
    static constexpr int TILE_BYTES = 32 * ROWB;
    static constexpr int SEG_BYTES = ((SEG_INTS * 4 + 15) / 16) * 16;
    static constexpr int WAVE_LDS = 2 * TILE_BYTES + SEG_BYTES;
    __device__ static int swz_k(int row) { return row & (PIECES - 1); }
    __device__ static int swz_v(int row) { return D == 64 ? ((row >> 1) & 3) : (row & 7); }
    // byte offset inside its row of the 16-B piece p of row `row`: in the row image (b128 fragment reads; the pieces are swizzled) and in the
    // transposable image (ds_read_tr; the 32-B chunks are swizzled, the two pieces of a chunk stay together).  Both swizzles are involutions
    // and invariant under +16 rows.
    __device__ static int row_piece(int row, int p) { return (p ^ swz_k(row)) << 4; }
    __device__ static int tr_piece(int row, int p) { return ((((p >> 1) ^ swz_v(row)) << 1) | (p & 1)) << 4; }
    __device__ static uint32_t row_img(int row, int p) { return row * ROWB + row_piece(row, p); }  // ... and inside the image
    __device__ static uint32_t tr_img(int row, int p) { return row * ROWB + tr_piece(row, p); }
};

// fragment read offsets of lane (rho, q) = (lane & 15, lane >> 4) inside a 16-row half of a tile: the b128 reads of a row image take row rho,
// pieces 4 s + q; the transposing reads of a transposable image take row 4 q + rho / 4, chunk m, 8 bytes at 8 (rho & 3)
template <int D>
__device__ __forceinline__ void frag_read_offsets(int rho, int q, uint32_t (&row_rd)[Geo<D>::KSTEPS], uint32_t (&tr_rd)[Geo<D>::MT]) {
    using G_ = Geo<D>;
#pragma unroll
    for (int s = 0; s < G_::KSTEPS; ++s) row_rd[s] = rho * G_::ROWB + G_::row_piece(rho, 4 * s + q);
    const int r = 4 * q + (rho >> 2);
#pragma unroll
    for (int m = 0; m < G_::MT; ++m) tr_rd[m] = r * G_::ROWB + G_::tr_piece(r, 2 * m) + 8 * (rho & 3);
}

// column fragments (B operand: Q^T, dO^T): the lane holds row[32 s + 8 q .. + 7] of its column's (query row, head); an unused column holds zeros
template <int D, typename X8, typename T>
__device__ __forceinline__ void load_col_frags(const T *row, bool used, int q, X8 (&f)[D / 32]) {
#pragma unroll
    for (int s = 0; s < D / 32; ++s) {
        u32x4 raw = {0u, 0u, 0u, 0u};
        if (used) raw = *(const u32x4 *)(row + 32 * s + 8 * q);
        f[s] = __builtin_bit_cast(X8, raw);
    }
}
// row fragments (A operand of S^T = K . Q^T) of the U 16-row halves of a row image
template <int D, int U, typename X8>
__device__ __forceinline__ void read_row_frags(const unsigned char *img, const uint32_t (&rd)[D / 32], X8 (&fr)[U][D / 32]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int s = 0; s < D / 32; ++s) fr[u][s] = *(const X8 *)(img + rd[s] + u * 16 * Geo<D>::ROWB);
}
// transposed fragments (A operand of O^T += V^T . P^T) of 32 rows of a transposable image: the transposing reads of the two 16-row halves,
// paired into one x8 whose k index j < 4 is row 4 q + j and j >= 4 row 16 + 4 q + j - 4 -- the key order of the S^T accumulators
template <typename T, int D>
__device__ __forceinline__ void read_tr_frags(const unsigned char *img, const uint32_t (&rd)[D / 16], typename MfmaT<T>::x8 (&fr)[D / 16]) {
#pragma unroll
    for (int m = 0; m < D / 16; ++m) {
        const typename MfmaT<T>::x4 lo = MfmaT<T>::tr(img + rd[m]), hi = MfmaT<T>::tr(img + rd[m] + 16 * Geo<D>::ROWB);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fr[m][j] = lo[j];
            fr[m][4 + j] = hi[j];
        }
    }
}

// K/V of one (b,g) as a buffer resource: loads are `buffer_load_dwordx4 v, voffset(VGPR), srsrc, soffset(SGPR)` -- the per-tile part of the
// address is scalar, the per-lane part a loop-invariant VGPR: no VALU address math.  The descriptor is built from wave-uniform values only
// (readfirstlane'd halves), so no waterfall loop is emitted.
__device__ __forceinline__ auto kv_rsrc(const unsigned char *base, int64_t bytes) {
    const uint64_t a = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), (short)0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}

// K/V of one (b,g) as the source of 32-key tiles.  One wave-wide 16-B load covers RPI rows (lane l: piece l % PIECES of row l / PIECES).
// The wave-uniform members are readfirstlane'd: that pins them in SGPRs (a soffset the compiler keeps in a VGPR costs a waterfall loop per load).
template <int D>
struct KvSrc {
    __amdgpu_buffer_rsrc_t krs, vrs;
    int krowb, vrowb;      // row pitch in bytes
    int kstep, vstep;      // RPI rows in bytes
    int ld_row, ld_piece;  // this lane's row and piece within one wave-wide load
    // LDS-DMA: lane l of load i lands at tile + i * 1 KiB + 16 l, i.e. row i * RPI + ld_row, stored piece ld_piece; it must fetch the source piece
    // that the swizzled image keeps at that position: offsets inside a full tile, K for a row image, V for a transposable image
    uint32_t kdma[Geo<D>::NLD], vdma[Geo<D>::NLD];
};
template <typename T, int D, class A>  // A: SelAttnParams, SelAttnBwdParams or BandAttnParams
__device__ __forceinline__ KvSrc<D> kv_src(const A &P, int b, int g, int lane) {
    using G_ = Geo<D>;
    const unsigned char *Kb = (const unsigned char *)((const T *)P.K + (int64_t)b * P.ksb + (int64_t)g * P.ksg);
    const unsigned char *Vb = (const unsigned char *)((const T *)P.V + (int64_t)b * P.vsb + (int64_t)g * P.vsg);
    const int64_t krowb = P.kss * 2, vrowb = P.vss * 2;
    KvSrc<D> t;
    t.krs = kv_rsrc(Kb, (int64_t)(P.S_kv - 1) * krowb + G_::ROWB);
    t.vrs = kv_rsrc(Vb, (int64_t)(P.S_kv - 1) * vrowb + G_::ROWB);
    t.krowb = uniform((int)krowb), t.vrowb = uniform((int)vrowb);
    t.kstep = uniform(G_::RPI * (int)krowb), t.vstep = uniform(G_::RPI * (int)vrowb);
    t.ld_row = lane / G_::PIECES, t.ld_piece = lane % G_::PIECES;
#pragma unroll
    for (int i = 0; i < G_::NLD; ++i) {
        const int r = i * G_::RPI + t.ld_row;
        t.kdma[i] = (uint32_t)(t.ld_row * krowb + G_::row_piece(r, t.ld_piece));
        t.vdma[i] = (uint32_t)(t.ld_row * vrowb + G_::tr_piece(r, t.ld_piece));
    }
    return t;
}

// the 32-key tile at key tok0 -> the wave's K image kl (row image) and V image vl (transposable image) by LDS-DMA (buffer_load_dwordx4 ... lds,
// no VGPR / ds_write on the path; completion is a vmcnt event).  The XOR swizzle is applied on the per-lane SOURCE offset because the DMA
// destination is lane-linear.  full: the tile has 32 rows -- scalar tile base + i * RPI rows, the per-lane offsets are loop invariant; else
// the rows past `last` re-read row `last` (the caller masks them)
template <int D>
__device__ __forceinline__ void tile_dma(const KvSrc<D> &t, unsigned char *kl, unsigned char *vl, int tok0, bool full, int last) {
#if defined(__HIP_DEVICE_COMPILE__)  // hipcc's host pass drops the whole kernel stub if it sees this builtin
    using G_ = Geo<D>;
    typedef __attribute__((address_space(3))) void lds_void;
    const int ks = uniform(tok0 * t.krowb), vs = uniform(tok0 * t.vrowb);
    if (full) {
#pragma unroll
        for (int i = 0; i < G_::NLD; ++i) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(t.krs, (lds_void *)(kl + i * 1024), 16, t.kdma[i], ks + i * t.kstep, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(t.vrs, (lds_void *)(vl + i * 1024), 16, t.vdma[i], vs + i * t.vstep, 0, 0);
        }
    } else {
#pragma unroll
        for (int i = 0; i < G_::NLD; ++i) {
            const int r = i * G_::RPI + t.ld_row;
            const int rc = min(r, last);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(t.krs, (lds_void *)(kl + i * 1024), 16, rc * t.krowb + G_::row_piece(r, t.ld_piece), ks, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(t.vrs, (lds_void *)(vl + i * 1024), 16, rc * t.vrowb + G_::tr_piece(r, t.ld_piece), vs, 0, 0);
        }
    }
#endif
}

// Paged K/V (the band forward's PAGED form): the pools are [n_pages, G, rows, D] with P.ksb / P.vsb as PAGE strides.  The base of a
// (page, group) plane is formed in 64 bits -- a pool may exceed 2 GiB --; the 32-bit offsets stay inside one plane of `rows` rows (the host
// bounds rows * row stride).  `page` is a checked table entry, wave uniform.
template <typename T>
__device__ __forceinline__ const unsigned char *kv_plane(const void *pool, int64_t page_stride, int64_t group_stride, int page, int g) {
    const uint64_t a = (uint64_t)((const T *)pool + (int64_t)page * page_stride + (int64_t)g * group_stride);
    // (wave uniform by construction: pinned in SGPRs, so a lane's choice between two planes is one select per half, not a 64-bit multiply)
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return (const unsigned char *)(((uint64_t)hi << 32) | lo);
}
// the descriptors of t on the plane of `page`: tile_dma then takes the row INSIDE the page as tok0
template <typename T, int D, class A>
__device__ __forceinline__ void kv_page(KvSrc<D> &t, const A &P, int page, int g, int rows) {
    t.krs = kv_rsrc(kv_plane<T>(P.K, P.ksb, P.ksg, page, g), (int64_t)(rows - 1) * t.krowb + Geo<D>::ROWB);
    t.vrs = kv_rsrc(kv_plane<T>(P.V, P.vsb, P.vsg, page, g), (int64_t)(rows - 1) * t.vrowb + Geo<D>::ROWB);
}
// A 32-key tile whose rows lie in TWO pages (p0: rows row0 .. rows - 1 of it, p1: the rest from its row 0): a buffer descriptor is wave
// uniform, so this arm gives every lane its own 64-bit source address -- one of the two wave-uniform plane bases by the lane's row, the row
// offset and the swizzled piece offset of tile_dma's tail arm -- through global_load_lds_dwordx4.  The destination is lane-linear like the
// buffer form's, so the LDS image is byte-identical, and completion is a vmcnt event like the buffer form's.  Rows past `last` re-read row
// `last` (clamped first, then the page of the clamped row: nothing beyond the wave's last key is read).
template <typename T, int D, class A>
__device__ __forceinline__ void paged_tile_dma2(const KvSrc<D> &t, const A &P, int p0, int p1, int g, unsigned char *kl, unsigned char *vl, int row0,
                                                int rows, int last) {
#if defined(__HIP_DEVICE_COMPILE__)  // (device-only builtin, like tile_dma's)
    using G_ = Geo<D>;
    typedef __attribute__((address_space(3))) void lds_void;
    typedef const __attribute__((address_space(1))) void gbl_void;
    const unsigned char *k0 = kv_plane<T>(P.K, P.ksb, P.ksg, p0, g), *k1 = kv_plane<T>(P.K, P.ksb, P.ksg, p1, g);
    const unsigned char *v0 = kv_plane<T>(P.V, P.vsb, P.vsg, p0, g), *v1 = kv_plane<T>(P.V, P.vsb, P.vsg, p1, g);
#pragma unroll
    for (int i = 0; i < G_::NLD; ++i) {
        const int r = i * G_::RPI + t.ld_row;
        const int pr = row0 + min(r, last);  // row counted from the start of page p0
        const bool second = pr >= rows;
        const int in = second ? pr - rows : pr;
        __builtin_amdgcn_global_load_lds((gbl_void *)((second ? k1 : k0) + (uint32_t)(in * t.krowb + G_::row_piece(r, t.ld_piece))), (lds_void *)(kl + i * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void *)((second ? v1 : v0) + (uint32_t)(in * t.vrowb + G_::tr_piece(r, t.ld_piece))), (lds_void *)(vl + i * 1024), 16, 0, 0);
    }
#endif
}

// workgroup index -> (b,g) pair and workgroup within the pair, W workgroups per pair.  map_mode 2 (B*G % 8 == 0): workgroups are dealt
// round-robin over the 8 XCDs (index % 8 labels the XCD), so every XCD gets whole (b,g) pairs and walks them one after the other: the K/V
// of one pair then stays in that XCD's 4 MiB L2.  Placement only changes speed, never results.
__device__ __forceinline__ void wg_pair(unsigned bid, int map_mode, int W, int &bg, int &tc) {
    if (map_mode == 2) {
        const int xcd = bid & 7, idx = bid >> 3;
        bg = (idx / W) * 8 + xcd;
        tc = idx % W;
    } else {
        bg = bid / W;
        tc = bid % W;
    }
}

constexpr int PART_PAD = 4;  // split-KV partial record per head: m, l, 2 pad floats, then D accumulators (16-B aligned)
constexpr float RESCALE_THR = 8.0f;  // log2 units: raise the running max only when a tile exceeds it by more than this

// combine split-KV partials: one wave per (row, head); the nsplit (m,l) records are read by nsplit lanes at once
// and the accumulators by all lanes with every split's load in flight together (no dependent-load chain)
template <typename T, int D>
__global__ __launch_bounds__(256) void sel_attn_combine_kernel(SelAttnParams P) {
    const int lane = lane_id();
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int h = P.h, ns = P.nsplit;  // ns <= 16
    if (wid >= P.R * h) return;
    const int64_t row = wid / h;
    const int hh = (int)(wid % h);
    const float *base = P.part + ((row * ns) * (int64_t)h + hh) * (D + PART_PAD);
    const int64_t sstride = (int64_t)h * (D + PART_PAD);  // floats between consecutive splits of this (row, head)
    float m = -INFINITY, l = 0.f;
    if (lane < ns) {
        m = base[lane * sstride];
        l = base[lane * sstride + 1];
    }
    const float mmax = wave_max(m);
    const float w = (m == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m - mmax);
    const float ltot = wave_sum(l * w);
    float acc[D / 64];
#pragma unroll
    for (int c = 0; c < D / 64; ++c) acc[c] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        if (s < ns) {
            const float ws = __shfl(w, s, 64);
#pragma unroll
            for (int c = 0; c < D / 64; ++c) acc[c] = fmaf(base[s * sstride + PART_PAD + c * 64 + lane], ws, acc[c]);
        }
    }
    const float inv = (ltot > 0.f) ? 1.f / ltot : 0.f;
    T *Or = (T *)P.O + (row * (int64_t)h + hh) * D;
#pragma unroll
    for (int c = 0; c < D / 64; ++c) Or[c * 64 + lane] = Elt<T>::from_f(acc[c] * inv);
    if (P.lse && lane == 0) P.lse[row * h + hh] = (ltot > 0.f) ? (mmax + __builtin_amdgcn_logf(ltot)) * LN2 : -INFINITY;
}

}  // namespace nsa
