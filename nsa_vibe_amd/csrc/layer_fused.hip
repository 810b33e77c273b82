// Layer-level pieces of NSAAttention around the three attention branches (the "next" rows of the scope table):
//   * small-M linear (decode projections): out[M,N] = A[M,K] . W[N,K]^T
//   * RoPE + KV-cache append of a fused QKV projection (reference: nsa_attention.py:552-572 decode, :1002-1024 prefill;
//     rope.py:16-51)
//   * compressed-token emission phi = mean over l raw tokens of RoPE'd K and raw V (compress_pool.py:9-38,
//     nsa_attention.py:588-604)
//   * gate MLP + 3-branch combine (nsa_attention.py:32-82, 85-124)
// Arithmetic follows the PyTorch operator chain the reference runs, including where it rounds to the activation dtype
// (rnd() below), so a bf16 module gives the same numbers whether these kernels or the eager ops are used.
#include <type_traits>

#include "attn_mfma_tiles.hpp"
#include "layer_fused.hpp"
#include "layer_gate.hpp"

namespace nsa {

// rotation of pair index i (of D/2) at position pos: (sin, cos) rounded to the activation dtype as the eager chain has them
template <typename T>
__device__ __forceinline__ void rope_sincos(int i, int D, float pos, float base, float inv_scale, float &sn, float &cs) {
    const float e = (-2.0f * (float)i) / (float)D;
    const float inv_freq = powf(base, e);
    const float ang = (pos * inv_scale) * inv_freq;
    sincosf(ang, &sn, &cs);
    sn = rnd<T>(sn);
    cs = rnd<T>(cs);
}
template <typename T>
__device__ __forceinline__ void rope_rotate(float x0, float x1, float sn, float cs, float &r0, float &r1) {
    r0 = rnd<T>(rnd<T>(x0 * cs) - rnd<T>(x1 * sn));
    r1 = rnd<T>(rnd<T>(x0 * sn) + rnd<T>(x1 * cs));
}
// rotate the pair (x0, x1) of pair index i (of D/2) at position pos
template <typename T>
__device__ __forceinline__ void rope_pair(float x0, float x1, int i, int D, float pos, float base, float inv_scale, float &r0, float &r1) {
    float sn, cs;
    rope_sincos<T>(i, D, pos, base, inv_scale, sn, cs);
    rope_rotate<T>(x0, x1, sn, cs, r0, r1);
}

// 8 elements of the activation dtype held raw (one 16-byte load) -> floats
template <typename T>
__device__ __forceinline__ void raw8(const u32x4 &raw, float (&out)[8]) {
    static_assert(sizeof(T) == 2, "raw8: 16-bit element types");
    const T *e = (const T *)&raw;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = Elt<T>::to_f(e[j]);
}

// RMSNorm's rsqrt(mean(x^2) + eps) from a lane's partial sum of rnd(x^2), with the rounding points of the eager chain
// (llama_block_nsa.py:16-19)
template <typename T>
__device__ __forceinline__ float rms_finish(float acc, int K, float eps) {
    float r = rnd<T>(wave_sum(acc) / (float)K);
    r = rnd<T>(r + eps);
    return rnd<T>(1.0f / sqrtf(r));
}
// of one row, computed by the whole wave
template <typename T>
__device__ __forceinline__ float row_rms(const T *xr, int K, bool vec, float eps) {
    float acc = 0.f;
    for (int k = lane_id() * 8; k < K; k += 512) {
        float v[8];
        load8<T>(xr + k, K - k, vec, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += rnd<T>(v[j] * v[j]);
    }
    return rms_finish<T>(acc, K, eps);
}

// epi: 0 none, 1 silu, 2 + res (the residual value of this output)
template <typename T>
__device__ __forceinline__ float linear_epilogue(float acc, int epi, float res) {
    float v = rnd<T>(acc);  // the GEMM result in the activation dtype, then the fused elementwise op rounds again like the eager chain
    if (epi == 1) v = rnd<T>(v / (1.f + expf(-v)));  // silu
    else if (epi == 2) v = v + res;
    return v;
}

// ------------------------------------------------------------------------------------------ RoPE + cache append
// Where the column pair starting at `col` of a fused QKV projection row [Q | K_sel V_sel | K_win V_win | K_raw V_raw] goes -- the one place
// that knows the layout.  The destinations are Q_out [B,S,NQ] and the six cache tensors [B,G,rows,D]; element (b, s) of the pair is at
// p + b sb + s ss.  Q is rotated as ONE row of width NQ, K_sel and K_win per group over Dk, the raw keys and the values not at all.
template <typename T>
struct QkvCol {
    T *p;            // null when the tensor is (the backward: a gradient that is zero)
    int64_t sb, ss;  // elements between batches / tokens
    int ri, rD;      // rotation: pair index and width; ri < 0 = not rotated
    // col < NT; rows = rows per (b, g) of a cache tensor, row0 = the row of s = 0 there
    __device__ __forceinline__ QkvCol(const RopeAppendParams &P, int col, int rows, int row0) {
        const int NQ = P.G * P.h * P.Dk, GK = P.G * P.Dk, GV = P.G * P.Dv;
        if (col < NQ) {
            p = (T *)P.Q_out + col;
            sb = (int64_t)P.S * NQ;
            ss = NQ;
            ri = col >> 1;
            rD = NQ;
            return;
        }
        int c = col - NQ;
        const int pairw = GK + GV;
        const int sp = c / pairw;
        c -= sp * pairw;
        const bool isv = c >= GK;
        if (isv) c -= GK;
        const int D = isv ? P.Dv : P.Dk;
        const int g = c / D, dc = c - g * D;
        T *base = (T *)P.cache[2 * sp + (isv ? 1 : 0)];
        p = base ? base + ((int64_t)g * rows + row0) * D + dc : nullptr;
        sb = (int64_t)P.G * rows * D;
        ss = D;
        ri = !isv && sp < 2 ? dc >> 1 : -1;
        rD = P.Dk;
    }
};

// prefill form.  A thread owns ONE column pair (its rotation frequency, destination tensor and column are computed once) and
// walks the tokens: consecutive threads = consecutive columns, so loads and stores stay coalesced.
template <typename T>
__global__ __launch_bounds__(256) void rope_cache_append_kernel(RopeAppendParams P) {
    const int NT = P.G * P.h * P.Dk + 3 * P.G * P.Dk + 3 * P.G * P.Dv;
    const int cp = blockIdx.x * 256 + threadIdx.x;
    if (cp >= NT / 2) return;
    const int col = 2 * cp;
    const QkvCol<T> c(P, col, P.S_max, P.t0);
    const float inv_freq = c.ri >= 0 ? powf(P.rope_base, (-2.0f * (float)c.ri) / (float)c.rD) : 0.f;
    // positions outside, sequences inside: the rotation (sincosf: most of this kernel's arithmetic) depends on the position only
    for (int s = blockIdx.y; s < P.S; s += gridDim.y) {
        float sn = 0.f, cs = 1.f;
        if (c.ri >= 0) {
            const float ang = ((float)(P.t0 + s) * P.inv_scale) * inv_freq;
            sincosf(ang, &sn, &cs);
            sn = rnd<T>(sn);
            cs = rnd<T>(cs);
        }
        for (int b = blockIdx.z; b < P.B; b += gridDim.z) {
            const T *src = (const T *)P.proj + ((int64_t)b * P.S + s) * NT + col;
            float x0 = Elt<T>::to_f(src[0]), x1 = Elt<T>::to_f(src[1]);
            if (c.ri >= 0) rope_rotate<T>(x0, x1, sn, cs, x0, x1);
            T *d = c.p + b * c.sb + s * c.ss;
            d[0] = Elt<T>::from_f(x0);
            d[1] = Elt<T>::from_f(x1);
        }
    }
}

int launch_rope_cache_append(const RopeAppendParams &P, int dtype, hipStream_t st) {
    const int NT = P.G * P.h * P.Dk + 3 * P.G * P.Dk + 3 * P.G * P.Dv;
    const int64_t ntok = (int64_t)P.B * P.S;
    if (ntok == 0) return NSA_OK;
    // (rows of positions x slices of the batch: about 2048 of them; a thread shares one rotation between the sequences of its slice)
    const unsigned gy = (unsigned)std::min<int64_t>(P.S, 2048);
    const unsigned gz = (unsigned)std::max<int64_t>(1, std::min<int64_t>(P.B, 2048 / gy));
    const dim3 grid((unsigned)((NT / 2 + 255) / 256), gy, gz);
    with_elt(dtype, [&](auto t) { hipLaunchKernelGGL(rope_cache_append_kernel<decltype(t)>, grid, dim3(256), 0, st, P); });
    NSA_LAUNCH_CHECK("rope_cache_append");
    return NSA_OK;
}

// backward of rope_cache_append: d(proj) from dQ [B,S,NQ] and the six cache-slice gradients [B,G,S,D] (S rows, not S_max; null = zero),
// read where the forward writes.  The rotation is orthogonal, so the gradient of a rotated pair is the pair rotated back by the same angle.
template <typename T>
__global__ __launch_bounds__(256) void rope_cache_append_bwd_kernel(RopeAppendParams P) {
    const int NT = P.G * P.h * P.Dk + 3 * P.G * P.Dk + 3 * P.G * P.Dv;
    const int cp = blockIdx.x * 256 + threadIdx.x;
    if (cp >= NT / 2) return;
    const int col = 2 * cp;
    const QkvCol<T> c(P, col, P.S, 0);
    const float inv_freq = c.ri >= 0 ? powf(P.rope_base, (-2.0f * (float)c.ri) / (float)c.rD) : 0.f;
    const int64_t ntok = (int64_t)P.B * P.S;
    for (int64_t row = blockIdx.y; row < ntok; row += gridDim.y) {
        const int b = (int)(row / P.S), s = (int)(row - (int64_t)b * P.S);
        float g0 = 0.f, g1 = 0.f;
        if (c.p) {
            const T *p = c.p + b * c.sb + s * c.ss;
            g0 = Elt<T>::to_f(p[0]);
            g1 = Elt<T>::to_f(p[1]);
        }
        if (c.ri >= 0) {
            const float ang = ((float)(P.t0 + s) * P.inv_scale) * inv_freq;
            float sn, cs;
            sincosf(ang, &sn, &cs);
            sn = rnd<T>(sn);
            cs = rnd<T>(cs);
            const float r0 = g0 * cs + g1 * sn;  // y0 = x0 c - x1 s, y1 = x0 s + x1 c  =>  dx0 = g0 c + g1 s, dx1 = -g0 s + g1 c
            g1 = g1 * cs - g0 * sn;
            g0 = r0;
        }
        T *d = (T *)P.proj + row * NT + col;
        d[0] = Elt<T>::from_f(g0);
        d[1] = Elt<T>::from_f(g1);
    }
}

int launch_rope_cache_append_bwd(const RopeAppendParams &P, int dtype, hipStream_t st) {
    const int NT = P.G * P.h * P.Dk + 3 * P.G * P.Dk + 3 * P.G * P.Dv;
    const int64_t ntok = (int64_t)P.B * P.S;
    if (ntok == 0) return NSA_OK;
    const dim3 grid((unsigned)((NT / 2 + 255) / 256), (unsigned)std::min<int64_t>(ntok, 2048));
    with_elt(dtype, [&](auto t) { hipLaunchKernelGGL(rope_cache_append_bwd_kernel<decltype(t)>, grid, dim3(256), 0, st, P); });
    NSA_LAUNCH_CHECK("rope_cache_append_bwd");
    return NSA_OK;
}

// decode step (S = 1): destination and rotation of a column pair with the position-only part (powf + sincosf) separated, so that a kernel can
// evaluate it while its loads are in flight
template <typename T>
struct RopeDest {
    float sn, cs;
    bool rot;
    T *dst;           // row b = 0
    int64_t dst_row;  // elements between consecutive rows b
    // with_rotation = false: destination only (sn / cs come from elsewhere, e.g. from a thread of the workgroup that evaluated them once)
    __device__ __forceinline__ void init(const RopeAppendParams &P, int col, bool with_rotation = true) {
        const QkvCol<T> c(P, col, P.S_max, P.t0);  // (the MFMA form clamps the columns of a partial tile to NT - 2 before it asks)
        sn = 0.f;
        cs = 1.f;
        rot = c.ri >= 0;
        if (rot && with_rotation) rope_sincos<T>(c.ri, c.rD, (float)P.t0, P.rope_base, P.inv_scale, sn, cs);
        dst = c.p;
        dst_row = c.sb;
    }
    __device__ __forceinline__ void store(int b, float x0, float x1) const {
        if (rot) rope_rotate<T>(x0, x1, sn, cs, x0, x1);
        dst[b * dst_row] = Elt<T>::from_f(x0);
        dst[b * dst_row + 1] = Elt<T>::from_f(x1);
    }
};

// ragged rows form (P.t_pos): the position of sequence b's first row and whether the sequence is live.  Not live: a padding slot (negative
// position) or rows past the caller's bound / the cache capacity; such a sequence appends nothing.  No silent clamp.
struct RopeSeq {
    int t0;
    bool live;
};
__device__ __forceinline__ RopeSeq rope_seq(const RopeAppendParams &P, int b) {
    const int t0 = P.t_pos[b];
    return RopeSeq{t0, t0 >= 0 && t0 <= min(P.t_max, P.S_max - 1) - (P.S - 1)};
}

// rows form (S consecutive tokens per sequence: row m = b S + s of the projection sits at position t0 + s): the destination of a column pair.
// The rotation of (pair, s) is the single step's rope_sincos call at (float)(t0 + s), evaluated by whoever owns that pair of values.
template <typename T>
struct RopeRowsDest {
    bool rot;
    int ri, rD;
    T *dst;          // row (b, s) = (0, 0)
    int64_t sb, ss;  // elements between sequences / positions
    __device__ __forceinline__ void init(const RopeAppendParams &P, int col) {
        const QkvCol<T> c(P, col, P.S_max, P.t0);
        rot = c.ri >= 0;
        ri = c.ri;
        rD = c.rD;
        dst = c.p;
        sb = c.sb;
        ss = c.ss;
    }
    __device__ __forceinline__ void sincos(const RopeAppendParams &P, int s, float &sn, float &cs) const {
        sn = 0.f;
        cs = 1.f;
        if (rot) rope_sincos<T>(ri, rD, (float)(P.t0 + s), P.rope_base, P.inv_scale, sn, cs);
    }
    __device__ __forceinline__ void store(int b, int s, float sn, float cs, float x0, float x1) const {
        if (rot) rope_rotate<T>(x0, x1, sn, cs, x0, x1);
        T *d = dst + b * sb + s * ss;
        d[0] = Elt<T>::from_f(x0);
        d[1] = Elt<T>::from_f(x1);
    }
    // ---- ragged form (P.t_pos; P.t0 = 0, so dst is row 0 of the tensor): the sequence's own position
    __device__ __forceinline__ void sincos_at(const RopeAppendParams &P, int pos, float &sn, float &cs) const {
        sn = 0.f;
        cs = 1.f;
        if (rot) rope_sincos<T>(ri, rD, (float)pos, P.rope_base, P.inv_scale, sn, cs);
    }
    // q: the pair belongs to Q_out [B,S,NQ] (row s, written for every row); else to a cache tensor: row sq.t0 + s, and only of a live
    // sequence -- the one guard between a wrong position and the neighbouring slab
    __device__ __forceinline__ void store_at(bool q, int b, int s, const RopeSeq &sq, float sn, float cs, float x0, float x1) const {
        if (!q && !sq.live) return;
        if (rot) rope_rotate<T>(x0, x1, sn, cs, x0, x1);
        T *d = dst + b * sb + (int64_t)(q ? s : sq.t0 + s) * ss;
        d[0] = Elt<T>::from_f(x0);
        d[1] = Elt<T>::from_f(x1);
    }
    // ---- paged form (RopePagedParams): dst is row 0 of the group's plane in pool page 0, sb the page stride
    __device__ __forceinline__ void init_paged(const RopeAppendParams &P, int col) {
        const QkvCol<T> c(P, col, LAYER_PAGE_TOKENS, 0);
        rot = c.ri >= 0;
        ri = c.ri;
        rD = c.rD;
        dst = c.p;
        sb = c.sb;
        ss = c.ss;
    }
    // page: the pool page of the row's position pos = sq.t0 + s, already tested against [0, n_pages) by the caller (rope_page); -1 = no store
    __device__ __forceinline__ void store_paged(bool q, int b, int s, const RopeSeq &sq, int page, float sn, float cs, float x0, float x1) const {
        if (!q && (!sq.live || page < 0)) return;
        if (rot) rope_rotate<T>(x0, x1, sn, cs, x0, x1);
        T *d = q ? dst + b * sb + (int64_t)s * ss : dst + (int64_t)page * sb + (int64_t)((sq.t0 + s) & (LAYER_PAGE_TOKENS - 1)) * ss;
        d[0] = Elt<T>::from_f(x0);
        d[1] = Elt<T>::from_f(x1);
    }
};
// the pool page that holds position pos of live sequence b, or -1: the entry is read only for a live sequence (then pos < capacity, so the
// index is inside the table's row) and returned only after its test against [0, n_pages)
__device__ __forceinline__ int rope_page(const LayerPageTable &pg, int b, const RopeSeq &sq, int pos) {
    if (!sq.live) return -1;
    const int e = pg.table[(int64_t)b * pg.stride + (pos >> 10)];
    return e >= 0 && e < pg.n_pages ? e : -1;
}

// ------------------------------------------------------------------------------------------ few-row projections on the VALU
// out[m, n] = A[m, :] . W[n, :] for a few rows m: a wave owns CW weight rows (1; 2 = a rotation pair; 4 = the LM head, where four rows in
// flight per wave let the weight matrix stream at memory speed) and keeps one accumulator per (weight row, row of A): fmaf over k
// ascending, j ascending, then wave_sum.  Two kernel templates differ in how the k axis is walked and nothing else; two policies say what
// the A operand is and where a finished row goes.
//
// A-operand policies: the 8 activations of a row at k .. k + 7 as floats, for the chunk loop (loaded at each use) and for the
// all-loads-first form (Regs<NC>: the raw 16-byte pieces of up to 2 rows, fetched before the first use).
// RowsA: rows of A; when norm_w is given RMSNorm(A) is folded in -- the dot products see rnd(rnd(x r) g), r = row_rms
template <typename T>
struct RowsA {
    const T *A, *norm_w;
    float eps;
    static __device__ __forceinline__ void normed(float (&av)[8], float r, const float (&gv)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) av[j] = rnd<T>(rnd<T>(av[j] * r) * gv[j]);
    }
    // (chunk loop: rms = one value per row of the pass, gv = the norm weights of the k chunk; plain arrays of the kernel, so that the
    // row-indexed one stays in registers)
    template <int RB>
    __device__ __forceinline__ void rows(float (&rms)[RB], int m0, int mm, int K, bool vec) const {
        if (norm_w)
            for (int r = 0; r < mm; ++r) rms[r] = row_rms<T>(A + (int64_t)(m0 + r) * K, K, vec, eps);
    }
    __device__ __forceinline__ void chunk(float (&gv)[8], int k, int K, bool vec) const {
        if (norm_w) load8<T>(norm_w + k, K - k, vec && ((uintptr_t)norm_w % 16 == 0), gv);
    }
    __device__ __forceinline__ void row(float rms, const float (&gv)[8], int m, int k, int K, bool vec, float (&av)[8]) const {
        load8<T>(A + (int64_t)m * K + k, K - k, vec, av);
        if (norm_w) normed(av, rms, gv);
    }
    template <int NC>
    struct Regs {
        u32x4 ar[2][NC], gr[NC];
        float rms[2], gv[8];
    };
    template <int NC>
    __device__ __forceinline__ void fetch(Regs<NC> &x, int c, int kc, int M, int K) const {
        if (norm_w) x.gr[c] = *(const u32x4 *)(norm_w + kc);
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (r < M) x.ar[r][c] = *(const u32x4 *)(A + (int64_t)r * K + kc);
    }
    template <int NC>
    __device__ __forceinline__ void rows(Regs<NC> &x, const bool (&has)[NC], int M, int K) const {
        x.rms[0] = x.rms[1] = 1.f;
        if (!norm_w) return;
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (r < M) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c)
                    if (has[c]) {
                        float v[8];
                        raw8<T>(x.ar[r][c], v);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc += rnd<T>(v[j] * v[j]);
                    }
                x.rms[r] = rms_finish<T>(acc, K, eps);
            }
    }
    template <int NC>
    __device__ __forceinline__ void chunk(Regs<NC> &x, int c) const {
        if (norm_w) raw8<T>(x.gr[c], x.gv);
    }
    template <int NC>
    __device__ __forceinline__ void row(const Regs<NC> &x, int r, int c, float (&av)[8]) const {
        raw8<T>(x.ar[r][c], av);
        if (norm_w) normed(av, x.rms[r], x.gv);
    }
};
// MixA (decode output projection, all-loads-first form only): A[r, k] = g_cmp O_cmp + g_sel O_sel + g_win O_win of group k / (K / G) with the
// gate probabilities gates[r G + g][3] (evaluated by the launch that produced the branches), rounded to the activation dtype exactly where
// the mix kernel rounds (mix3), so this is decode_finish + the plain projection in one launch, same bits
template <typename T>
struct MixA {
    const T *Oc, *Os, *Ow;
    const float *gates;
    int G;
    template <int NC>
    struct Regs {
        u32x4 oc[2][NC], os[2][NC], ow[2][NC];
        float pr[2][NC][3];
    };
    template <int NC>
    __device__ __forceinline__ void fetch(Regs<NC> &x, int c, int kc, int M, int K) const {
        const int g = kc / (K / G);
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (r < M) {
                const int64_t o = (int64_t)r * K + kc;
                x.oc[r][c] = *(const u32x4 *)(Oc + o);
                x.os[r][c] = *(const u32x4 *)(Os + o);
                x.ow[r][c] = *(const u32x4 *)(Ow + o);
                const float *gp = gates + ((int64_t)r * G + g) * 3;
#pragma unroll
                for (int i = 0; i < 3; ++i) x.pr[r][c][i] = gp[i];
            }
    }
    template <int NC>
    __device__ __forceinline__ void rows(Regs<NC> &, const bool (&)[NC], int, int) const {}
    template <int NC>
    __device__ __forceinline__ void chunk(Regs<NC> &, int) const {}
    template <int NC>
    __device__ __forceinline__ void row(const Regs<NC> &x, int r, int c, float (&av)[8]) const {
        float oc[8], os[8], ow[8];
        raw8<T>(x.oc[r][c], oc);
        raw8<T>(x.os[r][c], os);
        raw8<T>(x.ow[r][c], ow);
#pragma unroll
        for (int j = 0; j < 8; ++j) av[j] = rnd<T>(mix3<T>(x.pr[r][c], oc[j], os[j], ow[j]));
    }
};

// Epilogue policies: init(n0) once per wave (the all-loads-first form calls it while its loads are in flight) gives the wave's state, then
// store(state, m, n, s) by lane 0 with s = the dot products of row m with the weight rows n, n + 1, ...: a multiple of GROUP of them (the
// chunk loop hands them over GROUP at a time, as soon as they are summed).
// LinearEpi: out[m, n] = linear_epilogue(s)
template <typename T>
struct LinearEpi {
    static constexpr int MIN_BLOCKS = 1, GROUP = 1;
    T *out;
    const T *res;
    int epi, N;
    struct Wave {};
    __device__ __forceinline__ Wave init(int) const { return {}; }
    template <int CW>
    __device__ __forceinline__ void store(const Wave &, int m, int n0, const float (&s)[CW]) const {
#pragma unroll
        for (int cc = 0; cc < CW; ++cc)
            if (n0 + cc < N) {
                const int64_t idx = (int64_t)m * N + n0 + cc;
                out[idx] = Elt<T>::from_f(linear_epilogue<T>(s[cc], epi, epi == 2 ? Elt<T>::to_f(res[idx]) : 0.f));
            }
    }
};
// RopeEpi (CW = 2, the decode step's fused QKV projection): the pair, rounded to the activation dtype as the separate GEMM leaves it, is
// rotated and appended to Q_out / its cache tensor at position t0
template <typename T>
struct RopeEpi {
    static constexpr int MIN_BLOCKS = 2, GROUP = 2;
    RopeAppendParams P;
    using Wave = RopeDest<T>;
    __device__ __forceinline__ Wave init(int n0) const {
        Wave rd;
        rd.init(P, n0);
        return rd;
    }
    __device__ __forceinline__ void store(const Wave &rd, int m, int, const float (&s)[2]) const { rd.store(m, rnd<T>(s[0]), rnd<T>(s[1])); }
};
// RopeRowsEpi (CW = 2, chunk loop): the same for S <= 16 consecutive tokens per sequence, row m = b S + s appended at position t0 + s.  The
// wave's pair has one rotation per s: lane s evaluates it once (powf + sincosf), lane 0 picks it up from the wave's own LDS slice per row
template <typename T>
struct RopeRowsEpi {
    static constexpr int MIN_BLOCKS = 2, GROUP = 2;
    static constexpr int MAX_S = 16;
    RopeAppendParams P;
    struct Wave {
        RopeRowsDest<T> rd;
        const float *sc;  // [S][2]: (sin, cos) of position t0 + s
    };
    __device__ __forceinline__ Wave init(int n0) const {
        __shared__ float sc[4][MAX_S][2];
        Wave w;
        w.rd.init(P, n0);
        const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
        if (lane < P.S) w.rd.sincos(P, lane, sc[wave][lane][0], sc[wave][lane][1]);
        wave_lds_fence();
        w.sc = &sc[wave][0][0];
        return w;
    }
    __device__ __forceinline__ void store(const Wave &w, int m, int, const float (&s)[2]) const {
        const int b = m / P.S, si = m - b * P.S;
        w.rd.store(b, si, w.sc[2 * si], w.sc[2 * si + 1], rnd<T>(s[0]), rnd<T>(s[1]));
    }
};

// RopeRaggedEpi (CW = 2, chunk loop): RopeRowsEpi with per-sequence positions (P.t_pos), row m = b S + s appended at t_pos[b] + s where the
// sequence is live.  The wave's pair has one rotation per (b, s) now: lane m evaluates that of row m for the first 64 rows (the route
// hands the chunk loop the calls of one or two rows), lane 0 evaluates a later row's when it stores it.  The scalar form keeps its table.
// PAGED (nsa_layer_decode_paged): the argument block with the table at its end; a cache row goes to the page of its own position
template <typename T, bool PAGED = false>
struct RopeRaggedEpi {
    static constexpr int MIN_BLOCKS = 2, GROUP = 2;
    static constexpr int TABLE = 64;
    std::conditional_t<PAGED, RopePagedParams, RopeAppendParams> P;
    struct Wave {
        RopeRowsDest<T> rd;
        bool q;
        const float *sc;  // [min(B S, 64)][2]: (sin, cos) of row m's position
    };
    __device__ __forceinline__ Wave init(int n0) const {
        __shared__ float sc[4][TABLE][2];
        Wave w;
        if constexpr (PAGED) w.rd.init_paged(P, n0);
        else w.rd.init(P, n0);
        w.q = n0 < P.G * P.h * P.Dk;
        const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
        if (lane < P.B * P.S) {
            const int b = lane / P.S;
            w.rd.sincos_at(P, P.t_pos[b] + (lane - b * P.S), sc[wave][lane][0], sc[wave][lane][1]);
        }
        wave_lds_fence();
        w.sc = &sc[wave][0][0];
        return w;
    }
    __device__ __forceinline__ void store(const Wave &w, int m, int, const float (&s)[2]) const {
        const int b = m / P.S, si = m - b * P.S;
        const RopeSeq sq = rope_seq(P, b);
        float sn, cs;
        if (m < TABLE) {
            sn = w.sc[2 * m];
            cs = w.sc[2 * m + 1];
        } else {
            w.rd.sincos_at(P, sq.t0 + si, sn, cs);
        }
        if constexpr (PAGED) w.rd.store_paged(w.q, b, si, sq, w.q ? -1 : rope_page(P.pg, b, sq, sq.t0 + si), sn, cs, rnd<T>(s[0]), rnd<T>(s[1]));
        else w.rd.store_at(w.q, b, si, sq, sn, cs, rnd<T>(s[0]), rnd<T>(s[1]));
    }
};

// chunk-loop form (any dtype, K and alignment): k in 512-element chunks, rows of A in passes of 8 (CW = 4: at most 2 rows, one pass).  The
// loads of one k chunk are waited for before the next goes out.
template <typename T, int CW, typename AOp, typename Epi>
__global__ __launch_bounds__(256, Epi::MIN_BLOCKS) void proj_loop_kernel(const AOp a, const T *__restrict__ W, int M, int N, int K, const Epi e) {
    constexpr int RB = CW == 4 ? 2 : 8;  // rows of A per pass; the 4-row form is only routed 1-2 rows: one pass, no row loop
    const int lane = lane_id();
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * CW;
    if (n0 >= N) return;
    const bool vec = (K % 8 == 0) && (((uintptr_t)a.A | (uintptr_t)W) % 16 == 0);
    const typename Epi::Wave ew = e.init(n0);
    for (int m0 = 0; m0 < (CW == 4 ? 1 : M); m0 += RB) {
        const int mm = min(RB, M - m0);
        float rms[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) rms[r] = 1.f;
        a.rows(rms, m0, mm, K, vec);
        float acc[CW][RB];
#pragma unroll
        for (int cc = 0; cc < CW; ++cc)
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[cc][r] = 0.f;
        for (int k = lane * 8; k < K; k += 512) {
            // (the 4-row form keeps each row's activations in registers of their own, as the kernel it was folded from did: one shared
            // buffer costs it 3 VGPRs and with them a wave per SIMD)
            float wv[CW][8], av[CW == 4 ? RB : 1][8], gv[8];
#pragma unroll
            for (int cc = 0; cc < CW; ++cc) load8<T>(W + (int64_t)min(n0 + cc, N - 1) * K + k, K - k, vec, wv[cc]);
            a.chunk(gv, k, K, vec);
            for (int r = 0; r < mm; ++r) {
                float (&avr)[8] = av[CW == 4 ? r : 0];
                a.row(rms[r], gv, m0 + r, k, K, vec, avr);
#pragma unroll
                for (int cc = 0; cc < CW; ++cc)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[cc][r] = fmaf(wv[cc][j], avr[j], acc[cc][r]);
            }
        }
        for (int r = 0; r < mm; ++r)
#pragma unroll
            for (int cc = 0; cc < CW; cc += Epi::GROUP) {
                float s[Epi::GROUP];
#pragma unroll
                for (int i = 0; i < Epi::GROUP; ++i) s[i] = wave_sum(acc[cc + i][r]);
                if (lane == 0) e.store(ew, m0 + r, n0 + cc, s);
            }
    }
}

// all-loads-first form for 1-2 rows of 16-bit activations with K <= 512 NC (16-byte aligned rows): a decode step is a chain of such launches
// and each is as long as its chain of dependent memory round trips -- the chunk loop waits for the loads of one 512-element chunk before it
// issues the next (fc2 at K = 3072: six round trips in a row).  Here every load of the wave (weights, norm weights, the rows of A) goes out
// before the first use, and the epilogue's position-only arithmetic (RoPE: powf + sincosf, ~1 us) runs while they are in flight; the
// arithmetic is the chunk loop's in the same order (same bits).
template <typename T, int NC, int CW, typename AOp, typename Epi>
__global__ __launch_bounds__(256, Epi::MIN_BLOCKS) void proj_fast_kernel(const AOp a, const T *__restrict__ W, int M, int N, int K, const Epi e) {
    const int lane = lane_id();
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * CW;
    if (n0 >= N) return;
    u32x4 wr[CW][NC];
    typename AOp::template Regs<NC> x;
    bool has[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int k = lane * 8 + 512 * c;
        has[c] = k < K;
        const int kc = min(k, K - 8);
#pragma unroll
        for (int cc = 0; cc < CW; ++cc) wr[cc][c] = *(const u32x4 *)(W + (int64_t)min(n0 + cc, N - 1) * K + kc);
        a.fetch(x, c, kc, M, K);
    }
    const typename Epi::Wave ew = e.init(n0);
    a.rows(x, has, M, K);
    float acc[CW][2];
#pragma unroll
    for (int cc = 0; cc < CW; ++cc) acc[cc][0] = acc[cc][1] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (has[c]) {
            float wv[CW][8], av[8];
#pragma unroll
            for (int cc = 0; cc < CW; ++cc) raw8<T>(wr[cc][c], wv[cc]);
            a.chunk(x, c);
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if (r < M) {
                    a.row(x, r, c, av);
#pragma unroll
                    for (int j = 0; j < 8; ++j)
#pragma unroll
                        for (int cc = 0; cc < CW; ++cc) acc[cc][r] = fmaf(wv[cc][j], av[j], acc[cc][r]);
                }
        }
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (r < M) {
            float s[CW];
#pragma unroll
            for (int cc = 0; cc < CW; ++cc) s[cc] = wave_sum(acc[cc][r]);
            if (lane == 0) e.store(ew, r, n0, s);
        }
}

// ---- MFMA form for 9 <= M rows (batched decode): workgroup = 16 output columns x 64 rows, the 4 waves split the K axis.
// C^T[n, m] = W[n,:] . X[m,:]: W rows are the MFMA A operand (each W element is fetched once, straight from global in
// fragment shape), the rows of X the B operand (L1/L2 resident), all loads of a wave issued before its first MFMA; the four
// K-partials meet in LDS.  Thread t of the epilogue owns row m = t % 64 and columns 4 (t / 64) .. +3 (two rotation pairs).
// MIX (decode output projection): the rows of X are the three-branch mix, formed on the fly from X = O_cmp, mx.Os, mx.Ow and the row
// gates mx.gates[m G + g][3] with the rounding of the mix kernel (the same operand values as decode_finish + this kernel: same bits)
struct LinearMixArgs {
    const void *Os, *Ow;
    const float *gates;
    int G;
};
// NWV = waves of a workgroup that split the K axis: 4, or 8 for long rows (K >= 2048: fc2 of the MLP) -- a wave's k-steps go out in
// rounds of 6, each round a memory round trip, so K = 3072 on 4 waves was four of them in a row (15.5 us at 32 rows, 8.5 for fc1)
// ROWS (with ROPE): P.S <= 16 consecutive tokens per sequence, row m = b P.S + s appended at position P.t0 + s (RopeRowsDest)
// RAGGED (with ROWS): at position P.t_pos[b] + s, the cache rows of a live sequence only (rope_seq).  A template flag: the scalar
// instantiations keep their code
// PAGED (with RAGGED; nsa_layer_decode_paged): the argument block is RopePagedParams, the six caches are pools of pages; the thread looks up
// the page of its row's position beside the position itself and tests it before any address is formed (rope_page)
template <typename T, bool ROPE, bool MIX = false, int NWV = 4, bool ROWS = false, bool RAGGED = false, bool PAGED = false>
__global__ __launch_bounds__(NWV * 64, 2) void linear_mfma_kernel(std::conditional_t<PAGED, RopePagedParams, RopeAppendParams> P, const T *__restrict__ X,
                                                               const T *__restrict__ W,
                                                               T *__restrict__ out, int M, int N, int K, int epi, const T *__restrict__ res,
                                                               LinearMixArgs mx) {
    static_assert(NWV == 4 || (NWV == 8 && !ROPE && !MIX), "eight waves: the plain projection only");
    static_assert(!ROWS || ROPE, "rows form: the RoPE + append epilogue only");
    static_assert(!RAGGED || ROWS, "ragged form: the rows epilogue only");
    static_assert(!PAGED || RAGGED, "paged form: the ragged rows epilogue only");
    using MT_ = MfmaT<T>;
    using x8 = typename MT_::x8;
    __shared__ float part[NWV][16][65];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6), rho = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 64;
    const int ksteps = K / 32, per = (ksteps + NWV - 1) / NWV;
    const int s0 = wave * per, s1 = min(ksteps, s0 + per);
    // the residual of this thread's outputs, fetched now: in the epilogue it would be one more dependent memory round trip
    constexpr int CPT = 16 / NWV;  // columns per thread of the epilogue
    [[maybe_unused]] float resv[CPT];
    if constexpr (!ROPE) {
        if (epi == 2) {
            const int m = min(m0 + (int)(threadIdx.x & 63), M - 1), nq = (int)(threadIdx.x >> 6);
#pragma unroll
            for (int r = 0; r < CPT; ++r) resv[r] = Elt<T>::to_f(res[(int64_t)m * N + min(n0 + CPT * nq + r, N - 1)]);
        }
    }
    f32x4 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const T *wrow = W + (int64_t)min(n0 + rho, N - 1) * K + 8 * q;  // the last column tile may be partial: clamp, store guarded
    // ROPE (P.S == 1): the rotations of the workgroup's 8 column pairs depend on the position only -- threads 0..7 evaluate one each (powf +
    // sincosf) while the loads are in flight and pass it through LDS; every thread then needs only the destinations of its two pairs
    // ROWS: one rotation per (pair, s), 8 P.S <= 128 values: thread 8 s + pair evaluates one, entry [8 s + pair]
    [[maybe_unused]] std::conditional_t<ROWS, RopeRowsDest<T>, RopeDest<T>> rd[2];
    __shared__ float rsc[ROWS && !RAGGED ? 128 : 8][2];
    // RAGGED: a rotation per (pair, b, s) -- up to 64 sequences under one workgroup, too many for a table: the thread that stores row
    // m = m0 + t % 64 evaluates the rotations of its own two pairs at t_pos[b] + s here, before the loads go out (one position load each)
    [[maybe_unused]] RopeSeq sq{0, false};
    [[maybe_unused]] float rsn[2], rcs[2];
    [[maybe_unused]] int page = -1;  // PAGED: the pool page of this thread's row (one lookup beside the position's), -1 = no cache store
    if constexpr (RAGGED) {
        const int mr = min(m0 + (int)(threadIdx.x & 63), M - 1), b = mr / P.S;
        sq = rope_seq(P, b);
        if constexpr (PAGED) page = rope_page(P.pg, b, sq, sq.t0 + (mr - b * P.S));
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if constexpr (PAGED) rd[p].init_paged(P, min(n0 + 4 * (int)(threadIdx.x >> 6) + 2 * p, N - 2));
            else rd[p].init(P, min(n0 + 4 * (int)(threadIdx.x >> 6) + 2 * p, N - 2));
            rd[p].sincos_at(P, sq.t0 + (mr - b * P.S), rsn[p], rcs[p]);
        }
    } else if constexpr (ROWS) {
        if ((int)threadIdx.x < 8 * P.S) {
            RopeRowsDest<T> one;
            one.init(P, min(n0 + 2 * (int)(threadIdx.x & 7), N - 2));
            one.sincos(P, (int)(threadIdx.x >> 3), rsc[threadIdx.x][0], rsc[threadIdx.x][1]);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) rd[p].init(P, min(n0 + 4 * (int)(threadIdx.x >> 6) + 2 * p, N - 2));
    } else if constexpr (ROPE) {
        if (threadIdx.x < 8) {
            RopeDest<T> one;
            one.init(P, min(n0 + 2 * (int)threadIdx.x, N - 2));
            rsc[threadIdx.x][0] = one.sn;
            rsc[threadIdx.x][1] = one.cs;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) rd[p].init(P, min(n0 + 4 * (int)(threadIdx.x >> 6) + 2 * p, N - 2), false);
    }
    if constexpr (MIX) {
        const int kpg = K / mx.G;
        const int nmt = min(4, (M - m0 + 15) >> 4);  // 16-row tiles that hold a row (the plain form computes clamped duplicates instead)
        auto run = [&](auto RC) {
            constexpr int R = decltype(RC)::value;  // k-steps in flight: 3 R (nmt + 1) + ... loads per round
            for (int sb = s0; sb < s1; sb += R) {
                x8 wf[R], oc[R][4], os[R][4], ow[R][4];
                float pr[R][4][3];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int s = min(sb + i, s1 - 1);
                    wf[i] = *(const x8 *)(wrow + 32 * s);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        if (mt < nmt) {
                            const int m = min(m0 + 16 * mt + rho, M - 1);
                            const int64_t o = (int64_t)m * K + 32 * s + 8 * q;
                            oc[i][mt] = *(const x8 *)(X + o);
                            os[i][mt] = *(const x8 *)((const T *)mx.Os + o);
                            ow[i][mt] = *(const x8 *)((const T *)mx.Ow + o);
                            const float *gp = mx.gates + ((int64_t)m * mx.G + (32 * s + 8 * q) / kpg) * 3;
#pragma unroll
                            for (int k = 0; k < 3; ++k) pr[i][mt][k] = gp[k];
                        }
                }
#pragma unroll
                for (int i = 0; i < R; ++i)
                    if (sb + i < s1) {
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt)
                            if (mt < nmt) {
                                x8 xm;
#pragma unroll
                                for (int j = 0; j < 8; ++j)
                                    xm[j] = Elt<T>::from_f(mix3<T>(pr[i][mt], Elt<T>::to_f(oc[i][mt][j]), Elt<T>::to_f(os[i][mt][j]), Elt<T>::to_f(ow[i][mt][j])));
                                acc[mt] = MT_::mma(wf[i], xm, acc[mt]);
                            }
                    }
            }
        };
        if (nmt == 1) run(std::integral_constant<int, 6>{});
        else run(std::integral_constant<int, 2>{});
    } else {
        const int nmt = min(4, (M - m0 + 15) >> 4);  // 16-row tiles that hold a row: the others are neither fetched nor multiplied
        for (int sb = s0; sb < s1; sb += 6) {  // 6 k-steps (up to 30 loads) in flight per round
            x8 wf[6], xf[6][4];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int s = min(sb + i, s1 - 1);
                wf[i] = *(const x8 *)(wrow + 32 * s);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    if (mt < nmt) xf[i][mt] = *(const x8 *)(X + (int64_t)min(m0 + 16 * mt + rho, M - 1) * K + 32 * s + 8 * q);
            }
#pragma unroll
            for (int i = 0; i < 6; ++i)
                if (sb + i < s1) {
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        if (mt < nmt) acc[mt] = MT_::mma(wf[i], xf[i][mt], acc[mt]);
                }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][4 * q + r][16 * mt + rho] = acc[mt][r];
    __syncthreads();
    const int m = m0 + (threadIdx.x & 63), nq = threadIdx.x >> 6;
    float v[CPT];
#pragma unroll
    for (int r = 0; r < CPT; ++r) {
        const int n = CPT * nq + r, mm = threadIdx.x & 63;
        v[r] = (part[0][n][mm] + part[1][n][mm]) + (part[2][n][mm] + part[3][n][mm]);
        if constexpr (NWV == 8) v[r] += (part[4][n][mm] + part[5][n][mm]) + (part[6][n][mm] + part[7][n][mm]);
    }
    if (m >= M) return;
    if (ROPE) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (n0 + 4 * nq + 2 * p < N) {
                if constexpr (PAGED) {
                    const int b = m / P.S;
                    rd[p].store_paged(n0 + 4 * nq + 2 * p < P.G * P.h * P.Dk, b, m - b * P.S, sq, page, rsn[p], rcs[p], rnd<T>(v[2 * p]), rnd<T>(v[2 * p + 1]));
                } else if constexpr (RAGGED) {
                    const int b = m / P.S;
                    rd[p].store_at(n0 + 4 * nq + 2 * p < P.G * P.h * P.Dk, b, m - b * P.S, sq, rsn[p], rcs[p], rnd<T>(v[2 * p]), rnd<T>(v[2 * p + 1]));
                } else if constexpr (ROWS) {
                    const int b = m / P.S, s = m - b * P.S, e = 8 * s + 2 * nq + p;  // (the entry of this row's position)
                    rd[p].store(b, s, rsc[e][0], rsc[e][1], rnd<T>(v[2 * p]), rnd<T>(v[2 * p + 1]));
                } else {
                    rd[p].sn = rsc[2 * nq + p][0];  // (written before the barrier above)
                    rd[p].cs = rsc[2 * nq + p][1];
                    rd[p].store(m, rnd<T>(v[2 * p]), rnd<T>(v[2 * p + 1]));
                }
            }
    } else {
#pragma unroll
        for (int r = 0; r < CPT; ++r) {
            if (n0 + CPT * nq + r >= N) break;
            const int64_t idx = (int64_t)m * N + n0 + CPT * nq + r;
            out[idx] = Elt<T>::from_f(linear_epilogue<T>(v[r], epi, epi == 2 ? resv[r] : 0.f));  // (the residual from the registers)
        }
    }
}

// ---- the family's route: the only place that knows the bounds of its forms.  The launchers below switch on the answer, the callers read
// fold_norm (the block and the model step) and form (the mix) from it.
ProjRoute proj_route(const LinearCall &c, ProjKind kind) {
    const bool plain = kind == PROJ_PLAIN, mix = kind == PROJ_MIX, b16 = c.dtype == NSA_DT_BF16 || c.dtype == NSA_DT_F16;
    const bool aligned = (((uintptr_t)c.A | (uintptr_t)c.W | (uintptr_t)c.Os | (uintptr_t)c.Ow) % 16 == 0);  // (Os, Ow: null without a mix)
    ProjRoute r{};
    // the mix: 16-bit whole k-steps per group; rows 1-2 as VALU dot products of at most 2048 elements, from 3 on the MFMA kernel
    if (mix && !(b16 && aligned && c.M >= 1 && c.N >= 1 && c.G >= 1 && c.K % (32 * c.G) == 0 && (c.M >= 3 || c.K <= 2048))) return r;
    if (b16 && aligned && c.M >= 3 && c.K % 32 == 0) {
        r.form = PROJ_MFMA;
        r.waves = plain && c.K >= 2048 ? 8 : 4;
        r.grid = dim3((unsigned)((c.N + 15) / 16), (unsigned)((c.M + 63) / 64));
        return r;
    }
    // all-loads-first: 1-2 rows of 16-byte aligned 16-bit operands with K <= 512 NC, NC <= 8 (with a RoPE epilogue or a mix: 4); the rows
    // call stays with the chunk loop
    const int nc = (c.K + 511) / 512;
    const bool fast = mix || (kind != PROJ_ROPE_ROWS && b16 && aligned && c.M <= 2 && c.K >= 8 && c.K % 8 == 0 && c.K <= (plain ? 4096 : 2048) &&
                              (uintptr_t)c.norm_w % 16 == 0);
    const bool g4 = plain && c.N >= 4096 && (fast ? nc <= 2 : c.M <= 2);  // four weight rows per wave
    r.form = fast ? PROJ_FAST : PROJ_LOOP;
    r.nc = 2 * ((nc + 1) / 2);  // tiers of 2, 4, 6, 8 chunks
    r.cw = plain ? (g4 ? 4 : 1) : mix ? 1 : 2;
    r.grid = dim3((unsigned)((c.N + 4 * r.cw - 1) / (4 * r.cw)));
    r.fold_norm = !mix;
    return r;
}

// one launch of a VALU form as the route says: proj_fast_kernel with r.nc of the tiers NCS the policy pair is built for, else the chunk loop
template <typename T, int CW, int... NCS, typename AOp, typename Epi>
static void launch_proj_valu(const ProjRoute &r, const LinearCall &c, const AOp &a, const Epi &e) {
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, r.grid, dim3(256), 0, c.st, a, (const T *)c.W, c.M, c.N, c.K, e); };
    if constexpr (sizeof(T) == 2) {
        if (r.form == PROJ_FAST) {
            ((r.nc == NCS ? go(proj_fast_kernel<T, NCS, CW, AOp, Epi>) : void()), ...);
            return;
        }
    }
    if constexpr (std::is_same_v<AOp, RowsA<T>>) go(proj_loop_kernel<T, CW, AOp, Epi>);
}
template <bool ROPE, bool MIX, int NWV, bool ROWS, bool RAGGED = false, bool PAGED = false>
static void launch_linear_mfma(const std::conditional_t<PAGED, RopePagedParams, RopeAppendParams> &P, const ProjRoute &r, const LinearCall &c) {
    with_elt<false>(c.dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((linear_mfma_kernel<T, ROPE, MIX, NWV, ROWS, RAGGED, PAGED>), r.grid, dim3(NWV * 64), 0, c.st, P, (const T *)c.A, (const T *)c.W, (T *)c.out, c.M,
                           c.N, c.K, c.epi, (const T *)c.res, LinearMixArgs{c.Os, c.Ow, c.gates, c.G});
    });
}

int launch_linear_small_epi(const LinearCall &c) {
    const ProjRoute r = proj_route(c, PROJ_PLAIN);
    if (r.form == PROJ_MFMA) {
        NSA_CHECK_ARG(c.norm_w == nullptr, "linear_small: the MFMA form takes normalised input");  // (launch_linear_normed sees to it)
        if (r.waves == 8) launch_linear_mfma<false, false, 8, false>({}, r, c);
        else launch_linear_mfma<false, false, 4, false>({}, r, c);
        NSA_LAUNCH_CHECK("linear_small(mfma)");
        return NSA_OK;
    }
    with_elt(c.dtype, [&](auto t) {
        using T = decltype(t);
        const RowsA<T> a{(const T *)c.A, (const T *)c.norm_w, c.eps};
        const LinearEpi<T> e{(T *)c.out, (const T *)c.res, c.epi, c.N};
        if (r.cw == 4) launch_proj_valu<T, 4, 2>(r, c, a, e);
        else launch_proj_valu<T, 1, 2, 4, 6, 8>(r, c, a, e);
    });
    if (r.form == PROJ_FAST) NSA_LAUNCH_CHECK("linear_small(fast)");
    else NSA_LAUNCH_CHECK("linear_small");
    return NSA_OK;
}
int launch_linear_normed(const LinearCall &c, void *scratch) {
    if (proj_route(c, PROJ_PLAIN).fold_norm) return launch_linear_small_epi(c);
    if (int rc = launch_rmsnorm_rows(c.A, c.norm_w, scratch, c.M, c.K, c.eps, c.dtype, c.st)) return rc;
    LinearCall p = c;
    p.A = scratch;
    p.norm_w = nullptr;
    return launch_linear_small_epi(p);
}

int launch_linear_small_mix(const LinearCall &c) {
    const ProjRoute r = proj_route(c, PROJ_MIX);
    NSA_CHECK_ARG(r.form != PROJ_NONE && c.gates && c.out, "linear_small_mix: unsupported shape");
    if (r.form == PROJ_MFMA) {
        launch_linear_mfma<false, true, 4, false>({}, r, c);
    } else {
        with_elt<false>(c.dtype, [&](auto t) {
            using T = decltype(t);
            launch_proj_valu<T, 1, 2, 4>(r, c, MixA<T>{(const T *)c.A, (const T *)c.Os, (const T *)c.Ow, c.gates, c.G},
                                         LinearEpi<T>{(T *)c.out, (const T *)c.res, c.epi, c.N});
        });
    }
    NSA_LAUNCH_CHECK("linear_small_mix");
    return NSA_OK;
}

// c.N = the columns P maps (qkv_cols); c.norm_w: RMSNorm(c.A) folded in where the caller read fold_norm from this call's route
int launch_qkv_rope_append(const RopeAppendParams &P, const LinearCall &c, bool rows) {
    NSA_CHECK_ARG(P.S >= 1 && P.S <= RopeRowsEpi<float>::MAX_S, "qkv_rope_append: 1 to 16 tokens per sequence");
    const bool ragged = P.t_pos != nullptr;  // per-sequence positions: the RAGGED instantiations of the rows forms
    NSA_CHECK_ARG(!ragged || (rows && P.t0 == 0), "qkv_rope_append: a position array goes with the rows form and t0 = 0");
    const ProjRoute r = proj_route(c, rows ? PROJ_ROPE_ROWS : PROJ_ROPE);
    if (r.form == PROJ_MFMA) {
        if (rows) {
            if (ragged) launch_linear_mfma<true, false, 4, true, true>(P, r, c);
            else launch_linear_mfma<true, false, 4, true>(P, r, c);
            NSA_LAUNCH_CHECK("qkv_rope_append(rows, mfma)");
        } else {
            launch_linear_mfma<true, false, 4, false>(P, r, c);
            NSA_LAUNCH_CHECK("qkv_rope_append(mfma)");
        }
        return NSA_OK;
    }
    with_elt(c.dtype, [&](auto t) {
        using T = decltype(t);
        const RowsA<T> a{(const T *)c.A, (const T *)c.norm_w, c.eps};
        if (ragged) launch_proj_valu<T, 2>(r, c, a, RopeRaggedEpi<T>{P});
        else if (rows) launch_proj_valu<T, 2>(r, c, a, RopeRowsEpi<T>{P});
        else launch_proj_valu<T, 2, 2, 4>(r, c, a, RopeEpi<T>{P});
    });
    if (rows) NSA_LAUNCH_CHECK("qkv_rope_append(rows)");
    else if (r.form == PROJ_FAST) NSA_LAUNCH_CHECK("qkv_rope_append(fast)");
    else NSA_LAUNCH_CHECK("qkv_rope_append");
    return NSA_OK;
}

// the paged call's projection: the rows route (MFMA from three rows on, else the chunk loop), its PAGED instantiations
int launch_qkv_rope_append_paged(const RopePagedParams &P, const LinearCall &c) {
    NSA_CHECK_ARG(P.S >= 1 && P.S <= RopeRowsEpi<float>::MAX_S, "qkv_rope_append(paged): 1 to 16 tokens per sequence");
    NSA_CHECK_ARG(P.t_pos && P.t0 == 0 && P.pg.table && P.pg.n_pages >= 1 && P.pg.stride >= P.pg.max_pages && P.S_max == P.pg.max_pages * LAYER_PAGE_TOKENS,
                  "qkv_rope_append(paged): positions, a block table and the capacity max_pages * 1024");
    NSA_CHECK_ARG(c.dtype == NSA_DT_BF16 || c.dtype == NSA_DT_F16, "qkv_rope_append(paged): bf16 / f16 only");
    const ProjRoute r = proj_route(c, PROJ_ROPE_ROWS);
    if (r.form == PROJ_MFMA) {
        launch_linear_mfma<true, false, 4, true, true, true>(P, r, c);
        NSA_LAUNCH_CHECK("qkv_rope_append(paged, mfma)");
        return NSA_OK;
    }
    with_elt<false>(c.dtype, [&](auto t) {
        using T = decltype(t);
        launch_proj_valu<T, 2>(r, c, RowsA<T>{(const T *)c.A, (const T *)c.norm_w, c.eps}, RopeRaggedEpi<T, true>{P});
    });
    NSA_LAUNCH_CHECK("qkv_rope_append(paged)");
    return NSA_OK;
}

// the paged call's verdicts: wave b tests sequence b once for every later launch (they take t_live as their position array)
__global__ __launch_bounds__(256) void paged_live_kernel(PagedLiveParams P) {
    const int b = (int)(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = lane_id();
    if (b >= P.B) return;
    const int t0 = P.t_pos[b];
    bool ok = t0 >= 0 && t0 <= P.te - (P.S - 1);  // (te <= max_pages * 1024 - 1: the entries read below lie inside the table's row)
    if (ok) {
        const int last = (t0 + P.S - 1) >> 10;
        int bad = 0;
        for (int j = lane; j <= last; j += 64) {
            const int e = P.pg.table[(int64_t)b * P.pg.stride + j];
            bad |= (e < 0 || e >= P.pg.n_pages) ? 1 : 0;
        }
        ok = wave_sum_i(bad) == 0;
    }
    if (lane == 0) P.t_live[b] = ok ? t0 : -1;
}
int launch_paged_live(const PagedLiveParams &P, hipStream_t st) {
    NSA_CHECK_ARG(P.t_pos && P.t_live && P.pg.table && P.B >= 1 && P.S >= 1 && P.pg.n_pages >= 1 && P.pg.max_pages >= 1 && P.pg.stride >= P.pg.max_pages &&
                      P.te >= 0 && (int64_t)P.te <= (int64_t)P.pg.max_pages * LAYER_PAGE_TOKENS - 1,
                  "paged_live: positions, a block table and te inside the capacity max_pages * 1024");
    hipLaunchKernelGGL(paged_live_kernel, dim3((unsigned)((P.B + 3) / 4)), dim3(256), 0, st, P);
    NSA_LAUNCH_CHECK("paged_live");
    return NSA_OK;
}

// ------------------------------------------------------------------------------------------ compressed-token emission
// one 64-thread block per (b, g, j): K_cmp[j] = mean_i rope(K_raw[j d + i], pos = j d + i), V_cmp[j] = mean_i V_raw[j d + i]
template <typename T>
__global__ __launch_bounds__(64) void cmp_pool_kernel(CmpPoolParams P) {
    const int nj = P.j1 - P.j0;
    const int j = P.j0 + (int)(blockIdx.x % nj);
    const int bg = (int)(blockIdx.x / nj);
    const T *Kr = (const T *)P.K_raw + (int64_t)bg * P.S_max * P.Dk;
    const T *Vr = (const T *)P.V_raw + (int64_t)bg * P.S_max * P.Dv;
    T *Kc = (T *)P.K_cmp + ((int64_t)bg * P.n_cmp_max + j) * P.Dk;
    T *Vc = (T *)P.V_cmp + ((int64_t)bg * P.n_cmp_max + j) * P.Dv;
    const int r0 = j * P.d;
    for (int p = threadIdx.x; p < P.Dk / 2; p += 64) {
        float a0 = 0.f, a1 = 0.f;
        const float inv_freq = powf(P.rope_base, (-2.0f * (float)p) / (float)P.Dk);  // (rope_sincos's value, once per pair instead of per token)
        if (P.l <= 32) {
            // the l loads of the pair first (the loop below waits for each token's load behind the previous token's sincosf: a block was
            // as long as l dependent memory round trips)
            float xa[32], xb[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const T *src = Kr + (int64_t)(r0 + min(i, P.l - 1)) * P.Dk + 2 * p;
                xa[i] = Elt<T>::to_f(src[0]);
                xb[i] = Elt<T>::to_f(src[1]);
            }
#pragma unroll
            for (int i = 0; i < 32; ++i)
                if (i < P.l) {
                    float x0, x1, sn, cs;
                    sincosf(((float)(r0 + i) * P.inv_scale) * inv_freq, &sn, &cs);
                    rope_rotate<T>(xa[i], xb[i], rnd<T>(sn), rnd<T>(cs), x0, x1);
                    a0 += x0;
                    a1 += x1;
                }
        } else
        for (int i = 0; i < P.l; ++i) {
            const T *src = Kr + (int64_t)(r0 + i) * P.Dk + 2 * p;
            float x0, x1, sn, cs;
            sincosf(((float)(r0 + i) * P.inv_scale) * inv_freq, &sn, &cs);
            rope_rotate<T>(Elt<T>::to_f(src[0]), Elt<T>::to_f(src[1]), rnd<T>(sn), rnd<T>(cs), x0, x1);
            a0 += x0;
            a1 += x1;
        }
        Kc[2 * p] = Elt<T>::from_f(a0 / (float)P.l);
        Kc[2 * p + 1] = Elt<T>::from_f(a1 / (float)P.l);
    }
    for (int c = threadIdx.x; c < P.Dv; c += 64) {
        float a = 0.f;
        for (int i = 0; i < P.l; ++i) a += Elt<T>::to_f(Vr[(int64_t)(r0 + i) * P.Dv + c]);
        Vc[c] = Elt<T>::from_f(a / (float)P.l);
    }
}

// the same with the l rotations of a pair spread over the threads of a 256-thread block (the 64-thread form walks them one after the other:
// l x (powf + sincosf) in a row, 24 us for the ONE token a decode step emits): rotated keys and raw values go to LDS, then one thread per
// column sums them in the original order i = 0 .. l-1 -- the same fp32 additions, the same bits.  (Sharing a rotation between the (b, g)
// pairs of a block -- it depends on position and pair only -- was tried: fewer, serial blocks, 30 -> 45 us at 4k x 8.)
// RAGGED (launch_cmp_pool_ragged): ceil(S / d) blocks per (b, g); block k takes token n_cmp(t_pos[b]) + k and leaves -- the whole block, before
// the barrier -- unless the sequence is live and emits that token inside its S rows.  A template flag: the scalar kernel keeps its code.
// PAGED (with RAGGED; launch_cmp_pool_paged, l = 32, d = 16): the four tensors are pools of pages.  The window of token j -- raw rows
// [16 j, 16 j + 32) -- can straddle a page boundary (j = 63: rows 1008 .. 1039), so every window row is found through its own page: entry
// r >> 10 of the sequence's table row, one of the two entries the block tests before it forms any address (the first is also the page
// of compressed row j: j >> 6 = 16 j >> 10).  The additions and their order are the ragged kernel's: the same bits.
template <typename T, bool RAGGED = false, bool PAGED = false>
__global__ __launch_bounds__(256) void cmp_pool_wide_kernel(std::conditional_t<PAGED, CmpPoolPagedParams, CmpPoolParams> P) {
    static_assert(!PAGED || RAGGED, "paged form: the ragged form only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *rk = (float *)smem;    // [l][Dk] rotated raw keys
    float *rv = rk + P.l * P.Dk;  // [l][Dv] raw values
    int j, bg;
    if constexpr (RAGGED) {
        const int per = (P.S + P.d - 1) / P.d;
        bg = (int)(blockIdx.x / per);
        const int t0 = P.t_pos[bg / P.G];  // tokens the sequence holds before the call (one scalar load: bg is uniform)
        if (t0 < 0 || t0 > min(P.t_max, P.S_max - 1) - (P.S - 1)) return;
        auto ncmp = [&](int n) { return n < P.l ? 0 : (n - P.l) / P.d + 1; };  // compressed tokens of n cached ones (ncmp_of)
        j = ncmp(t0) + (int)(blockIdx.x - bg * per);
        if (j >= ncmp(t0 + P.S) || j >= P.n_cmp_max) return;
    } else {
        const int nj = P.j1 - P.j0;
        j = P.j0 + (int)(blockIdx.x % nj);
        bg = (int)(blockIdx.x / nj);
    }
    const int r0 = j * P.d, hp = P.Dk / 2;
    const T *Kr, *Vr;
    T *Kc, *Vc;
    [[maybe_unused]] int64_t pl0 = 0, pl1 = 0;  // PAGED: the (page, group) planes of the window's first and last row
    if constexpr (PAGED) {
        // (the sequence is live and emits j inside its rows: rows r0 .. r0 + l - 1 lie below t0 + S <= the capacity, their entries in the row)
        const int g = bg % P.G;
        const int32_t *row = P.pg.table + (int64_t)(bg / P.G) * P.pg.stride;
        const int e0 = row[r0 >> 10], e1 = row[(r0 + P.l - 1) >> 10];
        if (e0 < 0 || e0 >= P.pg.n_pages || e1 < 0 || e1 >= P.pg.n_pages) return;  // (the whole block, before the barrier)
        pl0 = (int64_t)e0 * P.G + g;  // (formed in 64 bits: a pool may exceed 2 GiB)
        pl1 = (int64_t)e1 * P.G + g;
        Kr = (const T *)P.K_raw;  // the pools: a window row's plane and row inside it are added per row (prow)
        Vr = (const T *)P.V_raw;
        Kc = (T *)P.K_cmp + (pl0 * LAYER_PAGE_CMP + (j & (LAYER_PAGE_CMP - 1))) * P.Dk;
        Vc = (T *)P.V_cmp + (pl0 * LAYER_PAGE_CMP + (j & (LAYER_PAGE_CMP - 1))) * P.Dv;
    } else {
        Kr = (const T *)P.K_raw + (int64_t)bg * P.S_max * P.Dk;
        Vr = (const T *)P.V_raw + (int64_t)bg * P.S_max * P.Dv;
        Kc = (T *)P.K_cmp + ((int64_t)bg * P.n_cmp_max + j) * P.Dk;
        Vc = (T *)P.V_cmp + ((int64_t)bg * P.n_cmp_max + j) * P.Dv;
    }
    // where raw row r of the sequence lies: PAGED -- in the first page's plane up to that page's last row, behind it in the second's
    auto prow = [&](int r) {
        if constexpr (PAGED) return ((r >> 10) == (r0 >> 10) ? pl0 : pl1) * LAYER_PAGE_TOKENS + (r & (LAYER_PAGE_TOKENS - 1));
        else return (int64_t)r;
    };
    for (int it = threadIdx.x; it < P.l * hp; it += 256) {
        const int i = it / hp, pp = it - i * hp;
        const T *src = Kr + prow(r0 + i) * P.Dk + 2 * pp;
        float x0, x1;
        rope_pair<T>(Elt<T>::to_f(src[0]), Elt<T>::to_f(src[1]), pp, P.Dk, (float)(r0 + i), P.rope_base, P.inv_scale, x0, x1);
        rk[i * P.Dk + 2 * pp] = x0;
        rk[i * P.Dk + 2 * pp + 1] = x1;
    }
    for (int it = threadIdx.x; it < P.l * P.Dv; it += 256) {
        const int i = it / P.Dv, c = it - i * P.Dv;
        rv[it] = Elt<T>::to_f(Vr[prow(r0 + i) * P.Dv + c]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < P.Dk + P.Dv; c += 256) {
        const bool isv = c >= P.Dk;
        const float *col = isv ? rv + (c - P.Dk) : rk + c;
        const int stride = isv ? P.Dv : P.Dk;
        float a = 0.f;
        for (int i = 0; i < P.l; ++i) a += col[i * stride];
        if (isv) Vc[c - P.Dk] = Elt<T>::from_f(a / (float)P.l);
        else Kc[c] = Elt<T>::from_f(a / (float)P.l);
    }
}

int launch_cmp_pool(const CmpPoolParams &P, int dtype, hipStream_t st) {
    const int64_t nblk = (int64_t)P.nbg * (P.j1 - P.j0);
    if (nblk <= 0) return NSA_OK;
    NSA_CHECK_ARG(nblk < ((int64_t)1 << 31), "cmp_pool: too many blocks");
    const size_t lds = sizeof(float) * (size_t)P.l * (size_t)(P.Dk + P.Dv);
    // (a prefill pools thousands of tokens: there the 64-thread form's many small blocks fill the chip better; the wide form is for the few
    // tokens of a decode step, where the length of one block's chain is the kernel's time)
    if (lds <= 48 * 1024 && P.Dk % 2 == 0 && nblk <= 1024) {
        with_elt(dtype, [&](auto t) { hipLaunchKernelGGL(cmp_pool_wide_kernel<decltype(t)>, dim3((unsigned)nblk), dim3(256), lds, st, P); });
        NSA_LAUNCH_CHECK("cmp_pool(wide)");
        return NSA_OK;
    }
    with_elt(dtype, [&](auto t) { hipLaunchKernelGGL(cmp_pool_kernel<decltype(t)>, dim3((unsigned)nblk), dim3(64), 0, st, P); });
    NSA_LAUNCH_CHECK("cmp_pool");
    return NSA_OK;
}

// the wide form only (the few tokens of a decode call): declined where its LDS bound fails
int launch_cmp_pool_ragged(const CmpPoolParams &P, int dtype, hipStream_t st) {
    NSA_CHECK_ARG(P.t_pos && P.S >= 1 && P.G >= 1 && P.d >= 1 && P.nbg % P.G == 0, "cmp_pool(ragged): positions, S >= 1 and whole sequences");
    const int64_t nblk = (int64_t)P.nbg * ((P.S + P.d - 1) / P.d);
    if (nblk <= 0) return NSA_OK;
    const size_t lds = sizeof(float) * (size_t)P.l * (size_t)(P.Dk + P.Dv);
    NSA_CHECK_ARG(lds <= 48 * 1024 && P.Dk % 2 == 0 && nblk < ((int64_t)1 << 31),
                  "cmp_pool(ragged): the wide form holds l (Dk + Dv) floats in 48 KiB of LDS (l = %d, Dk = %d, Dv = %d)", P.l, P.Dk, P.Dv);
    with_elt(dtype, [&](auto t) { hipLaunchKernelGGL((cmp_pool_wide_kernel<decltype(t), true>), dim3((unsigned)nblk), dim3(256), lds, st, P); });
    NSA_LAUNCH_CHECK("cmp_pool(ragged)");
    return NSA_OK;
}

// the same grid over pools of pages: the default block geometry only (a window then touches at most two pages, and compressed page j >> 6
// is the page of the window's first row)
int launch_cmp_pool_paged(const CmpPoolPagedParams &P, int dtype, hipStream_t st) {
    NSA_CHECK_ARG(P.t_pos && P.S >= 1 && P.G >= 1 && P.nbg >= 1 && P.nbg % P.G == 0, "cmp_pool(paged): positions, S >= 1 and whole sequences");
    NSA_CHECK_ARG(P.l == 32 && P.d == 16 && (dtype == NSA_DT_BF16 || dtype == NSA_DT_F16), "cmp_pool(paged): bf16 / f16 and the default block geometry only");
    NSA_CHECK_ARG(P.pg.table && P.pg.n_pages >= 1 && P.pg.max_pages >= 1 && P.pg.stride >= P.pg.max_pages && P.S_max == P.pg.max_pages * LAYER_PAGE_TOKENS &&
                      P.n_cmp_max == P.pg.max_pages * LAYER_PAGE_CMP,
                  "cmp_pool(paged): a block table and the capacities max_pages * 1024 / max_pages * 64");
    const int64_t nblk = (int64_t)P.nbg * ((P.S + P.d - 1) / P.d);
    const size_t lds = sizeof(float) * (size_t)P.l * (size_t)(P.Dk + P.Dv);
    NSA_CHECK_ARG(lds <= 48 * 1024 && P.Dk % 2 == 0 && nblk < ((int64_t)1 << 31),
                  "cmp_pool(paged): the wide form holds l (Dk + Dv) floats in 48 KiB of LDS (l = %d, Dk = %d, Dv = %d)", P.l, P.Dk, P.Dv);
    with_elt<false>(dtype, [&](auto t) { hipLaunchKernelGGL((cmp_pool_wide_kernel<decltype(t), true, true>), dim3((unsigned)nblk), dim3(256), lds, st, P); });
    NSA_LAUNCH_CHECK("cmp_pool(paged)");
    return NSA_OK;
}

// backward of the pooling: raw row r receives 1/l of the gradient of every compressed token whose window contains it
// (K: rotated back by the angle of position r).  dK_cmp/dV_cmp [nbg, n_cmp, D] -> dK_raw/dV_raw [nbg, S, D] (S rows).
template <typename T>
__global__ __launch_bounds__(64) void cmp_pool_bwd_kernel(CmpPoolParams P, const T *__restrict__ dKc, const T *__restrict__ dVc,
                                                          T *__restrict__ dKr, T *__restrict__ dVr, int S, int n_cmp) {
    const int r = (int)(blockIdx.x % S);
    const int bg = (int)(blockIdx.x / S);
    // windows j with j d <= r < j d + l
    const int jhi = min(n_cmp - 1, r / P.d);
    const int jlo = max(0, (r - P.l + P.d) / P.d);  // ceil((r - l + 1) / d) for r - l + 1 > 0, else 0
    const float inv_l = 1.0f / (float)P.l;
    for (int p = threadIdx.x; p < P.Dk / 2; p += 64) {
        float g0 = 0.f, g1 = 0.f;
        for (int j = jlo; j <= jhi; ++j) {
            if (j * P.d + P.l <= r) continue;
            const T *src = dKc + ((int64_t)bg * n_cmp + j) * P.Dk + 2 * p;
            g0 += Elt<T>::to_f(src[0]);
            g1 += Elt<T>::to_f(src[1]);
        }
        g0 *= inv_l;
        g1 *= inv_l;
        const float inv_freq = powf(P.rope_base, (-2.0f * (float)p) / (float)P.Dk);
        float sn, cs;
        sincosf(((float)r * P.inv_scale) * inv_freq, &sn, &cs);
        sn = rnd<T>(sn);
        cs = rnd<T>(cs);
        T *dst = dKr + ((int64_t)bg * S + r) * P.Dk + 2 * p;
        dst[0] = Elt<T>::from_f(g0 * cs + g1 * sn);
        dst[1] = Elt<T>::from_f(g1 * cs - g0 * sn);
    }
    for (int c = threadIdx.x; c < P.Dv; c += 64) {
        float g = 0.f;
        for (int j = jlo; j <= jhi; ++j) {
            if (j * P.d + P.l <= r) continue;
            g += Elt<T>::to_f(dVc[((int64_t)bg * n_cmp + j) * P.Dv + c]);
        }
        dVr[((int64_t)bg * S + r) * P.Dv + c] = Elt<T>::from_f(g * inv_l);
    }
}

int launch_cmp_pool_bwd(const CmpPoolParams &P, const void *dKc, const void *dVc, void *dKr, void *dVr, int S, int n_cmp, int dtype,
                        hipStream_t st) {
    const int64_t nblk = (int64_t)P.nbg * S;
    if (nblk <= 0) return NSA_OK;
    NSA_CHECK_ARG(nblk < ((int64_t)1 << 31), "cmp_pool_bwd: too many blocks");
    with_elt(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(cmp_pool_bwd_kernel<T>, dim3((unsigned)nblk), dim3(64), 0, st, P, (const T *)dKc, (const T *)dVc, (T *)dKr, (T *)dVr, S, n_cmp);
    });
    NSA_LAUNCH_CHECK("cmp_pool_bwd");
    return NSA_OK;
}

// ------------------------------------------------------------------------------------------ RMSNorm of a few rows
// y = (x * rsqrt(mean(x^2) + eps)) * w, one wave per row, rounded where the eager chain rounds (llama_block_nsa.py:16-19)
template <typename T>
__device__ __forceinline__ void store8(T *p, const float (&v)[8]) {  // 8 consecutive elements, 16-byte aligned for 2-byte types
    if constexpr (sizeof(T) == 2) {
        u32x4 raw;
        T *e = (T *)&raw;
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = Elt<T>::from_f(v[j]);
        *(u32x4 *)p = raw;
    } else {
        *(f32x4 *)p = (f32x4){v[0], v[1], v[2], v[3]};
        *(f32x4 *)(p + 4) = (f32x4){v[4], v[5], v[6], v[7]};
    }
}

template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_rows_kernel(const T *__restrict__ x, const T *__restrict__ w, T *__restrict__ y, int M, int dim,
                                                           float eps, int vec) {
    const int lane = lane_id();
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const T *xr = x + (int64_t)m * dim;
    T *yr = y + (int64_t)m * dim;
    if (vec) {  // dim % 8 == 0 and 16-byte aligned rows: whole rows per load instruction
        const float r = row_rms<T>(xr, dim, true, eps);
        for (int k = lane * 8; k < dim; k += 512) {
            float xv[8], wv[8], o[8];
            load8<T>(xr + k, 8, true, xv);
            load8<T>(w + k, 8, true, wv);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = rnd<T>(xv[j] * r) * wv[j];
            store8<T>(yr + k, o);
        }
        return;
    }
    float acc = 0.f;
    for (int i = lane; i < dim; i += 64) {
        const float v = Elt<T>::to_f(xr[i]);
        acc += rnd<T>(v * v);
    }
    const float r = rms_finish<T>(acc, dim, eps);
    for (int i = lane; i < dim; i += 64) yr[i] = Elt<T>::from_f(rnd<T>(Elt<T>::to_f(xr[i]) * r) * Elt<T>::to_f(w[i]));
}

int launch_rmsnorm_rows(const void *x, const void *w, void *y, int M, int dim, float eps, int dtype, hipStream_t st) {
    if (M == 0) return NSA_OK;
    const dim3 grid((unsigned)((M + 3) / 4)), block(256);
    const int vec = dim % 8 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)y % 16 == 0;
    with_elt(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(rmsnorm_rows_kernel<T>, grid, block, 0, st, (const T *)x, (const T *)w, (T *)y, M, dim, eps, vec);
    });
    NSA_LAUNCH_CHECK("rmsnorm_rows");
    return NSA_OK;
}

// backward of y = (x r) w, r = rsqrt(mean(x^2) + eps):  dx = r (g - xh mean(g xh)),  g = dy w,  xh = x r;  dw = sum_rows dy xh.
// A workgroup owns RMS_BWD_ROWS consecutive rows (one wave per row at a time); the per-column dw sums stay in registers across the
// rows of a wave, are added over the 4 waves through LDS and leave as one fp32 partial row per workgroup; a second kernel adds the
// partial rows in fixed order (no atomics: reproducible).  dim % 8 == 0, dim <= 4096.
constexpr int RMS_BWD_ROWS = 64;
constexpr int RMS_BWD_CH = 8;  // 8-element chunks per lane: dim <= 512 * 8
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_rows_bwd_kernel(const T *__restrict__ x, const T *__restrict__ w, const T *__restrict__ dy,
                                                               T *__restrict__ dx, float *__restrict__ part, int M, int dim, float eps) {
    __shared__ float red[4][64 * 8];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int r0 = blockIdx.x * RMS_BWD_ROWS;
    float dwacc[RMS_BWD_CH][8];
#pragma unroll
    for (int c = 0; c < RMS_BWD_CH; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) dwacc[c][j] = 0.f;
    for (int m = r0 + wave; m < min(M, r0 + RMS_BWD_ROWS); m += 4) {
        const T *xr = x + (int64_t)m * dim, *gr = dy + (int64_t)m * dim;
        const float r = row_rms<T>(xr, dim, true, eps);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < RMS_BWD_CH; ++c) {
            const int k = lane * 8 + 512 * c;
            if (k < dim) {
                float xv[8], gv[8], wv[8];
                load8<T>(xr + k, 8, true, xv);
                load8<T>(gr + k, 8, true, gv);
                load8<T>(w + k, 8, true, wv);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = xv[j] * r;
                    dot = fmaf(gv[j] * wv[j], xh, dot);
                    dwacc[c][j] = fmaf(gv[j], xh, dwacc[c][j]);
                }
            }
        }
        const float mean = wave_sum(dot) / (float)dim;
        T *dr = dx + (int64_t)m * dim;
#pragma unroll
        for (int c = 0; c < RMS_BWD_CH; ++c) {
            const int k = lane * 8 + 512 * c;
            if (k < dim) {
                float xv[8], gv[8], wv[8], o[8];
                load8<T>(xr + k, 8, true, xv);
                load8<T>(gr + k, 8, true, gv);
                load8<T>(w + k, 8, true, wv);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = r * (gv[j] * wv[j] - xv[j] * r * mean);
                store8<T>(dr + k, o);
            }
        }
    }
    // dw partial of the workgroup: waves added in fixed order
#pragma unroll
    for (int c = 0; c < RMS_BWD_CH; ++c) {
        if (512 * c >= dim) break;  // uniform
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) red[wave][lane * 8 + j] = dwacc[c][j];
        __syncthreads();
        for (int i = threadIdx.x; i < 512; i += 256) {
            const int k = 512 * c + i;
            if (k < dim) part[(int64_t)blockIdx.x * dim + k] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
        }
    }
}

// dw[k] = sum over the workgroup partials, fixed order: a workgroup owns 64 columns, its 4 waves take every 4th partial row with 8
// independent accumulators (the loads of 8 rows are in flight together; one dependent chain per column made this kernel 235 us)
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_dw_reduce_kernel(const float *__restrict__ part, T *__restrict__ dw, int nparts, int dim) {
    __shared__ float red[4][64];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k < dim) {
        int p = wave;
        for (; p + 28 < nparts; p += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += part[(int64_t)(p + 4 * u) * dim + k];
        }
        for (; p < nparts; p += 4) acc[0] += part[(int64_t)p * dim + k];
    }
    red[wave][lane] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    __syncthreads();
    if (wave == 0 && k < dim) dw[k] = Elt<T>::from_f(((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
}

size_t rmsnorm_rows_bwd_workspace(int M, int dim) { return (size_t)((M + RMS_BWD_ROWS - 1) / RMS_BWD_ROWS) * dim * sizeof(float); }

template <typename T>
static int launch_rmsnorm_bwd_t(const void *x, const void *w, const void *dy, void *dx, void *dw, int M, int dim, float eps, float *part,
                                hipStream_t st) {
    const int nparts = (M + RMS_BWD_ROWS - 1) / RMS_BWD_ROWS;
    hipLaunchKernelGGL(rmsnorm_rows_bwd_kernel<T>, dim3((unsigned)nparts), dim3(256), 0, st, (const T *)x, (const T *)w, (const T *)dy, (T *)dx,
                       part, M, dim, eps);
    NSA_LAUNCH_CHECK("rmsnorm_rows_bwd");
    hipLaunchKernelGGL(rmsnorm_dw_reduce_kernel<T>, dim3((unsigned)((dim + 63) / 64)), dim3(256), 0, st, (const float *)part, (T *)dw, nparts,
                       dim);
    NSA_LAUNCH_CHECK("rmsnorm_dw_reduce");
    return NSA_OK;
}

int launch_rmsnorm_rows_bwd(const void *x, const void *w, const void *dy, void *dx, void *dw, int M, int dim, float eps, int dtype,
                            void *workspace, size_t workspace_bytes, hipStream_t st) {
    NSA_CHECK_ARG(dim % 8 == 0 && dim <= 512 * RMS_BWD_CH, "rmsnorm_rows_bwd: dim must be a multiple of 8 and <= %d (got %d)", 512 * RMS_BWD_CH, dim);
    NSA_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)dy % 16 == 0 && (uintptr_t)dx % 16 == 0,
                  "rmsnorm_rows_bwd: 16-byte aligned tensors required");
    NSA_CHECK_ARG(workspace && workspace_bytes >= rmsnorm_rows_bwd_workspace(M, dim) && (uintptr_t)workspace % 16 == 0,
                  "rmsnorm_rows_bwd: workspace too small");
    int rc = NSA_OK;
    with_elt(dtype, [&](auto t) { rc = launch_rmsnorm_bwd_t<decltype(t)>(x, w, dy, dx, dw, M, dim, eps, (float *)workspace, st); });
    return rc;
}

// ------------------------------------------------------------------------------------------ gate MLP + combine
// one wave per (b, s, g) row: q_pooled = mean_h Q -> fc1 -> silu -> fc2 -> / tau -> softmax (one-hot when the top two
// logits are more than 50 apart, nsa_attention.py:70-81) -> O = g_cmp O_cmp + g_sel O_sel + g_win O_win
template <typename T>
__global__ __launch_bounds__(256) void gate_combine_kernel(GateCombineParams P) {
    __shared__ float sqp[4][256];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= P.R) return;
    float pr[3];
    if constexpr (sizeof(T) == 2) {
        // the m7c geometry with 16-byte aligned branch outputs: every load of the row -- Q, the gate weights AND the three branch outputs (one
        // 16-byte piece per lane instead of six 2-byte loads) -- is out before the gate arithmetic starts
        const int ne = P.h * P.Dv;
        if (P.Dk == 64 && P.Hd <= 32 && P.h <= 8 && ne % 8 == 0 && ne <= 512 &&
            (((uintptr_t)P.O_cmp | (uintptr_t)P.O_sel | (uintptr_t)P.O_win | (uintptr_t)P.O_out) % 16 == 0)) {
            GateFast<T> gf;
            gf.load((const T *)P.Q + row * P.h * 64, P.h, P.Hd, P.w1, P.b1, P.w2, P.b2);
            const int64_t base = row * ne;
            const bool mine = lane * 8 < ne;
            const int off = mine ? lane * 8 : 0;
            const u32x4 rc = *(const u32x4 *)((const T *)P.O_cmp + base + off), rs = *(const u32x4 *)((const T *)P.O_sel + base + off),
                        rw = *(const u32x4 *)((const T *)P.O_win + base + off);
            gf.compute(P.h, P.Hd, P.tau, sqp[wave], pr);
            if (P.gates_out && lane < 3) P.gates_out[row * 3 + lane] = lane == 0 ? pr[0] : (lane == 1 ? pr[1] : pr[2]);
            if (mine) {
                float oc[8], os[8], ow[8];
                raw8<T>(rc, oc);
                raw8<T>(rs, os);
                raw8<T>(rw, ow);
                u32x4 outv;
                T *ov = (T *)&outv;
#pragma unroll
                for (int j = 0; j < 8; ++j) ov[j] = Elt<T>::from_f(mix3<T>(pr, oc[j], os[j], ow[j]));
                *(u32x4 *)((T *)P.O_out + base + off) = outv;
            }
            return;
        }
    }
    if (P.Dk == 64 && P.Hd <= 32 && P.h <= 8) {
        GateFast<T> gf;
        gf.load((const T *)P.Q + row * P.h * 64, P.h, P.Hd, P.w1, P.b1, P.w2, P.b2);
        gf.compute(P.h, P.Hd, P.tau, sqp[wave], pr);
    } else {
        gate_probs<T>((const T *)P.Q + row * P.h * P.Dk, P.h, P.Dk, P.Hd, P.w1, P.b1, P.w2, P.b2, P.tau, sqp[wave], pr);
    }
    if (P.gates_out && lane < 3) P.gates_out[row * 3 + lane] = lane == 0 ? pr[0] : (lane == 1 ? pr[1] : pr[2]);
    const int64_t base = row * P.h * P.Dv;
    const T *Oc = (const T *)P.O_cmp + base, *Os = (const T *)P.O_sel + base, *Ow = (const T *)P.O_win + base;
    T *Oo = (T *)P.O_out + base;
    for (int e = lane; e < P.h * P.Dv; e += 64)
        Oo[e] = Elt<T>::from_f(mix3<T>(pr, Elt<T>::to_f(Oc[e]), Elt<T>::to_f(Os[e]), Elt<T>::to_f(Ow[e])));
}

// backward of the combine: dO_i = gate_i dO (activation dtype) and dgate_i = sum_{h,d} O_i dO (fp32) per row; the gradient of
// the tiny gate MLP itself is taken by the host side from dgate.
template <typename T>
__global__ __launch_bounds__(256) void gate_combine_bwd_kernel(GateCombineParams P, const T *__restrict__ dO, const float *__restrict__ gates,
                                                               T *__restrict__ dOc, T *__restrict__ dOs, T *__restrict__ dOw,
                                                               float *__restrict__ dgates) {
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= P.R) return;
    const float g0 = gates[row * 3], g1 = gates[row * 3 + 1], g2 = gates[row * 3 + 2];
    const int64_t base = row * P.h * P.Dv;
    const T *Oc = (const T *)P.O_cmp + base, *Os = (const T *)P.O_sel + base, *Ow = (const T *)P.O_win + base;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int e = lane; e < P.h * P.Dv; e += 64) {
        const float d = Elt<T>::to_f(dO[base + e]);
        a0 = fmaf(Elt<T>::to_f(Oc[e]), d, a0);
        a1 = fmaf(Elt<T>::to_f(Os[e]), d, a1);
        a2 = fmaf(Elt<T>::to_f(Ow[e]), d, a2);
        dOc[base + e] = Elt<T>::from_f(g0 * d);
        dOs[base + e] = Elt<T>::from_f(g1 * d);
        dOw[base + e] = Elt<T>::from_f(g2 * d);
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0) {
        dgates[row * 3] = a0;
        dgates[row * 3 + 1] = a1;
        dgates[row * 3 + 2] = a2;
    }
}

int launch_gate_combine_bwd(const GateCombineParams &P, const void *dO, const float *gates, void *dOc, void *dOs, void *dOw, float *dgates,
                            int dtype, hipStream_t st) {
    if (P.R == 0) return NSA_OK;
    const dim3 grid((unsigned)((P.R + 3) / 4)), block(256);
    with_elt(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(gate_combine_bwd_kernel<T>, grid, block, 0, st, P, (const T *)dO, gates, (T *)dOc, (T *)dOs, (T *)dOw, dgates);
    });
    NSA_LAUNCH_CHECK("gate_combine_bwd");
    return NSA_OK;
}

// decode: split-KV combine of the three branches + gate + mix in one pass.  One wave per (row, head), Dv = 64 (lane = column).
// Each branch arrives either as split-KV partial records (ns > 1, layout of sel_attn_combine_kernel) or final (ns == 1).
template <typename T>
__global__ __launch_bounds__(256) void decode_finish_kernel(DecodeFinishParams P) {
    __shared__ float sqp[4][256];
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
    if (wid >= P.R * P.h) return;
    const int64_t row = wid / P.h;
    const int hh = (int)(wid - row * P.h);
    constexpr int D = 64;
    const T *Qr = (const T *)P.Q + row * P.h * P.Dk;
    const bool fast = P.Dk == 64 && P.Hd <= 32 && P.h <= 8;
    // ---- every load first (split indices are clamped instead of predicated: a clamped duplicate gets weight 0 below)
    GateFast<T> gf;
    if (fast) gf.load(Qr, P.h, P.Hd, P.w1, P.b1, P.w2, P.b2);
    float mv[3], lv[3], pv[3][16], fin[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ns = P.ns[i];
        const bool split = ns > 1;
        const float *base = split ? P.part[i] + ((row * ns) * (int64_t)P.h + hh) * (D + PART_PAD) : (const float *)nullptr;
        const int64_t sstride = (int64_t)P.h * (D + PART_PAD);
        fin[i] = split ? 0.f : Elt<T>::to_f(((const T *)P.O[i])[wid * D + lane]);
        mv[i] = (split && lane < ns) ? base[lane * sstride] : -INFINITY;
        lv[i] = (split && lane < ns) ? base[lane * sstride + 1] : 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) pv[i][s] = split ? base[min(s, ns - 1) * sstride + PART_PAD + lane] : 0.f;
    }
    // ---- arithmetic
    float pr[3];
    if (fast) gf.compute(P.h, P.Hd, P.tau, sqp[wave], pr);
    else gate_probs<T>(Qr, P.h, P.Dk, P.Hd, P.w1, P.b1, P.w2, P.b2, P.tau, sqp[wave], pr);
    float o[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float mmax = wave_max(mv[i]);
        const float w = (mv[i] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mv[i] - mmax);  // lanes >= ns: 0
        const float ltot = wave_sum(lv[i] * w);
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = fmaf(pv[i][s], __shfl(w, s, 64), acc);
        // the branch output in the activation dtype, as its own combine pass leaves it
        o[i] = P.ns[i] > 1 ? rnd<T>(acc * (ltot > 0.f ? 1.f / ltot : 0.f)) : fin[i];
    }
    if (P.gates_out && hh == 0 && lane < 3) P.gates_out[row * 3 + lane] = lane == 0 ? pr[0] : (lane == 1 ? pr[1] : pr[2]);
    ((T *)P.O_out)[wid * D + lane] = Elt<T>::from_f(mix3<T>(pr, o[0], o[1], o[2]));
}

int launch_decode_finish(const DecodeFinishParams &P, int dtype, hipStream_t st) {
    if (P.R == 0) return NSA_OK;
    NSA_CHECK_ARG(P.Dv == 64 && P.Dk <= 256 && P.Hd >= 1 && P.Hd <= 64, "decode_finish: Dv = 64, Dk <= 256, hidden <= 64 supported");
    for (int i = 0; i < 3; ++i) NSA_CHECK_ARG(P.ns[i] >= 1 && P.ns[i] <= 16 && (P.ns[i] == 1 ? P.O[i] != nullptr : P.part[i] != nullptr), "decode_finish: bad branch input");
    const dim3 grid((unsigned)((P.R * P.h + 3) / 4)), block(256);
    // (anything that is not a 16-bit dtype takes the fp32 kernel here)
    with_elt(dtype == NSA_DT_BF16 || dtype == NSA_DT_F16 ? dtype : NSA_DT_F32,
             [&](auto t) { hipLaunchKernelGGL(decode_finish_kernel<decltype(t)>, grid, block, 0, st, P); });
    NSA_LAUNCH_CHECK("decode_finish");
    return NSA_OK;
}

int launch_gate_combine(const GateCombineParams &P, int dtype, hipStream_t st) {
    if (P.R == 0) return NSA_OK;
    NSA_CHECK_ARG(P.Dk <= 256 && P.Hd >= 1 && P.Hd <= 64, "gate_combine: Dk <= 256 and 1 <= hidden <= 64 supported");
    const dim3 grid((unsigned)((P.R + 3) / 4)), block(256);
    with_elt(dtype, [&](auto t) { hipLaunchKernelGGL(gate_combine_kernel<decltype(t)>, grid, block, 0, st, P); });
    NSA_LAUNCH_CHECK("gate_combine");
    return NSA_OK;
}

// ------------------------------------------------------------------------------------------ model-level helpers (decode)
// x[b, :] = embed[tokens[b], :]
template <typename T>
__global__ __launch_bounds__(256) void embed_rows_kernel(const int32_t *__restrict__ tokens, const T *__restrict__ embed, T *__restrict__ x, int B,
                                                         int dim, int vocab) {
    const int b = blockIdx.x;
    const int tok = min(max(tokens[b], 0), vocab - 1);
    for (int i = threadIdx.x; i < dim; i += 256) x[(int64_t)b * dim + i] = embed[(int64_t)tok * dim + i];
}
int launch_embed_rows(const int32_t *tokens, const void *embed, void *x, int B, int dim, int vocab, int dtype, hipStream_t st) {
    if (B == 0) return NSA_OK;
    with_elt(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(embed_rows_kernel<T>, dim3(B), dim3(256), 0, st, tokens, (const T *)embed, (T *)x, B, dim, vocab);
    });
    NSA_LAUNCH_CHECK("embed_rows");
    return NSA_OK;
}

// next[b] = argmax_v logits[b, v] (first maximum wins).  Stage 1: grid (chunks, B), one workgroup per 4096-value chunk -> (max, index)
// partials; stage 2: one wave per row over the partials.
constexpr int ARGMAX_CHUNK = 4096;
template <typename T>
__global__ __launch_bounds__(256) void argmax_part_kernel(const T *__restrict__ logits, float *__restrict__ pv, int32_t *__restrict__ pi, int vocab) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int b = blockIdx.y, lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const T *row = logits + (int64_t)b * vocab;
    const int v0 = blockIdx.x * ARGMAX_CHUNK, v1 = min(vocab, v0 + ARGMAX_CHUNK);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = v0 + threadIdx.x; v < v1; v += 256) {
        const float x = Elt<T>::to_f(row[v]);
        if (x > best) {
            best = x;
            bi = v;
        }
    }
    const float wm = wave_max(best);
    int cand = best == wm ? bi : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    if (lane == 0) {
        sv[wave] = wm;
        si[wave] = cand;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = sv[0];
        int i = si[0];
        for (int w = 1; w < 4; ++w)
            if (sv[w] > m || (sv[w] == m && si[w] < i)) {
                m = sv[w];
                i = si[w];
            }
        pv[(int64_t)b * gridDim.x + blockIdx.x] = m;
        pi[(int64_t)b * gridDim.x + blockIdx.x] = i;
    }
}
__global__ __launch_bounds__(64) void argmax_final_kernel(const float *__restrict__ pv, const int32_t *__restrict__ pi, int32_t *__restrict__ next,
                                                         int nchunk) {
    const int b = blockIdx.x, lane = lane_id();
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < nchunk; c += 64) {
        const float x = pv[(int64_t)b * nchunk + c];
        const int i = pi[(int64_t)b * nchunk + c];
        if (x > best || (x == best && i < bi)) {
            best = x;
            bi = i;
        }
    }
    const float wm = wave_max(best);
    int cand = best == wm ? bi : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    if (lane == 0) next[b] = cand == 0x7fffffff ? 0 : cand;
}
size_t argmax_rows_workspace(int B, int vocab) { return (size_t)B * ((vocab + ARGMAX_CHUNK - 1) / ARGMAX_CHUNK) * 8; }
int launch_argmax_rows(const void *logits, int32_t *next, int B, int vocab, int dtype, void *ws, hipStream_t st) {
    if (B == 0) return NSA_OK;
    const int nchunk = (vocab + ARGMAX_CHUNK - 1) / ARGMAX_CHUNK;
    float *pv = (float *)ws;
    int32_t *pi = (int32_t *)(pv + (size_t)B * nchunk);
    const dim3 grid((unsigned)nchunk, (unsigned)B);
    with_elt(dtype, [&](auto t) { hipLaunchKernelGGL(argmax_part_kernel<decltype(t)>, grid, dim3(256), 0, st, (const decltype(t) *)logits, pv, pi, vocab); });
    NSA_LAUNCH_CHECK("argmax_part");
    hipLaunchKernelGGL(argmax_final_kernel, dim3(B), dim3(64), 0, st, (const float *)pv, (const int32_t *)pi, next, nchunk);
    NSA_LAUNCH_CHECK("argmax_final");
    return NSA_OK;
}

}  // namespace nsa
