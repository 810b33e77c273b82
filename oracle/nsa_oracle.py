"""ctypes/numpy front-end of the CPU oracle (oracle/nsa_oracle.c).

TEST INFRASTRUCTURE ONLY -- see the header of nsa_oracle.c.  Only tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module; the
product package (nsa_vibe_amd/) never does.

Function names follow the reference (nsa/core/block_index.py, selection_scorer.py,
attention_kernels.py); arrays are numpy, fp32 / int32, C-contiguous.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libnsa_oracle.so")
_lib = None


def build(force: bool = False) -> str:
    """Compile the oracle with gcc (Makefile in this directory)."""
    src = os.path.join(_HERE, "nsa_oracle.c")
    if force or not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(src):
        subprocess.check_call(["make", "-s", "-C", _HERE, "-B", "libnsa_oracle.so"])
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(_LIB_PATH)
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@dataclass
class OracleBlockMeta:
    """Same fields as the reference BlockMeta (nsa/core/block_index.py:7-22), numpy arrays."""

    l: int
    d: int
    l_sel: int
    n_sel: int
    w: int
    cmp_starts: np.ndarray
    sel_starts: np.ndarray
    M_csl_indptr: np.ndarray
    M_csl_indices: np.ndarray
    M_csl_values: np.ndarray
    M_csl_coo_indices: np.ndarray
    M_csl_coo_values: np.ndarray


def build_block_meta(seq_len: int, l: int, d: int, l_sel: int, n_sel: int, w: int) -> OracleBlockMeta:
    """nsa/core/block_index.py:74-99."""
    if l % d != 0 or l_sel % d != 0:
        raise ValueError("Require d|l and d|l_sel in M0")
    if d <= 0 or l <= 0 or l_sel <= 0:
        raise ValueError("Block parameters must be positive")
    L = lib()
    s_cmp, s_sel = C.c_int(), C.c_int()
    L.nsa_oracle_block_counts(seq_len, l, d, l_sel, C.byref(s_cmp), C.byref(s_sel))
    S_cmp, S_sel = s_cmp.value, s_sel.value
    indptr = np.zeros(S_cmp + 1, np.int32)
    cap = max(1, S_cmp * (l // l_sel + 2))
    indices = np.zeros(cap, np.int32)
    values = np.zeros(cap, np.float32)
    nnz = L.nsa_oracle_build_csr(seq_len, l, d, l_sel, _p(indptr), _p(indices), _p(values))
    indices, values = indices[:nnz].copy(), values[:nnz].copy()
    rows = np.repeat(np.arange(S_cmp, dtype=np.int32), np.diff(indptr))
    return OracleBlockMeta(
        l, d, l_sel, n_sel, w,
        (np.arange(S_cmp, dtype=np.int32) * d).astype(np.int32),
        (np.arange(S_sel, dtype=np.int32) * l_sel).astype(np.int32),
        indptr, indices, values,
        np.stack([rows, indices]).astype(np.int32), values.copy(),
    )


def compute_pcmp_all(Q, K_cmp, scale: float) -> np.ndarray:
    """nsa/core/selection_scorer.py:42-61.  Q [B,S,G,h,Dk], K_cmp [B,G,S_cmp,Dk] -> [B,S,G,h,S_cmp]."""
    Q, K_cmp = _f32(Q), _f32(K_cmp)
    B, S, G, h, Dk = Q.shape
    S_cmp = K_cmp.shape[2]
    P = np.zeros((B, S, G, h, S_cmp), np.float32)
    lib().nsa_oracle_pcmp_all(_p(Q), _p(K_cmp), _p(P), B, S, G, h, Dk, S_cmp, C.c_float(scale))
    return P


def map_pcmp_to_pslc_and_pgrp(p_cmp_all, meta: OracleBlockMeta):
    """selection_scorer.py:89-116 then .sum(dim=3) (nsa_attention.py:1091).

    p_cmp_all [..., h, S_cmp_cur] -> (p_slc [..., h, S_sel], p_grp [..., S_sel])."""
    p = _f32(p_cmp_all)
    lead = p.shape[:-2]
    h, S_cmp_cur = p.shape[-2:]
    S_sel = int(meta.sel_starts.size)
    R = int(np.prod(lead)) if lead else 1
    p_slc = np.zeros((R, h, S_sel), np.float32)
    p_grp = np.zeros((R, S_sel), np.float32)
    if S_cmp_cur > 0 and S_sel > 0:
        lib().nsa_oracle_map_pcmp_to_pgrp(
            _p(p), C.c_long(R), h, S_cmp_cur, _p(meta.M_csl_indptr), _p(meta.M_csl_indices),
            _p(meta.M_csl_values), int(meta.cmp_starts.size), S_sel, _p(p_slc), _p(p_grp))
    return p_slc.reshape(*lead, h, S_sel), p_grp.reshape(*lead, S_sel)


def select_topn_ranges_rows(p_grp_rows, t_tokens, meta: OracleBlockMeta, n_top: int,
                            force_init: bool = True, force_local: int = 2) -> np.ndarray:
    """Sequential-mode selector on a list of rows with per-row token position."""
    p = _f32(p_grp_rows)
    R, S_sel = p.shape
    t = _i32(t_tokens)
    out = np.zeros((R, n_top, 2), np.int32)
    lib().nsa_oracle_select_topn_seq(_p(p), C.c_long(R), S_sel, int(meta.l_sel), n_top, _p(t),
                                     int(bool(force_init)), int(force_local), _p(out))
    return out


def select_topn_ranges(p_grp, meta: OracleBlockMeta, n_top: int, t_token: int,
                       force_init: bool = True, force_local: int = 2) -> np.ndarray:
    """nsa/core/selection_scorer.py:124-249.  p_grp [B,G,S_sel] -> int32 [B,G,n_top,2]."""
    p = _f32(p_grp)
    B, G, S_sel = p.shape
    t = np.full(B * G, t_token, np.int32)
    return select_topn_ranges_rows(p.reshape(B * G, S_sel), t, meta, n_top, force_init,
                                   force_local).reshape(B, G, n_top, 2)


def select_topn_ranges_batched(p_grp_all, meta: OracleBlockMeta, n_top: int, S: int,
                               force_init: bool = True, force_local: int = 2) -> np.ndarray:
    """nsa/core/selection_scorer.py:255-362 (+ v2 converter :434-605).  [B,S,G,S_sel] -> [B,S,G,K,2]."""
    p = _f32(p_grp_all)
    B, S_q, G, S_sel = p.shape
    assert S_q == S
    K = C.c_int()
    L = lib()
    L.nsa_oracle_select_topn_batched(None, B, S, G, S_sel, int(meta.l_sel), n_top,
                                     int(bool(force_init)), int(force_local), None, C.byref(K))
    out = np.zeros((B, S, G, K.value, 2), np.int32)
    L.nsa_oracle_select_topn_batched(_p(p), B, S, G, S_sel, int(meta.l_sel), n_top,
                                     int(bool(force_init)), int(force_local), _p(out), C.byref(K))
    return out


def convert_indices_to_ranges_batched_v2(indices, meta: OracleBlockMeta, S: int) -> np.ndarray:
    """nsa/core/selection_scorer.py:434-605.  indices [B,S,G,K] -> int32 [B,S,G,K,2]."""
    x = _i32(indices)
    B, S_q, G, K = x.shape
    out = np.zeros((B, S_q, G, K, 2), np.int32)
    if K == 0:
        return out
    t_rows = _i32(np.broadcast_to(np.arange(S_q, dtype=np.int32)[None, :, None], (B, S_q, G)))
    lib().nsa_oracle_indices_to_ranges_v2(_p(x), C.c_long(B * S_q * G), K, int(meta.sel_starts.size),
                                          int(meta.l_sel), _p(t_rows), _p(out))
    return out


def sel_attention_masked(Q, K, V, ranges, scale: float | None = None, return_lse: bool = False):
    """nsa/core/attention_kernels.py:705-772.  fp32 math; returns O [B,S,G,h,Dv] (fp32)."""
    Q, K, V = _f32(Q), _f32(K), _f32(V)
    rg = _i32(ranges)
    B, S, G, h, Dk = Q.shape
    S_kv, Dv = K.shape[2], V.shape[3]
    n = rg.shape[3]
    if scale is None:
        scale = 1.0 / float(np.sqrt(Dk))
    O = np.zeros((B, S, G, h, Dv), np.float32)
    lse = np.zeros((B, S, G, h), np.float32)
    if S_kv > 0 and n > 0:
        lib().nsa_oracle_sel_attention_masked(_p(Q), _p(K), _p(V), _p(rg), _p(O), _p(lse), B, S, G,
                                              h, Dk, Dv, S_kv, n, C.c_float(scale))
    else:
        lse[:] = -np.inf
    return (O, lse) if return_lse else O


def sel_attention_masked_bwd(Q, K, V, ranges, dO, scale: float | None = None):
    """Gradient of sel_attention_masked w.r.t. Q, K, V (fp64 inner math)."""
    Q, K, V, dO = _f32(Q), _f32(K), _f32(V), _f32(dO)
    rg = _i32(ranges)
    B, S, G, h, Dk = Q.shape
    S_kv, Dv = K.shape[2], V.shape[3]
    n = rg.shape[3]
    if scale is None:
        scale = 1.0 / float(np.sqrt(Dk))
    dQ, dK, dV = np.zeros_like(Q), np.zeros_like(K), np.zeros_like(V)
    lib().nsa_oracle_sel_attention_masked_bwd(_p(Q), _p(K), _p(V), _p(rg), _p(dO), _p(dQ), _p(dK),
                                              _p(dV), B, S, G, h, Dk, Dv, S_kv, n, C.c_float(scale))
    return dQ, dK, dV


def band_ranges(S: int, S_kv: int, t0: int = 0, a: int = 0, dd: int = 1, c: int = 0, w: int = 2 ** 30) -> np.ndarray:
    """Key interval [lo, hi) of query row t (position t0 + t) for the sliding / compressed branches, [S,2] int32:
    hi = 0 if t0+t+1 < a else min(S_kv, (t0+t+1-a)//dd + c); lo = max(0, hi - w).
    Sliding window (nsa/core/attention_kernels.py:159-161: allowed = col <= row & col >= row-(w-1)): a=0, dd=1, c=0.
    Compressed (attention_kernels.py:118-121: num_cmp = 0 if t+1 < l else (t+1-l)//d + 1, clamped to S_cmp): a=l, dd=d, c=1."""
    e = np.arange(S, dtype=np.int64) + (t0 + 1 - a)
    hi = np.where(e < 0, 0, np.maximum(e, 0) // dd + c)
    hi = np.minimum(hi, S_kv)
    lo = np.maximum(hi - w, 0)
    return np.stack((lo, hi), axis=-1).astype(np.int32)


def band_attention(Q, K, V, *, t0: int = 0, a: int = 0, dd: int = 1, c: int = 0, w: int = 2 ** 30, scale=None,
                   return_lse: bool = False):
    """Softmax attention of row t over its key interval (band_ranges); rows with an empty interval give zeros.
    Restated through sel_attention_masked with one range per row (the masked SDPA of attention_kernels.py:163-177
    is the same math as :705-772 with this mask)."""
    Q = _f32(Q)
    B, S, G = Q.shape[:3]
    rg = np.broadcast_to(band_ranges(S, np.asarray(K).shape[2], t0, a, dd, c, w).reshape(1, S, 1, 1, 2), (B, S, G, 1, 2))
    return sel_attention_masked(Q, K, V, np.ascontiguousarray(rg), scale, return_lse)


def band_attention_bwd(Q, K, V, dO, *, t0: int = 0, a: int = 0, dd: int = 1, c: int = 0, w: int = 2 ** 30, scale=None):
    Q = _f32(Q)
    B, S, G = Q.shape[:3]
    rg = np.broadcast_to(band_ranges(S, np.asarray(K).shape[2], t0, a, dd, c, w).reshape(1, S, 1, 1, 2), (B, S, G, 1, 2))
    return sel_attention_masked_bwd(Q, K, V, np.ascontiguousarray(rg), dO, scale)


def sliding_window_attention(Q, K, V, w: int, *, t0: int = 0, scale=None):
    """nsa/core/attention_kernels.py:146-178 (w <= 0 or no keys -> zeros, :153-154)."""
    return band_attention(Q, K, V, t0=t0, a=0, dd=1, c=0, w=max(int(w), 0), scale=scale)


def batched_causal_attention_compressed(Q, K_cmp, V_cmp, l: int, d: int, *, t0: int = 0, scale=None):
    """Compressed branch with the mask of attention_kernels.py:118-123 and a true softmax over the allowed tokens
    (the reference's per-token call at :139-141 degenerates to key 0; see nsa_vibe_amd/band_attention.py)."""
    return band_attention(Q, K_cmp, V_cmp, t0=t0, a=int(l), dd=int(d), c=1, scale=scale)


def sel_attention_first_key_parity(Q, V, ranges) -> np.ndarray:
    """PARITY MODE of the reference's packed / gather executors (attention_kernels.py:181-226, 273-388): SDPA(is_causal=True) with one
    query sees only the first gathered key, so every head returns V at the start of the first non-empty range (slot order); a row
    without a range stays zero.  Pure numpy (small cases)."""
    V, r = np.asarray(V), np.asarray(ranges)
    B, S, G, h = np.asarray(Q).shape[:4]
    S_kv = V.shape[2]
    O = np.zeros((B, S, G, h, V.shape[3]), dtype=V.dtype)
    for b in range(B):
        for t in range(S):
            for g in range(G):
                for s0, e0 in r[b, t, g]:
                    s0 = min(max(int(s0), 0), S_kv)
                    e0 = min(max(int(e0), s0), S_kv)
                    if e0 > s0:
                        O[b, t, g] = V[b, g, s0]
                        break
    return O


def sel_attention_head_causal_parity(Q, K, V, ranges, scale=None) -> np.ndarray:
    """PARITY MODE of NSAAttention._sdpa_over_ranges (nsa_attention.py:1779-1855): tokens of the union of the clamped ranges in ascending
    order; SDPA(is_causal=True) sees the h heads as query positions, so head i attends the first i+1 gathered tokens; a row without a
    token gives zeros (the reference feeds a single zero key / value).  Pure numpy (small cases)."""
    Q, K, V, r = (np.asarray(x) for x in (Q, K, V, ranges))
    B, S, G, h, Dk = Q.shape
    S_kv = K.shape[2]
    sc = float(scale) if scale else 1.0 / np.sqrt(Dk)
    O = np.zeros((B, S, G, h, V.shape[3]), dtype=np.float32)
    for b in range(B):
        for t in range(S):
            for g in range(G):
                m = np.zeros(S_kv, dtype=bool)
                for s0, e0 in r[b, t, g]:
                    s0, e0 = min(max(int(s0), 0), S_kv), min(max(int(e0), 0), S_kv)
                    if e0 > s0:
                        m[s0:e0] = True
                idx = np.nonzero(m)[0][:h]
                if idx.size == 0:
                    continue
                k, v = K[b, g, idx].astype(np.float32), V[b, g, idx].astype(np.float32)
                for i in range(h):
                    nv = min(i + 1, idx.size)
                    s = (Q[b, t, g, i].astype(np.float32) @ k[:nv].T) * sc
                    p = np.exp(s - s.max())
                    O[b, t, g, i] = (p / p.sum()) @ v[:nv]
    return O.astype(V.dtype) if V.dtype == np.float32 else O


def normalise_ranges(r: np.ndarray) -> list:
    """Drop e<=s entries (SURVEY 7 hard part (c)); returns nested lists of (s,e) per row."""
    r = np.asarray(r)
    flat = r.reshape(-1, r.shape[-2], 2)
    return [[(int(s), int(e)) for s, e in row if e > s] for row in flat]


def num_threads() -> int:
    return int(lib().nsa_oracle_num_threads())


def set_num_threads(n: int) -> None:
    lib().nsa_oracle_set_num_threads(int(n))


def gate_combine(Q, O_cmp, O_sel, O_win, w1, b1, w2, b2, tau: float, return_logits: bool = False):
    """GateMLP.forward + the module's eager three-branch mix (nsa/core/nsa_attention.py:32-82, 1380-1395), fp32.
    Q [R,h,Dk] (or [...,h,Dk]), O_* [R,h,Dv]; w1 [Hd,Dk], b1 [Hd], w2 [3,Hd], b2 [3] -> gates [R,3], O [R,h,Dv] (, logits [R,3])."""
    Q, Oc, Os, Ow = _f32(Q), _f32(O_cmp), _f32(O_sel), _f32(O_win)
    w1, b1, w2, b2 = _f32(w1), _f32(b1), _f32(w2), _f32(b2)
    h, Dk, Dv, Hd = Q.shape[-2], Q.shape[-1], Oc.shape[-1], w1.shape[0]
    R = Q.size // (h * Dk)
    assert Oc.size == Os.size == Ow.size == R * h * Dv and w1.shape == (Hd, Dk) and w2.shape == (3, Hd)
    gates, O, lg = np.zeros((R, 3), np.float32), np.zeros((R, h, Dv), np.float32), np.zeros((R, 3), np.float32)
    lib().nsa_oracle_gate_combine(_p(Q), _p(Oc), _p(Os), _p(Ow), _p(w1), _p(b1), _p(w2), _p(b2), C.c_long(R), h, Dk, Dv, Hd,
                                  C.c_float(tau), _p(gates), _p(O), _p(lg))
    return (gates, O, lg) if return_logits else (gates, O)


def gate_combine_bwd(Q, O_cmp, O_sel, O_win, w1, b1, w2, b2, tau: float, dO) -> dict:
    """gradient of gate_combine for the upstream dO [R,h,Dv] -> dict dO_cmp, dO_sel, dO_win [R,h,Dv], dgates [R,3], dQ [R,h,Dk],
    dW1, db1, dW2, db2 (summed over the rows; no gradient into the MLP from a peaked, one-hot row)"""
    Q, Oc, Os, Ow, dO = _f32(Q), _f32(O_cmp), _f32(O_sel), _f32(O_win), _f32(dO)
    w1, b1, w2, b2 = _f32(w1), _f32(b1), _f32(w2), _f32(b2)
    h, Dk, Dv, Hd = Q.shape[-2], Q.shape[-1], Oc.shape[-1], w1.shape[0]
    R = Q.size // (h * Dk)
    assert Oc.size == Os.size == Ow.size == dO.size == R * h * Dv
    out = dict(dO_cmp=np.zeros((R, h, Dv), np.float32), dO_sel=np.zeros((R, h, Dv), np.float32), dO_win=np.zeros((R, h, Dv), np.float32),
               dgates=np.zeros((R, 3), np.float32), dQ=np.zeros((R, h, Dk), np.float32), dW1=np.zeros((Hd, Dk), np.float32),
               db1=np.zeros(Hd, np.float32), dW2=np.zeros((3, Hd), np.float32), db2=np.zeros(3, np.float32))
    lib().nsa_oracle_gate_combine_bwd(_p(Q), _p(Oc), _p(Os), _p(Ow), _p(w1), _p(b1), _p(w2), _p(b2), _p(dO), C.c_long(R), h, Dk, Dv, Hd,
                                      C.c_float(tau), *(_p(out[k]) for k in ("dO_cmp", "dO_sel", "dO_win", "dgates", "dQ", "dW1", "db1",
                                                                             "dW2", "db2")))
    return out


# RoPE and the compressed-token pooling (nsa/core/rope.py:6-51, nsa/core/compress_pool.py:9-38).  dtype: the activation dtype whose rounding
# chain is followed, "fp32" / "bf16" / "fp16" (or the package's NSA_DT_* code); inputs must already be representable in it.
_DT_CODE = {"fp32": 0, "bf16": 1, "fp16": 2, 0: 0, 1: 1, 2: 2}


def _pos(pos, n):
    pos = np.ascontiguousarray(np.broadcast_to(np.asarray(pos, np.int64), (n,)), np.int32)
    assert pos.min(initial=0) >= 0
    return pos


def rope_inv_freq(D: int, base: float = 10000.0) -> np.ndarray:
    """build_inv_freq (nsa/core/rope.py:6-13): fl(base ** fl(-2 i / D)), [D/2] fp32"""
    out = np.zeros(D // 2, np.float32)
    lib().nsa_oracle_rope_inv_freq(D, C.c_float(base), _p(out))
    return out


def rope(x, pos, dtype="fp32", scale: float = 1.0, base: float = 10000.0) -> np.ndarray:
    """apply_rope (nsa/core/rope.py:16-51): x [..., S, D], pos [S] (or one position per row of x) -> y like x"""
    x = _f32(x)
    D = x.shape[-1]
    R = x.size // D
    S = x.shape[-2] if x.ndim >= 2 else 1
    p = _pos(pos, S)
    p = np.ascontiguousarray(np.broadcast_to(p, (R // S, S)).reshape(R))
    y = np.zeros_like(x)
    lib().nsa_oracle_rope(_p(x), _p(p), C.c_long(R), D, C.c_float(base), C.c_float(scale), _DT_CODE[dtype], _p(y))
    return y


def rope_bwd(g, pos, dtype="fp32", scale: float = 1.0, base: float = 10000.0) -> np.ndarray:
    """gradient of rope for the upstream g [..., S, D] -> dx like g"""
    g = _f32(g)
    D = g.shape[-1]
    R = g.size // D
    S = g.shape[-2] if g.ndim >= 2 else 1
    p = np.ascontiguousarray(np.broadcast_to(_pos(pos, S), (R // S, S)).reshape(R))
    dx = np.zeros_like(g)
    lib().nsa_oracle_rope_bwd(_p(g), _p(p), C.c_long(R), D, C.c_float(base), C.c_float(scale), _DT_CODE[dtype], _p(dx))
    return dx


def cmp_pool(K_raw, V_raw, l: int, d: int, pos=None, dtype="fp32", base: float = 10000.0):
    """avg_pool_phi_rope_kv (nsa/core/compress_pool.py:9-38): K_raw [..., S, Dk], V_raw [..., S, Dv], pos [S] (default arange(S))
    -> K_cmp [..., n_cmp, Dk], V_cmp [..., n_cmp, Dv]"""
    K, V = _f32(K_raw), _f32(V_raw)
    S, Dk, Dv = K.shape[-2], K.shape[-1], V.shape[-1]
    nbg = K.size // (S * Dk)
    assert V.size == nbg * S * Dv
    p = _pos(np.arange(S) if pos is None else pos, S)
    n = 0 if S < l else (S - l) // d + 1
    Kc, Vc = np.zeros(K.shape[:-2] + (n, Dk), np.float32), np.zeros(V.shape[:-2] + (n, Dv), np.float32)
    lib().nsa_oracle_cmp_pool(_p(K), _p(V), _p(p), C.c_long(nbg), S, Dk, Dv, l, d, C.c_float(base), _DT_CODE[dtype], _p(Kc), _p(Vc))
    return Kc, Vc


def cmp_pool_bwd(dK_cmp, dV_cmp, S: int, l: int, d: int, pos=None, dtype="fp32", base: float = 10000.0):
    """gradient of cmp_pool: dK_cmp [..., n_cmp, Dk], dV_cmp [..., n_cmp, Dv] -> dK_raw [..., S, Dk], dV_raw [..., S, Dv]"""
    dK, dV = _f32(dK_cmp), _f32(dV_cmp)
    n, Dk, Dv = dK.shape[-2], dK.shape[-1], dV.shape[-1]
    lead = dK.shape[:-2]
    nbg = int(np.prod(lead, dtype=np.int64))
    assert dV.shape == lead + (n, Dv) and (n == 0 or (n - 1) * d + l <= S)
    p = _pos(np.arange(S) if pos is None else pos, S)
    dKr, dVr = np.zeros(lead + (S, Dk), np.float32), np.zeros(lead + (S, Dv), np.float32)
    lib().nsa_oracle_cmp_pool_bwd(_p(dK), _p(dV), _p(p), C.c_long(nbg), S, n, Dk, Dv, l, d, C.c_float(base), _DT_CODE[dtype], _p(dKr), _p(dVr))
    return dKr, dVr


# ---- error bounds of a RoPE kernel against the functions above (float64) ----------------------------------------------------------------
# A kernel whose inv_freq is within 1 ulp of build_inv_freq's and whose scaled position p / s is within 1 ulp (p * fl(1 / s) is) evaluates
# the fp32 angle a = fl(fl(p / s) f_i) to within  a 2^-22 + 2 ulp32(a) + 2^-22  (the 2^-22 term: its sin / cos, ~2 ulp32 each).  An element
# of a rotated pair (x0, x1) is then within  |(x0, x1)| angle_err + c ulp_T(|(x0, x1)|):  c covers the sin / cos rounded to the dtype on both
# sides (they may land one ulp_T(1) apart: (|x0| + |x1|) 2^-m <= 2 sqrt(2) ulp_T(|x|)), the two products and the sum rounded on both sides
# (3 ulp_T) and, for fp32, the device sincosf (~2 ulp, another 4.4 ulp32(|x|)):  c = 6 for bf16 / fp16, 8 for fp32.
_MANT = {"fp32": 23, "bf16": 7, "fp16": 10}
_EMIN = {"fp32": -126, "bf16": -126, "fp16": -14}
ROPE_C = {"fp32": 8.0, "bf16": 6.0, "fp16": 6.0}


def ulp(v, dtype="fp32") -> np.ndarray:
    """ulp of |v| in dtype (float64; 0 where v == 0, the subnormal spacing below the normal range)"""
    v = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    return np.where(v > 0, np.exp2(np.maximum(e, _EMIN[dtype]) - _MANT[dtype]), 0.0)


def rope_angle_err(pos, D: int, scale: float = 1.0, base: float = 10000.0) -> np.ndarray:
    """[len(pos), D/2] bound on a kernel's fp32 angle error (see above)"""
    s = scale if scale > 0 else 1.0
    a = np.asarray(pos, np.float64)[:, None] / s * rope_inv_freq(D, base).astype(np.float64)[None, :]
    return a * 2.0 ** -22 + 2.0 * ulp(a) + 2.0 ** -22


def _pair_norm(x):
    x = np.asarray(x, np.float64)
    n = np.sqrt(x[..., 0::2] ** 2 + x[..., 1::2] ** 2)
    return np.repeat(n, 2, axis=-1)


def rope_bound(x, pos, dtype="fp32", scale: float = 1.0, c=None, base: float = 10000.0) -> np.ndarray:
    """per-element bound on |kernel - rope(x, pos)| (and on rope_bwd with x = the upstream gradient): x [..., S, D], pos [S]"""
    D = x.shape[-1]
    n = _pair_norm(x)
    err = np.repeat(rope_angle_err(np.asarray(pos).reshape(-1), D, scale, base), 2, axis=-1)
    return n * err + (ROPE_C[dtype] if c is None else c) * ulp(n, dtype)


def cmp_pool_bound(K_raw, V_raw, l: int, d: int, pos=None, dtype="fp32", base: float = 10000.0):
    """per-element bounds (K_cmp, V_cmp) on a pooling kernel: the mean of the l rows' rope_bound, the fp32 sum of l terms (l 2^-24 of the
    mean magnitude) and the final rounding to the dtype on both sides (1 ulp_T)"""
    S = K_raw.shape[-2]
    p = np.arange(S) if pos is None else np.asarray(pos)
    bk, nk, nv = rope_bound(K_raw, p, dtype, base=base), _pair_norm(K_raw), np.abs(np.asarray(V_raw, np.float64))
    n = 0 if S < l else (S - l) // d + 1
    w = lambda a: np.stack([a[..., j * d: j * d + l, :].mean(-2) for j in range(n)], -2) if n else a[..., :0, :]  # noqa: E731
    mk, mv = w(nk), w(nv)
    return w(bk) + ulp(mk, dtype) + l * 2.0 ** -24 * mk, ulp(mv, dtype) + l * 2.0 ** -24 * mv


def cmp_pool_bwd_bound(dK_cmp, dV_cmp, S: int, l: int, d: int, pos=None, dtype="fp32", base: float = 10000.0):
    """per-element bounds (dK_raw, dV_raw) on a pooling backward kernel: rope_bound of the pooled gradient g = sum_j dK_cmp[j] / l (taken
    on sum_j |dK_cmp[j]| / l) with c + w + 1 for the w = ceil(l / d) windows of a row (the reference rounds each window's share and each
    partial sum to the dtype before the rotation, a kernel may sum in fp32 and round once), its fp32 sum; exactly 0 on rows in no window"""
    dK, dV = np.asarray(dK_cmp, np.float64), np.asarray(dV_cmp, np.float64)
    n = dK.shape[-2]
    gk, gv = np.zeros(dK.shape[:-2] + (S, dK.shape[-1])), np.zeros(dV.shape[:-2] + (S, dV.shape[-1]))
    ak, av = np.zeros_like(gk), np.zeros_like(gv)
    for j in range(n):
        gk[..., j * d: j * d + l, :] += dK[..., j: j + 1, :] / l
        gv[..., j * d: j * d + l, :] += dV[..., j: j + 1, :] / l
        ak[..., j * d: j * d + l, :] += np.abs(dK[..., j: j + 1, :]) / l
        av[..., j * d: j * d + l, :] += np.abs(dV[..., j: j + 1, :]) / l
    p = np.arange(S) if pos is None else np.asarray(pos)
    nk, w = _pair_norm(ak), -(-l // d)
    bk = rope_bound(ak, p, dtype, c=ROPE_C[dtype] + w + 1.0, base=base) + 2.0 ** -22 * nk
    return bk, (w + 1.0) * ulp(av, dtype) + 2.0 ** -22 * av


# ---- float64 backward of the selection / band attention with per-element error bounds (numpy only) ---------------------------------------
_U = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}  # unit roundoff u_T (half an ulp of 1)
_TINY = {k: 2.0 ** (_EMIN[k] - _MANT[k] - 1) for k in _MANT}     # half the subnormal spacing: the rounding error below the normal range
_U32 = 2.0 ** -24


def round_to(a, dtype="fp32") -> np.ndarray:
    """a rounded to the nearest value of dtype (ties to even), returned as float64"""
    a = np.asarray(a, np.float64)
    if dtype == "fp16":
        return a.astype(np.float16).astype(np.float64)
    f = np.ascontiguousarray(a.astype(np.float32))
    if dtype == "fp32":
        return f.astype(np.float64)
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape).astype(np.float64)


def _rd(x, dtype):
    """bound on |round_T(y) - y| for |y| <= x: u_T x, or half the subnormal spacing"""
    return np.maximum(_U[dtype] * x, _TINY[dtype])


def _rows_keys(a, Kc):
    """[R,h,D] x [C,D] -> [R,h,C]"""
    return np.matmul(a, Kc.T)


def _keys_sum(p, a):
    """[R,h,C] x [R,h,D] -> [C,D]: the sum over (row, head)"""
    return np.matmul(p.reshape(-1, p.shape[-1]).T, a.reshape(-1, a.shape[-1]))


def sel_attention_bwd_terms(Q, K, V, ranges, dO, dtype, scale=None, extend=False, probe_only=False, chunk=64):
    """Generator behind sel_attention_bwd_bound: the float64 terms of the backward, one dict per (b, g, chunk of query rows):
      b, g, rows [R], cols [C] (ascending keys: every key some row of the chunk selects; extend=True adds the rest of their 64-key blocks
      and the key on either side of every range, for mutants that switch a key on), cnt [R,C] (ranges of the row covering the key),
      lse [R,h], O [R,h,Dv], active [R] (rows with a non-zero dO) and, on the active rows `ar` (indices into rows), for EVERY column
      (covered or not: p = exp(s - lse) is what a kernel with a wrong mask evaluates there) p, dS, e_p, e_dS [A,h,C]; see
      sel_attention_bwd_bound for the two error terms.  probe_only: the rows with a zero dO are left out altogether."""
    Q, K, V, dO = (np.asarray(x, np.float64) for x in (Q, K, V, dO))
    rg = np.asarray(ranges, np.int64)
    B, S, G, h, Dk = Q.shape
    S_kv, Dv, n = K.shape[2], V.shape[3], rg.shape[3]
    sc = float(np.float32(1.0 / np.sqrt(Dk) if not scale else scale))  # the fp32 scale a kernel is handed
    s0 = np.clip(rg[..., 0], 0, S_kv)
    e0 = np.clip(rg[..., 1], s0, S_kv)
    for b in range(B):
        for g in range(G):
            todo = np.nonzero(dO[b, :, g].reshape(S, -1).any(axis=1))[0] if probe_only else np.arange(S)
            step = max(chunk // 4, 1) if probe_only else chunk  # probe rows lie apart: fewer of them share the keys of a chunk
            for r0 in range(0, todo.size, step):
                rows = todo[r0: r0 + step]
                R = rows.size
                st, en = s0[b, rows, g], e0[b, rows, g]  # [R,n]
                diff = np.zeros((R, S_kv + 2), np.int32)
                ri = np.repeat(np.arange(R), n)
                np.add.at(diff, (ri, st.reshape(-1)), 1)
                np.add.at(diff, (ri, en.reshape(-1)), -1)
                cnt_full = np.cumsum(diff, axis=1)[:, :S_kv]
                keep = cnt_full.any(axis=0)
                if extend and keep.any():
                    blk = np.zeros((S_kv + 63) // 64, bool)
                    blk[np.nonzero(keep)[0] // 64] = True
                    keep = np.repeat(blk, 64)[:S_kv]
                    ne = en > st
                    for k in (st[ne] - 1, en[ne]):
                        keep[k[(k >= 0) & (k < S_kv)]] = True
                cols = np.nonzero(keep)[0]
                cnt = cnt_full[:, cols]
                mask = cnt > 0
                Kc, Vc = K[b, g, cols], V[b, g, cols]
                q, do = Q[b, rows, g], dO[b, rows, g]
                s = _rows_keys(q, Kc) * sc
                sm = np.where(mask[:, None, :], s, -np.inf)
                live = mask.any(axis=1)
                m = np.where(live[:, None], sm.max(axis=2, initial=-np.inf), 0.0)
                with np.errstate(divide="ignore"):
                    lse = np.where(live[:, None], m + np.log(np.exp(sm - m[:, :, None]).sum(axis=2)), -np.inf)
                p_all = np.where(live[:, None, None], np.exp(s - np.where(live[:, None], lse, 0.0)[:, :, None]), 0.0)
                p = p_all * mask[:, None, :]
                O = np.matmul(p, Vc)
                active = do.reshape(R, -1).any(axis=1)
                out = dict(b=b, g=g, rows=rows, cols=cols, cnt=cnt, lse=lse, O=O, active=active, scale=sc)
                ar = np.nonzero(active)[0]
                if ar.size and cols.size:
                    qa, da, pa, Oa = q[ar], do[ar], p_all[ar], O[ar]
                    dP = _rows_keys(da, Vc)
                    delta = (da * Oa).sum(axis=2)
                    x = pa * (dP - delta[:, :, None])
                    dS = x * sc
                    # p: the fp32 logit (Dk products summed in fp32), scale log2(e) and lse log2(e) formed and rounded in fp32, the fused
                    # multiply-add, the hardware exp2 (1 ulp) -- the generic kernel's __expf(s scale - lse) has the same count
                    eta = 2.0 ** -22 * (np.abs(s[ar]) + np.abs(np.where(live[ar, None], lse[ar], 0.0))[:, :, None] + 1.0) \
                        + Dk * _U32 * sc * _rows_keys(np.abs(qa), np.abs(Kc))
                    e_p = _rd(pa * (1.0 + eta), dtype) + eta * pa
                    e_dP = Dv * _U32 * _rows_keys(np.abs(da), np.abs(Vc))
                    e_delta = (np.abs(da) * _rd(np.abs(Oa), dtype)).sum(axis=2) + Dv * _U32 * (np.abs(da) * np.abs(Oa)).sum(axis=2)
                    ex = eta * np.abs(x) + pa * (1.0 + eta) * (e_dP + e_delta[:, :, None])
                    pert = np.abs(dS) + sc * ex
                    e_dS = sc * ex + np.maximum(_U[dtype] * pert, _TINY[dtype] * max(sc, 1.0)) + 2.0 ** -22 * pert
                    out.update(ar=ar, p=pa, dS=dS, e_p=e_p, e_dS=e_dS, q=qa, dO=da, Kc=Kc, Vc=Vc)
                yield out


def sel_attention_bwd_bound(Q, K, V, ranges, dO, dtype, scale=None, probe_only=False):
    """Float64 backward of sel_attention_masked with a per-element bound on what a kernel of activation type T = dtype may differ by.
    Inputs must already be representable in T.  -> (dQ, dK, dV), (bQ, bK, bV), (O, lse): gradients and bounds shaped like Q, K, V, the
    forward output O [B,S,G,h,Dv] and lse [B,S,G,h] (-inf on rows without a key), all float64.  Rows whose dO is zero add no term;
    probe_only=True skips them altogether (a probe phase, dO on every s-th row, then costs its probe rows only) and leaves their O at 0
    and their lse at -inf.

    Per (row, head, selected key), with s = scale q.k, p = exp(s - lse), dP = dO.v, delta = sum_dv dO O, dS = p (dP - delta) scale:
        dV[key] += p dO      dK[key] += dS q      dQ[row, head] += dS k.
    A kernel is given the T-rounded O and the fp32 lse of THIS forward (no forward error enters) and rounds where its header says
    (sel_attn_bwd_mfma.hip, band_attn_mfma.hip, sel_attn_generic.hip); rd_T(y) = max(u_T |y|, half the subnormal spacing of T) is one
    rounding to T, u_T = 2^-8 / 2^-11 / 2^-24 for bf16 / fp16 / fp32.  Each term of the bound is one of those points:
      eta     relative error of the fp32 p: the logit's Dk-term fp32 sum (Dk 2^-24 scale sum|q||k|), the fp32 constants scale log2(e)
              and lse log2(e), the fused multiply-add and the exp2 instruction: 2^-22 (|s| + |lse| + 1) in all
      e_p     = rd_T(p (1 + eta)) + eta p            P is rounded to T as the MFMA operand of dV  (c = 1: one rounding)
      e_delta = sum_dv |dO| rd_T(O) + Dv 2^-24 sum_dv |dO||O|      O enters as the rounded forward output; the fp32 row sum
      e_dP    = Dv 2^-24 sum_dv |dO||v|              the fp32 sum of dP
      e_dS    = scale (eta |x| + p (e_dP + e_delta)) + rd_T(dS') + 2^-22 |dS'|,  x = p (dP - delta), dS' = |dS| + the first term:
              dS is rounded to T as the MFMA operand of dK and dQ (c = 1; before the scale in the dK kernel, after it in the dQ
              kernels: the same relative rounding), the fp32 products around it
      bV = sum e_p |dO| + (N + 2) 2^-24 sum (p + e_p)|dO|                    N terms summed in fp32, in any order (splits, atomics)
      bK = sum e_dS |q| + (N + 2) 2^-24 sum (|dS| + e_dS)|q|                 the same, and the final multiplication by scale
      bQ = sum e_dS |k| + N 2^-24 sum (|dS| + e_dS)|k| + rd_T(|dQ| + those)  dQ is stored in T
    The sums run over the selected (row, head, key) terms only: where none lands, gradient and bound are 0 and a kernel must write an
    exact zero.  The bound does not depend on the summation order, so it holds for the atomics of the generic kernel as well."""
    Q = np.asarray(Q, np.float64)
    B, S, G, h, Dk = Q.shape
    S_kv, Dv = np.asarray(K).shape[2], np.asarray(V).shape[3]
    dQ, bQ = np.zeros((B, S, G, h, Dk)), np.zeros((B, S, G, h, Dk))
    dK, bK, aK = (np.zeros((B, G, S_kv, Dk)) for _ in range(3))
    dV, bV, aV = (np.zeros((B, G, S_kv, Dv)) for _ in range(3))
    nKV = np.zeros((B, G, S_kv))
    O, lse = np.zeros((B, S, G, h, Dv)), np.full((B, S, G, h), -np.inf)
    for c in sel_attention_bwd_terms(Q, K, V, ranges, dO, dtype, scale, probe_only=probe_only):
        b, g, rows, cols = c["b"], c["g"], c["rows"], c["cols"]
        O[b, rows, g], lse[b, rows, g] = c["O"], c["lse"]
        if "ar" not in c:
            continue
        ar = c["ar"]
        mk = (c["cnt"][ar] > 0)[:, None, :]
        p, dS, e_p, e_dS = (c[k] * mk for k in ("p", "dS", "e_p", "e_dS"))
        aq, ado, aKc = np.abs(c["q"]), np.abs(c["dO"]), np.abs(c["Kc"])
        dV[b, g, cols] += _keys_sum(p, c["dO"])
        dK[b, g, cols] += _keys_sum(dS, c["q"])
        bV[b, g, cols] += _keys_sum(e_p, ado)
        aV[b, g, cols] += _keys_sum(p + e_p, ado)
        bK[b, g, cols] += _keys_sum(e_dS, aq)
        aK[b, g, cols] += _keys_sum(np.abs(dS) + e_dS, aq)
        nKV[b, g, cols] += h * mk[:, 0, :].sum(axis=0)
        dq = np.matmul(dS, c["Kc"])
        eq = np.matmul(e_dS, aKc)
        eq += mk.sum(axis=2)[:, :, None] * _U32 * np.matmul(np.abs(dS) + e_dS, aKc)
        dQ[b, rows[ar], g] = dq
        bQ[b, rows[ar], g] = np.where(mk.any(axis=2)[:, :, None], eq + _rd(np.abs(dq) + eq, dtype), 0.0)
    bV += (nKV[..., None] + 2.0) * _U32 * aV
    bK += (nKV[..., None] + 2.0) * _U32 * aK
    return (dQ, dK, dV), (bQ, bK, bV), (O, lse)


def band_ranges_rows(B: int, S: int, G: int, S_kv: int, **band) -> np.ndarray:
    """band_ranges as the one-range-per-row ranges tensor [B,S,G,1,2] of the selection functions"""
    return np.ascontiguousarray(np.broadcast_to(band_ranges(S, S_kv, **band).reshape(1, S, 1, 1, 2), (B, S, G, 1, 2)))


def band_attention_bwd_bound(Q, K, V, dO, dtype, *, t0: int = 0, a: int = 0, dd: int = 1, c: int = 0, w: int = 2 ** 30, scale=None):
    """sel_attention_bwd_bound of the sliding / compressed band (band_ranges: one key interval per row)"""
    B, S, G = np.asarray(Q).shape[:3]
    rg = band_ranges_rows(B, S, G, np.asarray(K).shape[2], t0=t0, a=a, dd=dd, c=c, w=w)
    return sel_attention_bwd_bound(Q, K, V, rg, dO, dtype, scale)
