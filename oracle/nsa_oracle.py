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
