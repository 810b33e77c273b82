"""Sliding-window and compressed branch attention on MI355X (band attention kernel).

Operator names and argument order follow the reference (nsa/core/attention_kernels.py):
    sliding_window_attention(Q, K, V, w)                      :146-178  (banded causal softmax, keys [t-w+1 .. t])
    batched_causal_attention_compressed(Q, K_cmp, V_cmp, l, d) :106-143  (keys [0, num_cmp(t)), num_cmp from the
                                                                          emission schedule :118-121)
Layouts: Q [B,S,G,h,Dk], K/V [B,G,S_kv,D*] -> O [B,S,G,h,Dv] in V's dtype.  `t0` is the absolute position of query
row 0 (0 for prefill; a decode step passes S = 1 and t0 = position of the new token), so the same operator serves
the decode calls of nsa_attention.py:674-703.  The compressed branch uses the true softmax over the emitted tokens
-- the reference's per-token SDPA call (is_causal=True with one query, :139-141) attends key 0 only, a quirk that
is deliberately not reproduced.
Both are one C-ABI call (nsa_band_attn_fwd); the backward (nsa_band_attn_bwd) takes dQ with a dense query-major kernel and
dK/dV with the key-block-major selection backward kernels (the band written as one [lo, hi) range per row).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .selection_attention import _bwd_variant, _positions_to, _ragged_positions, _unit_rows_pool
from ._native import _DT, _need_gpu, _needs_grad, _scale_arg, _stream, _unit_rows, _ws_args, workspace, workspace_at

_W_INF = 2 ** 30


def band_ranges(S: int, S_kv: int, t0: int, a: int, dd: int, c: int, w: int, device) -> torch.Tensor:
    """[S,2] int32 key interval [lo, hi) of every query row (the rule of nsa_band_attn_fwd, include/nsa_sel_hip.h)."""
    e = torch.arange(S, device=device, dtype=torch.int64) + (t0 + 1 - a)
    hi = torch.where(e < 0, torch.zeros_like(e), torch.div(e.clamp_min(0), dd, rounding_mode="floor") + c).clamp(max=S_kv)
    lo = (hi - w).clamp_min(0)
    return torch.stack((lo, hi), dim=-1).to(torch.int32)


def _fwd(Q, K, V, band, scale, variant, want_lse, t_pos=None, t_max=None):
    who = "band attention"
    if t_pos is not None:  # ragged form: the positions are checked before anything native is touched
        if Q.dim() != 5:
            raise RuntimeError("band attention: expected Q[B,S,G,h,Dk] K[B,G,S_kv,Dk] V[B,G,S_kv,Dv]")
        if band[0] != 0:
            raise RuntimeError(f"{who}: t_pos and a non-zero t0 are mutually exclusive")
        if Q.requires_grad or K.requires_grad or V.requires_grad:
            raise RuntimeError(f"{who}: per-sequence positions (t_pos) are forward only: no input may require grad")
        t_pos, t_max, host = _ragged_positions(who, t_pos, t_max, Q.shape[0], Q.shape[1])
    elif t_max is not None:
        raise RuntimeError(f"{who}: t_max is the bound of t_pos and needs it")
    dev = _need_gpu(Q, K, V)
    if not (Q.dtype == K.dtype == V.dtype) or Q.dtype not in _DT:
        raise RuntimeError(f"band attention: Q/K/V must share a dtype in fp32/bf16/fp16 (got {Q.dtype},{K.dtype},{V.dtype})")
    if Q.dim() != 5 or K.dim() != 4 or V.dim() != 4:
        raise RuntimeError("band attention: expected Q[B,S,G,h,Dk] K[B,G,S_kv,Dk] V[B,G,S_kv,Dv]")
    B, S, G, h, Dk = Q.shape
    S_kv, Dv = K.shape[2], V.shape[3]
    if K.shape[:2] != (B, G) or V.shape[:3] != (B, G, S_kv) or K.shape[3] != Dk:
        raise RuntimeError("band attention: inconsistent shapes")
    t0, a, dd, c, w = band
    Qc, (Kc, *ks), (Vc, *vs) = Q.contiguous(), _unit_rows(K), _unit_rows(V)
    O = torch.empty((B, S, G, h, Dv), dtype=V.dtype, device=dev)
    lse = torch.empty((B, S, G, h), dtype=torch.float32, device=dev) if want_lse else None
    if O.numel() == 0:
        return O, lse, (Qc, Kc, Vc)
    L = _lib.lib()
    dt = _DT[Q.dtype]
    ws = workspace(dev, L.nsa_band_attn_fwd_workspace(B, S, G, h, Dk, Dv, dt), "band")
    name, at, row0 = "nsa_band_attn_fwd", (), (int(t0),)  # row s at token t0 + s ...
    if t_pos is not None:  # ... or, in the ragged form, at t_pos[b] + s: the positions stand behind lse, and there is no t0
        if host is None and t_pos.device != dev:
            raise RuntimeError("all tensors must be on the same device")
        pos = _positions_to(dev, t_pos, host)
        name, at, row0 = "nsa_band_attn_fwd_ragged", (pos.data_ptr(), t_max), ()
    rc = getattr(L, name)(Qc.data_ptr(), Kc.data_ptr() if S_kv else None, Vc.data_ptr() if S_kv else None, O.data_ptr(),
              lse.data_ptr() if lse is not None else None, *at, B, S, G, h, Dk, Dv, S_kv, *ks, *vs, *row0, int(a), int(dd), int(c),
              int(min(w, _W_INF)), dt, _scale_arg(scale), int(variant), *_ws_args(ws), _stream(dev))
    _lib.check(rc, name)
    return O, lse, (Qc, Kc, Vc)


def _fwd_paged(Q, K_pool, V_pool, block_table, band, scale, want_lse, t_pos, t_max):
    """the ragged forward over pools of pages (nsa_band_attn_fwd_paged); everything is checked before anything native is touched"""
    who = "band attention (paged)"
    if Q.dim() != 5:
        raise RuntimeError(f"{who}: expected Q[B,S,G,h,Dk] K_pool[n_pages,G,page_rows,Dk] V_pool[n_pages,G,page_rows,Dv]")
    B, S, G, h, Dk = Q.shape
    bt = block_table
    if not isinstance(bt, torch.Tensor) or bt.device.type == "cpu" or bt.dtype != torch.int32 or bt.dim() != 2:
        raise RuntimeError(f"{who}: block_table must be a device int32 tensor [B, max_pages] (it is never read back); got "
                           f"{getattr(bt, 'dtype', type(bt))} {tuple(getattr(bt, 'shape', ()))} on {getattr(bt, 'device', 'the host')}")
    if bt.shape[0] != B or bt.shape[1] < 1:
        raise RuntimeError(f"{who}: block_table has shape {tuple(bt.shape)} for B = {B} sequences: expected [B, max_pages >= 1]")
    if bt.stride(1) != 1:
        raise RuntimeError(f"{who}: block_table must have a contiguous last dimension (stride {bt.stride(1)})")
    if band[0] != 0:
        raise RuntimeError(f"{who}: t_pos and a non-zero t0 are mutually exclusive")
    if t_pos is None:
        raise RuntimeError(f"{who}: block_table needs the per-sequence positions t_pos")
    if Q.requires_grad or K_pool.requires_grad or V_pool.requires_grad:
        raise RuntimeError(f"{who}: paged caches (block_table) are forward only: no input may require grad")
    t_pos, t_max, host = _ragged_positions(who, t_pos, t_max, B, S)
    dev = _need_gpu(Q, K_pool, V_pool, bt)
    if host is None and t_pos.device != dev:
        raise RuntimeError("all tensors must be on the same device")
    if not (Q.dtype == K_pool.dtype == V_pool.dtype) or Q.dtype not in _DT:
        raise RuntimeError(f"{who}: Q and the pools must share a dtype (got {Q.dtype},{K_pool.dtype},{V_pool.dtype})")
    if K_pool.dim() != 4 or V_pool.dim() != 4:
        raise RuntimeError(f"{who}: expected Q[B,S,G,h,Dk] K_pool[n_pages,G,page_rows,Dk] V_pool[n_pages,G,page_rows,Dv]")
    page_rows = K_pool.shape[2]
    (Kk, *ks), (Vv, *vs) = _unit_rows_pool(who, "K_pool", K_pool, page_rows), _unit_rows_pool(who, "V_pool", V_pool, page_rows)
    n_pages, max_pages, Dv = Kk.shape[0], bt.shape[1], Vv.shape[3]
    if Vv.shape[0] != n_pages or not (Kk.shape[1] == Vv.shape[1] == G) or Kk.shape[3] != Dk:
        raise RuntimeError(f"{who}: the two pools must share n_pages and G = {G}, with Dk = {Dk} columns in K_pool")
    t0, a, dd, c, w = band
    O = torch.empty((B, S, G, h, Dv), dtype=V_pool.dtype, device=dev)
    lse = torch.empty((B, S, G, h), dtype=torch.float32, device=dev) if want_lse else None
    if O.numel() == 0:
        return O, lse
    L = _lib.lib()
    dt = _DT[Q.dtype]
    Qc = Q.contiguous()
    pos = _positions_to(dev, t_pos, host)
    ws = workspace(dev, L.nsa_band_attn_fwd_paged_workspace(B, S, G, h, Dk, Dv, dt), "band")
    rc = L.nsa_band_attn_fwd_paged(Qc.data_ptr(), Kk.data_ptr(), Vv.data_ptr(), bt.data_ptr(), bt.stride(0), n_pages, max_pages, page_rows, O.data_ptr(),
                                   lse.data_ptr() if lse is not None else None, pos.data_ptr(), t_max, B, S, G, h, Dk, Dv, *ks, *vs, int(a), int(dd), int(c),
                                   int(min(w, _W_INF)), dt, _scale_arg(scale), *_ws_args(ws), _stream(dev))
    _lib.check(rc, "nsa_band_attn_fwd_paged")
    return O, lse


class _BandAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, K, V, band, scale, variant, bwd_variant):
        O, lse, (Qc, Kc, Vc) = _fwd(Q, K, V, band, scale, variant, True)
        ctx.save_for_backward(Qc, Kc, Vc, O, lse)
        ctx.band, ctx.scale = band, scale
        ctx.bwd_variant = _bwd_variant(variant, bwd_variant)
        return O

    @staticmethod
    def backward(ctx, dO):
        Qc, Kc, Vc, O, lse = ctx.saved_tensors
        dev = Qc.device
        B, S, G, h, Dk = Qc.shape
        S_kv, Dv = Kc.shape[2], Vc.shape[3]
        t0, a, dd, c, w = ctx.band
        dO = dO.contiguous()
        dQ = torch.empty_like(Qc)
        dK = torch.empty((B, G, S_kv, Dk), dtype=torch.float32, device=dev)
        dV = torch.empty((B, G, S_kv, Dv), dtype=torch.float32, device=dev)
        L = _lib.lib()
        dt = _DT[Qc.dtype]
        wptr, wsize, _ = workspace_at(dev, L.nsa_band_attn_bwd_workspace(B, S, G, h, Dk, Dv, S_kv, dt, ctx.bwd_variant), "band_bwd", 256)
        rc = L.nsa_band_attn_bwd(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), O.data_ptr(), lse.data_ptr(), dO.data_ptr(), dQ.data_ptr(),
                                 dK.data_ptr(), dV.data_ptr(), B, S, G, h, Dk, Dv, S_kv, *_unit_rows(Kc)[1:], *_unit_rows(Vc)[1:],
                                 int(t0), int(a), int(dd), int(c), int(min(w, _W_INF)), dt, _scale_arg(ctx.scale),
                                 int(ctx.bwd_variant), wptr, wsize, _stream(dev))
        _lib.check(rc, "nsa_band_attn_bwd")
        return dQ, dK.to(Kc.dtype), dV.to(Vc.dtype), None, None, None, None


def band_attention_hip(Q, K, V, *, t0: int = 0, a: int = 0, dd: int = 1, c: int = 0, w: int = _W_INF,
                       scale: Optional[float] = None, variant: int = 0, return_lse: bool = False,
                       bwd_variant: Optional[int] = None, t_pos=None, t_max: Optional[int] = None, block_table=None):
    """Row t attends keys [max(0, hi - w), hi), hi = (t0+t+1 >= a) ? min(S_kv, (t0+t+1-a)//dd + c) : 0.

    variant: 0 auto, 1 generic, 2 MFMA (forward); bwd_variant: the same for the backward, None = 0 unless variant is 1.
    t_pos / t_max (ragged batch, nsa_band_attn_fwd_ragged; forward only, exclusive with a non-zero t0): sequence b's row t sits at
    t_pos[b] + t.  t_pos is a device int32 tensor [B] (t_max, a host bound of t_pos[b] + S - 1, is then required: nothing is read back) or
    host integers (t_max defaults to max + S - 1).  A sequence with a negative position, one beyond t_max, or one whose last row would need
    keys past S_kv gives zero rows and lse = -inf.
    block_table (paged caches, nsa_band_attn_fwd_paged; forward only, needs t_pos): K / V are POOLS [n_pages, G, page_rows, D] -- views with
    page, group and row strides are used in place, the last dimension must be contiguous; page_rows, read from their shape, is a power of two
    in [32, 65536] -- and block_table is a device int32 tensor [B, max_pages] with a contiguous last dimension, never read on the host: key
    row r of sequence b is row r % page_rows of pool page block_table[b, r // page_rows].  The capacity is max_pages * page_rows.  A
    sequence is inactive (zero rows, lse = -inf, nothing read) under the ragged rule, or when a table entry it needs -- those covering its
    key rows from the window start of its first row to the end of its last -- lies outside [0, n_pages); entries outside that set are never
    read.  O and lse are those of the ragged call on the contiguous caches bit for bit.  bf16 / f16 at D = 64 or 128 only: anything else
    raises the library's message, there is no fallback.  variant is not used."""
    band = (int(t0), int(a), int(dd), int(c), int(w))
    if block_table is not None:
        O, lse = _fwd_paged(Q, K, V, block_table, band, scale, return_lse, t_pos, t_max)
        return (O, lse) if return_lse else O
    if t_pos is not None or t_max is not None:
        O, lse, _ = _fwd(Q, K, V, band, scale, variant, return_lse, t_pos, t_max)
        return (O, lse) if return_lse else O
    if _needs_grad(Q, K, V):
        if return_lse:
            raise RuntimeError("return_lse is not available on the autograd path")
        if K.shape[2] == 0:
            return Q.new_zeros(Q.shape[:-1] + (V.shape[-1],)) + 0.0 * Q.sum()
        return _BandAttnFn.apply(Q, K, V, band, scale, variant, bwd_variant)
    O, lse, _ = _fwd(Q, K, V, band, scale, variant, return_lse)
    return (O, lse) if return_lse else O


def sliding_window_attention(Q, K, V, w: int, *, t0: int = 0, scale: Optional[float] = None, variant: int = 0, t_pos=None,
                             t_max: Optional[int] = None, block_table=None):
    """Keys [t-w+1 .. t] of row t (reference attention_kernels.py:146-178; w <= 0 or no keys -> zeros, :153-154).
    t_pos / t_max: per-sequence positions of a ragged batch; block_table: K / V are pools of pages (band_attention_hip; pages of 1024
    rows share their page ids with selection_decode_paged)."""
    return band_attention_hip(Q, K, V, t0=t0, a=0, dd=1, c=0, w=max(int(w), 0), scale=scale, variant=variant, t_pos=t_pos, t_max=t_max,
                              block_table=block_table)


def batched_causal_attention_compressed(Q, K_cmp, V_cmp, l: int, d: int, *, t0: int = 0, scale: Optional[float] = None,
                                        variant: int = 0, t_pos=None, t_max: Optional[int] = None, block_table=None):
    """Keys [0, num_cmp(t)), num_cmp(t) = 0 if t+1 < l else (t+1-l)//d + 1, clamped to S_cmp (attention_kernels.py:118-121).
    t_pos / t_max: per-sequence positions of a ragged batch; block_table: K_cmp / V_cmp are pools of pages (band_attention_hip; pages of
    64 rows at d = 16 share their page ids with selection_decode_paged)."""
    return band_attention_hip(Q, K_cmp, V_cmp, t0=t0, a=int(l), dd=int(d), c=1, w=_W_INF, scale=scale, variant=variant, t_pos=t_pos,
                              t_max=t_max, block_table=block_table)


def batched_causal_attention_compressed_first_key_parity(Q, K_cmp, V_cmp, l: int, d: int, *, t0: int = 0):
    """PARITY MODE, opt-in: what the reference's own batched_causal_attention_compressed returns on CPU (attention_kernels.py:106-143).
    It evaluates every token through SDPA(is_causal=True) with ONE query (:139-141), so only compressed token 0 is visible:
    O[b,t,g,h,:] = V_cmp[b,g,0] when num_cmp(t) > 0, zeros otherwise (max |quirk - true softmax| ~ 5 on random inputs: g13 goldens keep it as
    O_ref_quirk).  The same first-key rule as the selection branch's packed executor, so it runs on nsa_sel_attn_first_key_parity with the
    single range [0, num_cmp(t)) per row.  Q and K_cmp do not influence the result.  Inference only."""
    from .selection_attention import selection_attention_first_key_parity

    B, S, G = Q.shape[:3]
    rg = band_ranges(S, K_cmp.shape[2], int(t0), int(l), int(d), 1, _W_INF, Q.device)  # [S, 2]: [0, num_cmp(t))
    ranges = rg.view(1, S, 1, 1, 2).expand(B, S, G, 1, 2).contiguous()
    return selection_attention_first_key_parity(Q, K_cmp, V_cmp, ranges)
