"""Selection attention executor on MI355X: `selection_attention_hip(Q, K, V, ranges)`.

Same call signature and result layout as every selection executor of the reference
(nsa/core/attention_kernels.py:181-186,273-278,391-396,705-710 and the native slot
nsa/kernels/cuda_sel_kernel/__init__.py:47-52):

    Q [B,S,G,h,Dk], K [B,G,S_kv,Dk], V [B,G,S_kv,Dv], ranges [B,S,G,n,2] int32/int64
    -> O [B,S,G,h,Dv] in V's dtype, on V's device.

Semantics = the reference's masked path (attention_kernels.py:705-772): softmax over the UNION
of the clamped ranges, non-causal inside the selected set, empty rows -> zeros.  Inputs are
borrowed (the caller's ranges tensor is never modified -- the reference clamps an int64 ranges
tensor in place, attention_kernels.py:723-724).  Differentiable: backward runs the HIP backward
kernel (dQ, dK, dV) with P recomputed from the forward's log-sum-exp.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .block_index import build_block_meta
from .kv_cache import n_cmp_at
from ._native import _DT, _need_gpu, _needs_grad, _plan_ints, _scale_arg, _sel_mode, _stream, _unit_rows, _ws_args, workspace


def _prep_ranges(ranges: torch.Tensor) -> torch.Tensor:
    """[B,S,G,n,2] int32 contiguous.  Like the reference's range normaliser (kernels/triton_sel_kernel/__init__.py:17-39) extra singleton
    dimensions are squeezed away and a 4-D tensor is taken as batch-less; the clamp to [0,S_kv] happens in the kernels."""
    while ranges.dim() > 5:
        d = next((i for i in range(ranges.dim()) if ranges.size(i) == 1), None)
        if d is None:
            break
        ranges = ranges.squeeze(d)
    if ranges.dim() == 4:
        ranges = ranges.unsqueeze(0)
    if ranges.dim() != 5 or ranges.shape[-1] != 2:
        raise ValueError(f"ranges must be [B,S,G,n,2] (start,end), got {tuple(ranges.shape)}")
    if ranges.dtype != torch.int32:
        ranges = ranges.to(torch.int32)  # a copy: the caller's tensor stays untouched
    return ranges.contiguous()


def _fwd(Q, K, V, ranges, scale, variant, want_lse):
    dev = _need_gpu(Q, K, V, ranges)
    if not (Q.dtype == K.dtype == V.dtype) or Q.dtype not in _DT:
        raise RuntimeError(f"selection_attention_hip: Q/K/V must share a dtype in fp32/bf16/fp16 (got {Q.dtype},{K.dtype},{V.dtype})")
    if Q.dim() != 5 or K.dim() != 4 or V.dim() != 4 or ranges.dim() != 5 or ranges.shape[-1] != 2:
        raise RuntimeError("selection_attention_hip: expected Q[B,S,G,h,Dk] K[B,G,S_kv,Dk] V[B,G,S_kv,Dv] ranges[B,S,G,n,2]")
    B, S, G, h, Dk = Q.shape
    S_kv, Dv = K.shape[2], V.shape[3]
    n = ranges.shape[3]
    if K.shape[:2] != (B, G) or V.shape[:3] != (B, G, S_kv) or K.shape[3] != Dk or ranges.shape[:3] != (B, S, G):
        raise RuntimeError("selection_attention_hip: inconsistent shapes")
    Qc, (Kc, *ks), (Vc, *vs), rg = Q.contiguous(), _unit_rows(K), _unit_rows(V), _prep_ranges(ranges)
    O = torch.empty((B, S, G, h, Dv), dtype=V.dtype, device=dev)
    lse = torch.empty((B, S, G, h), dtype=torch.float32, device=dev) if want_lse else None
    if O.numel() == 0:
        return O, lse, (Qc, Kc, Vc, rg)
    L = _lib.lib()
    dt = _DT[Q.dtype]
    ws = workspace(dev, L.nsa_sel_attn_fwd_workspace_kv(B, S, G, h, Dk, Dv, S_kv, n, dt), "attn")
    rc = L.nsa_sel_attn_fwd(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), rg.data_ptr(), O.data_ptr(),
                            lse.data_ptr() if lse is not None else None, B, S, G, h, Dk, Dv, S_kv, n, *ks, *vs,
                            dt, _scale_arg(scale), int(variant), *_ws_args(ws), _stream(dev))
    _lib.check(rc, "nsa_sel_attn_fwd")
    return O, lse, (Qc, Kc, Vc, rg)


class _SelAttnFn(torch.autograd.Function):
    """autograd wrapper (pattern of the reference's Triton wrapper,
    nsa/kernels/triton_sel_kernel/__init__.py:125-142: save Q,K,V,ranges; backward -> dQ,dK,dV,None)."""

    @staticmethod
    def forward(ctx, Q, K, V, ranges, scale, variant, bwd_variant):
        O, lse, (Qc, Kc, Vc, rg) = _fwd(Q, K, V, ranges, scale, variant, True)
        ctx.save_for_backward(Qc, Kc, Vc, rg, O, lse)
        ctx.scale = scale
        ctx.bwd_variant = _bwd_variant(variant, bwd_variant)
        return O

    @staticmethod
    def backward(ctx, dO):
        Qc, Kc, Vc, rg, O, lse = ctx.saved_tensors
        dev = Qc.device
        B, S, G, h, Dk = Qc.shape
        S_kv, Dv = Kc.shape[2], Vc.shape[3]
        dO = dO.contiguous()
        dQ = torch.empty_like(Qc)
        dK = torch.empty((B, G, S_kv, Dk), dtype=torch.float32, device=dev)
        dV = torch.empty((B, G, S_kv, Dv), dtype=torch.float32, device=dev)
        L = _lib.lib()
        ws = workspace(dev, L.nsa_sel_attn_bwd_workspace(B, S, G, h, Dk, Dv, S_kv, _DT[Qc.dtype], ctx.bwd_variant), "attn_bwd")
        rc = L.nsa_sel_attn_bwd(Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), rg.data_ptr(), O.data_ptr(),
                                lse.data_ptr(), dO.data_ptr(), dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(),
                                B, S, G, h, Dk, Dv, S_kv, rg.shape[3], *_unit_rows(Kc)[1:], *_unit_rows(Vc)[1:],
                                _DT[Qc.dtype], _scale_arg(ctx.scale), int(ctx.bwd_variant),
                                *_ws_args(ws), _stream(dev))
        _lib.check(rc, "nsa_sel_attn_bwd")
        return dQ, dK.to(Kc.dtype), dV.to(Vc.dtype), None, None, None, None


def _bwd_variant(variant: int, bwd_variant: Optional[int]) -> int:
    """Kernel choice of the backward: an explicit bwd_variant, else 0 (auto) unless the forward was asked for the generic kernel
    (variant 1 keeps the generic kernels on both passes)."""
    if bwd_variant is None:
        return 0 if variant != 1 else 1
    if bwd_variant not in (0, 1, 2):
        raise ValueError(f"bwd_variant must be None, 0, 1 or 2 (got {bwd_variant})")
    return int(bwd_variant)


def selection_attention_hip(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, ranges: torch.Tensor, *,
                            scale: Optional[float] = None, variant: int = 0, return_lse: bool = False,
                            bwd_variant: Optional[int] = None):
    """The MI355X selection executor (drop-in for selection_attention_cuda / grouped_selection_attention_masked).

    variant: 0 auto (MFMA kernel when dtype/shape allow, else the generic kernel), 1 generic, 2 MFMA.
    bwd_variant: the same choice for the backward; None = 0 (auto) unless variant is 1.  2 raises where the MFMA backward does not
    cover the shape (bf16/f16, Dk = Dv = 64 or 128, h <= 16, 16-byte aligned K/V strides)."""
    if _needs_grad(Q, K, V):
        if return_lse:
            raise RuntimeError("return_lse is not available on the autograd path")
        return _SelAttnFn.apply(Q, K, V, ranges, scale, variant, bwd_variant)
    O, lse, _ = _fwd(Q, K, V, ranges, scale, variant, return_lse)
    return (O, lse) if return_lse else O


def selection_attention_first_key_parity(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, ranges: torch.Tensor) -> torch.Tensor:
    """PARITY MODE, opt-in: what the reference's default packed / gather executors return (grouped_selection_attention_packed,
    attention_kernels.py:273-388; grouped_selection_attention, :181-226).  Their SDPA call is `is_causal=True` with one query, so only
    the first gathered key is visible and O[b,t,g,h,:] = V[b,g,start of the first non-empty range] for every head (zeros when the row
    has none).  Same executor signature as selection_attention_hip; Q and K do not influence the result.  Inference only."""
    dev = _need_gpu(Q, K, V)
    if _needs_grad(V):
        raise RuntimeError("selection_attention_first_key_parity is an inference-only parity mode")
    B, S, G, h, _ = Q.shape
    S_kv, Dv = V.shape[2], V.shape[3]
    (Vv, *vs), rg = _unit_rows(V), _prep_ranges(ranges)
    O = torch.empty((B, S, G, h, Dv), dtype=V.dtype, device=dev)
    rc = _lib.lib().nsa_sel_attn_first_key_parity(Vv.data_ptr(), rg.data_ptr(), O.data_ptr(), B, S, G, h, Dv, S_kv, rg.shape[3], *vs,
                                                  _DT[V.dtype], _stream(dev))
    _lib.check(rc, "nsa_sel_attn_first_key_parity")
    return O


def selection_attention_head_causal_parity(Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, ranges: torch.Tensor, *,
                                           scale: Optional[float] = None) -> torch.Tensor:
    """PARITY MODE, opt-in: what NSAAttention._sdpa_over_ranges returns (nsa/core/nsa_attention.py:1779-1855), the gather route the
    reference's decode and sequential prefill fall to (and the only one left under NSA_FORCE_PARITY=1).  It hands SDPA the h heads of a
    group as the query LENGTH with is_causal=True, so head i attends the first i+1 tokens of the gathered union (ascending token
    order); rows without a token give zeros.  Executor signature ([B,S,G,...] tensors); inference only."""
    dev = _need_gpu(Q, K, V)
    if _needs_grad(Q, K, V):
        raise RuntimeError("selection_attention_head_causal_parity is an inference-only parity mode")
    if not (Q.dtype == K.dtype == V.dtype) or Q.dtype not in _DT:
        raise RuntimeError("selection_attention_head_causal_parity: Q/K/V must share a dtype in fp32/bf16/fp16")
    B, S, G, h, Dk = Q.shape
    S_kv, Dv = V.shape[2], V.shape[3]
    Qc, (Kk, *ks), (Vv, *vs), rg = Q.contiguous(), _unit_rows(K), _unit_rows(V), _prep_ranges(ranges)
    if rg.shape[:3] != (B, S, G) or Kk.shape[:3] != (B, G, S_kv):
        raise RuntimeError("selection_attention_head_causal_parity: inconsistent shapes")
    O = torch.empty((B, S, G, h, Dv), dtype=V.dtype, device=dev)
    rc = _lib.lib().nsa_sel_attn_head_causal_parity(Qc.data_ptr(), Kk.data_ptr(), Vv.data_ptr(), rg.data_ptr(), O.data_ptr(), B, S, G, h, Dk,
                                                    Dv, S_kv, rg.shape[3], *ks, *vs, _DT[Q.dtype], _scale_arg(scale), _stream(dev))
    _lib.check(rc, "nsa_sel_attn_head_causal_parity")
    return O


def selection_decode_step(Q: torch.Tensor, K_cmp: torch.Tensor, K: torch.Tensor, V: torch.Tensor, meta, n_top: int, t_token: int,
                          *, scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                          ranges_out: Optional[torch.Tensor] = None):
    """One decode step of the selected branch in a single native call.

    Q [B,1,G,h,Dk], K_cmp [B,G,S_cmp,Dk], K/V [B,G,S_kv,D] (views of a preallocated cache are fine), meta = BlockMeta
    covering t_token.  Returns (O [B,1,G,h,Dv], ranges [B,G,n_top,2] int32) = what the decode branch of the
    reference computes with compute_pcmp_all -> map_pcmp_to_pslc_batched -> sum(dim=3) -> select_topn_ranges ->
    selection executor (nsa/core/nsa_attention.py:651-672, 704-830), sequential-selector semantics."""
    L = _lib.lib()
    return _selection_decode(L.nsa_sel_decode_step, L.nsa_sel_decode_step_workspace, "decode", False, Q, K_cmp, K, V, meta, n_top, t_token, scale,
                             out, ranges_out)


def _selection_decode(call, size, tag: str, rows: bool, Q, K_cmp, K, V, meta, n_top, t0, scale, out, ranges_out):
    """the body of selection_decode_step (rows = False: S = 1, ranges without the S axis, no S in the C signatures) and selection_decode_rows.
    (The single step is host bound at small shapes -- tools/prof_decode_step_host.py -- so the workspace and scale idioms stay inline here.)"""
    dev = _need_gpu(Q, K_cmp, K, V)
    B, S, G, h, Dk = Q.shape
    S_kv, Dv = K.shape[2], V.shape[3]
    S_cmp, S_sel = K_cmp.shape[2], meta.S_sel
    if not rows and S != 1:
        raise RuntimeError("selection_decode_step: decode requires S == 1")
    if rows and S_kv < t0 + S:
        raise RuntimeError("selection_decode_rows: the cache must hold the S tokens t0 .. t0 + S - 1")
    Qc, (Kc, *cs), (Kk, *ks), (Vv, *vs) = Q.contiguous(), _unit_rows(K_cmp), _unit_rows(K), _unit_rows(V)
    O = out if out is not None else torch.empty((B, S, G, h, Dv), dtype=V.dtype, device=dev)
    rg = ranges_out if ranges_out is not None else torch.empty((B, S, G, n_top, 2) if rows else (B, G, n_top, 2), dtype=torch.int32, device=dev)
    if rows and O.numel() == 0:
        return O, rg
    dt = _DT[Q.dtype]
    s = (S,) if rows else ()
    ws = workspace(dev, size(B, *s, G, h, Dk, Dv, S_cmp, S_sel, n_top, dt) + 16, tag)
    wptr = (ws.data_ptr() + 15) & ~15
    cptr, crows, cvals = meta.device_csc(dev)
    rc = call(Qc.data_ptr(), Kc.data_ptr(), Kk.data_ptr(), Vv.data_ptr(), cptr.data_ptr(), crows.data_ptr(), cvals.data_ptr(), rg.data_ptr(),
              O.data_ptr(), B, *s, G, h, Dk, Dv, S_cmp, S_sel, S_kv, int(meta.l), int(meta.d), int(meta.l_sel), int(n_top), int(t0), *cs, *ks, *vs, dt,
              float(scale) if scale else 0.0, wptr, ws.numel() - (wptr - ws.data_ptr()), _stream(dev))
    _lib.check(rc, call.__name__)
    return O, rg


def selection_decode_step_plan(B: int, G: int, h: int, Dk: int, Dv: int, S_cmp: int, S_sel: int, S_kv: int, n_top: int,
                               dtype: torch.dtype = torch.bfloat16) -> dict:
    """What selection_decode_step does with a shape under the current tuning switches (nsa_sel_decode_step_plan; default block geometry,
    aligned contiguous-row inputs): {"launches": 1 exactly when the call is the one-launch step, otherwise an estimate > 1 of the separate route's launches, "form": 0 logits in registers /
    1 four chunks per wave / 2 one-pass / -1 step declined, "nsplit": workgroups per row (0 when declined)}.  Launches no kernel, but asks the HIP runtime for the current device's CU count (which initialises the runtime): the
    answer is for the device that is current when it is called."""
    ints = _plan_ints("nsa_sel_decode_step_plan", 3, int(B), int(G), int(h), int(Dk), int(Dv), int(S_cmp), int(S_sel), int(S_kv), int(n_top), _DT[dtype])
    return dict(zip(("launches", "form", "nsplit"), ints))


def selection_decode_rows(Q: torch.Tensor, K_cmp: torch.Tensor, K: torch.Tensor, V: torch.Tensor, meta, n_top: int, t0: int,
                          *, scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                          ranges_out: Optional[torch.Tensor] = None):
    """The decode step of the selected branch for S consecutive tokens per sequence in a single native call (nsa_sel_decode_rows).

    Q [B,S,G,h,Dk] holds the queries of tokens t0 .. t0 + S - 1; K_cmp [B,G,S_cmp,Dk] and K/V [B,G,S_kv,D] are the cache AFTER those S
    tokens were appended (S_kv >= t0 + S) and meta = BlockMeta of t0 + S tokens.  Row s computes what selection_decode_step computes at
    t = t0 + s on the cache truncated to t + 1 tokens (its own n_cmp(t) compressed rows, sequential selection at t, K/V[:t+1]).
    Returns (O [B,S,G,h,Dv], ranges [B,S,G,n_top,2] int32)."""
    L = _lib.lib()
    return _selection_decode(L.nsa_sel_decode_rows, L.nsa_sel_decode_rows_workspace, "decode_rows", True, Q, K_cmp, K, V, meta, n_top, t0, scale,
                             out, ranges_out)


def selection_decode_rows_plan(B: int, S: int, G: int, h: int, Dk: int, Dv: int, S_cmp: int, S_sel: int, S_kv: int, n_top: int,
                               dtype: torch.dtype = torch.bfloat16) -> dict:
    """What selection_decode_rows does with a shape under the current tuning switches (nsa_sel_decode_rows_plan; default block geometry,
    aligned contiguous-row inputs, a cache of exactly S_kv = t0 + S tokens): {"launches": 1 exactly when the call is the one-launch rows
    form, otherwise an estimate > 1 of the separate launches, "form": 0 logits in registers / 1 four chunks per wave / -1 declined}."""
    ints = _plan_ints("nsa_sel_decode_rows_plan", 2, int(B), int(S), int(G), int(h), int(Dk), int(Dv), int(S_cmp), int(S_sel), int(S_kv), int(n_top),
                      _DT[dtype])
    return dict(zip(("launches", "form"), ints))


def _ragged_positions(who: str, t_pos, t_max, B: int, S: int):
    """the per-sequence positions of a ragged call, checked before any native call -> (positions, t_max, host): a device int32 tensor [B]
    as given (host = None; t_max is then required: nothing is read back), or host integers (a sequence or a CPU tensor) as a list with
    t_max defaulting to max + S - 1; the caller copies the list to the device without blocking (_positions_to)"""
    if isinstance(t_pos, torch.Tensor) and t_pos.device.type != "cpu":
        if t_pos.dtype != torch.int32 or t_pos.dim() != 1 or t_pos.numel() != B or not t_pos.is_contiguous():
            raise RuntimeError(f"{who}: t_pos on the device must be a contiguous int32 tensor [B = {B}] (got {t_pos.dtype}, {tuple(t_pos.shape)})")
        if t_max is None:
            raise RuntimeError(f"{who}: t_max (a host upper bound of t_pos[b] + S - 1) is required with device positions: they are never read back")
        host = None
    else:
        if isinstance(t_pos, torch.Tensor):
            if t_pos.is_floating_point() or t_pos.is_complex() or t_pos.dtype == torch.bool or t_pos.dim() != 1:
                raise RuntimeError(f"{who}: t_pos must hold integers, one per sequence (got {t_pos.dtype}, {tuple(t_pos.shape)})")
            host = [int(v) for v in t_pos.tolist()]
        else:
            try:
                host = list(t_pos)
            except TypeError:
                raise RuntimeError(f"{who}: t_pos must be a device int32 tensor [B] or a sequence of B integers") from None
            if any(isinstance(v, bool) or not isinstance(v, int) for v in host):
                raise RuntimeError(f"{who}: t_pos must hold integers")
        if len(host) != B:
            raise RuntimeError(f"{who}: t_pos has {len(host)} entries for B = {B} sequences")
        if any(v >= 2 ** 30 or v < -2 ** 31 for v in host):
            raise RuntimeError(f"{who}: t_pos out of range")
        if t_max is None:
            t_max = max([v for v in host if v >= 0], default=0) + S - 1
    t_max = int(t_max)
    if t_max < 0 or t_max >= 2 ** 30:
        raise RuntimeError(f"{who}: t_max must be in [0, 2^30)")
    return t_pos, t_max, host


def _positions_to(dev, t_pos, host):
    """device int32 [B] of the positions: the caller's device tensor, or the host integers through pinned memory (a non-blocking copy)"""
    if host is None:
        return t_pos
    return torch.tensor(host, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)


def selection_decode_ragged_plan(B: int, S: int, G: int, h: int, Dk: int, Dv: int, S_cmp: int, S_sel: int, S_kv: int, n_top: int, t_max: int,
                                 dtype: torch.dtype = torch.bfloat16) -> dict:
    """What selection_decode_ragged does with a shape whose largest live row sits at t_max (nsa_sel_decode_ragged_plan; default block
    geometry, aligned inputs): {"launches": 1, "form": 0 logits in registers / 1 four chunks per wave / 3 the long-row form (tuning switch
    DECODE_LONG = 1 only: a t_max beyond the unsplit forms, up to 131,071)}, or {"launches": 0, "form": -1} where the call declines --
    there is no other native route with per-sequence positions."""
    ints = _plan_ints("nsa_sel_decode_ragged_plan", 2, int(B), int(S), int(G), int(h), int(Dk), int(Dv), int(S_cmp), int(S_sel), int(S_kv), int(n_top),
                      _DT[dtype], int(t_max))
    return dict(zip(("launches", "form"), ints))


def selection_decode_ragged(Q: torch.Tensor, K_cmp: torch.Tensor, K: torch.Tensor, V: torch.Tensor, meta, n_top: int, t_pos, *,
                            t_max: Optional[int] = None, scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                            ranges_out: Optional[torch.Tensor] = None):
    """The decode step of the selected branch for a batch whose sequences sit at DIFFERENT positions, in one native call
    (nsa_sel_decode_ragged: the rows form of the one-launch step with a device array of positions).

    Q [B,S,G,h,Dk] (1 <= S <= 16): row (b, s) is token t_pos[b] + s of sequence b and computes what selection_decode_step computes at that
    token on sequence b's cache truncated to it.  K_cmp [B,G,S_cmp,Dk], K/V [B,G,S_kv,D] and meta give the caches' capacity: the block
    metadata of at least t_max + 1 tokens, and the rows the buffers may be read up to.
    t_pos: a device int32 tensor [B] -- then t_max, a host upper bound of t_pos[b] + S - 1, is required and nothing is synchronised -- or
    host integers (a sequence or a CPU tensor), copied to the device without blocking, with t_max defaulting to max + S - 1.
    A sequence with t_pos[b] < 0 or t_pos[b] + S - 1 > min(t_max, S_kv - 1) is inactive: it reads nothing and its O and ranges rows are
    zeros (the padding slot of a serving batch).
    Where the native call declines (selection_decode_ragged_plan: launches 0 -- a t_max beyond the unsplit forms unless the tuning switch
    DECODE_LONG = 1 lets the long-row form take it, up to t_max = 131,071) host positions run one selection_decode_rows call per active
    sequence on that sequence's views (same ranges, O from that route); device positions raise RuntimeError with the library's message.
    Returns (O [B,S,G,h,Dv], ranges [B,S,G,n_top,2] int32).  Inference only."""
    who = "selection_decode_ragged"
    if Q.dim() != 5:
        raise RuntimeError(f"{who}: expected Q[B,S,G,h,Dk]")
    B, S, G, h, Dk = Q.shape
    t_pos, t_max, host = _ragged_positions(who, t_pos, t_max, B, S)
    dev = _need_gpu(Q, K_cmp, K, V)
    if host is None and t_pos.device != dev:
        raise RuntimeError("all tensors must be on the same device")
    S_kv, Dv = K.shape[2], V.shape[3]
    S_cmp, S_sel = K_cmp.shape[2], meta.S_sel
    O = out if out is not None else torch.empty((B, S, G, h, Dv), dtype=V.dtype, device=dev)
    rg = ranges_out if ranges_out is not None else torch.empty((B, S, G, n_top, 2), dtype=torch.int32, device=dev)
    if O.numel() == 0:
        return O, rg
    dt = _DT[Q.dtype]
    if host is not None and selection_decode_ragged_plan(B, S, G, h, Dk, Dv, S_cmp, S_sel, S_kv, n_top, t_max, Q.dtype)["launches"] == 0:
        # declined (a t_max beyond the unsplit forms, fp32, ...): the positions are known here, so each active sequence takes the rows call
        O.zero_()
        rg.zero_()
        for b, t0 in enumerate(host):
            if t0 < 0 or t0 + S - 1 > min(t_max, S_kv - 1):
                continue
            n_tok = t0 + S
            n_c = n_cmp_at(n_tok, meta.l, meta.d)
            selection_decode_rows(Q[b:b + 1], K_cmp[b:b + 1, :, :min(n_c, S_cmp)], K[b:b + 1, :, :n_tok], V[b:b + 1, :, :n_tok],
                                  build_block_meta(n_tok, meta.l, meta.d, meta.l_sel, meta.n_sel, meta.w), n_top, t0, scale=scale,
                                  out=O[b:b + 1], ranges_out=rg[b:b + 1])
        return O, rg
    L = _lib.lib()
    Qc, (Kc, *cs), (Kk, *ks), (Vv, *vs) = Q.contiguous(), _unit_rows(K_cmp), _unit_rows(K), _unit_rows(V)
    pos = _positions_to(dev, t_pos, host)
    cptr, crows, cvals = meta.device_csc(dev)
    ws = workspace(dev, L.nsa_sel_decode_ragged_workspace(B, S, G, h, Dk, Dv, S_cmp, S_sel, n_top, dt), "decode_ragged")
    rc = L.nsa_sel_decode_ragged(Qc.data_ptr(), Kc.data_ptr() if S_cmp else None, Kk.data_ptr(), Vv.data_ptr(), cptr.data_ptr(), crows.data_ptr(),
                                 cvals.data_ptr(), rg.data_ptr(), O.data_ptr(), pos.data_ptr(), t_max, B, S, G, h, Dk, Dv, S_cmp, S_sel, S_kv,
                                 int(meta.l), int(meta.d), int(meta.l_sel), int(n_top), *cs, *ks, *vs, dt, _scale_arg(scale), *_ws_args(ws), _stream(dev))
    _lib.check(rc, "nsa_sel_decode_ragged")
    return O, rg


PAGE_TOKENS = 1024  # tokens per cache page of the paged decode step: one scorer chunk (64 compressed rows), 16 selection blocks


def selection_decode_paged_plan(B: int, S: int, G: int, h: int, Dk: int, Dv: int, S_cmp: int, S_sel: int, max_pages: int, n_top: int, t_max: int,
                                dtype: torch.dtype = torch.bfloat16, page_tokens: int = PAGE_TOKENS) -> dict:
    """What selection_decode_paged does with a shape whose largest live row sits at t_max (nsa_sel_decode_paged_plan): the plan of
    selection_decode_ragged_plan for a capacity of max_pages * 1024 tokens -- {"launches": 1, "form": 0 / 1 / 3}, or {"launches": 0,
    "form": -1} where the call declines (a shape the ragged call declines, or a page size other than 1024)."""
    ints = _plan_ints("nsa_sel_decode_paged_plan", 2, int(B), int(S), int(G), int(h), int(Dk), int(Dv), int(S_cmp), int(S_sel), int(max_pages),
                      int(page_tokens), int(n_top), _DT[dtype], int(t_max))
    return dict(zip(("launches", "form"), ints))


def _unit_rows_pool(who: str, name: str, X: torch.Tensor, rows: int):
    """a pool [n_pages, G, rows, D] as the C ABI takes it -> (X, its page, group and row strides); a pool is never copied"""
    if X.dim() != 4 or X.shape[2] != rows:
        raise RuntimeError(f"{who}: {name} must be [n_pages, G, {rows}, D] (got {tuple(X.shape)})")
    if X.stride(-1) != 1:
        raise RuntimeError(f"{who}: {name} must have a contiguous last dimension (a pool is used in place, never copied)")
    return X, X.stride(0), X.stride(1), X.stride(2)


def selection_decode_paged(Q: torch.Tensor, Kc_pool: torch.Tensor, K_pool: torch.Tensor, V_pool: torch.Tensor, block_table: torch.Tensor, meta,
                           n_top: int, t_pos, t_max: Optional[int] = None, out: Optional[torch.Tensor] = None,
                           ranges_out: Optional[torch.Tensor] = None, *, scale: Optional[float] = None):
    """selection_decode_ragged over PAGED caches, in one native call (nsa_sel_decode_paged).

    K_pool / V_pool [n_pages, G, 1024, D] and Kc_pool [n_pages, G, 64, D] are pools of pages (views with page, group and row strides are
    fine; the last dimension must be contiguous); block_table is a device int32 tensor [B, max_pages] whose entry [b, j] is the pool page
    that holds tokens [1024 j, 1024 j + 1024) of sequence b's K and V and compressed rows [64 j, 64 j + 64) of its K_cmp.  Its last
    dimension must be contiguous; it is never read back.  Q, meta, n_top, t_pos and t_max are those of selection_decode_ragged, with
    max_pages * 1024 as the caches' capacity: meta covers at least min(t_max, capacity - 1) + 1 tokens.
    A sequence is inactive -- zero O and ranges rows, nothing read -- under the ragged rule (t_pos[b] < 0, or t_pos[b] + S - 1 >
    min(t_max, capacity - 1)) or when one of the table entries it needs, j = 0 .. (t_pos[b] + S - 1) >> 10, lies outside [0, n_pages).
    For a table that scatters contiguous caches into pages the result is selection_decode_ragged's on those caches bit for bit.
    There is no per-sequence fallback: the contiguous operators cannot read a pool, so a declined shape (selection_decode_paged_plan:
    launches 0; a t_max beyond the unsplit forms is one unless the tuning switch DECODE_LONG = 1, which reaches t_max = 131,071) raises RuntimeError with the library's message.  Returns (O [B,S,G,h,Dv], ranges [B,S,G,n_top,2] int32).  Inference only."""
    who = "selection_decode_paged"
    if Q.dim() != 5:
        raise RuntimeError(f"{who}: expected Q[B,S,G,h,Dk]")
    B, S, G, h, Dk = Q.shape
    bt = block_table
    if not isinstance(bt, torch.Tensor) or bt.device.type == "cpu" or bt.dtype != torch.int32 or bt.dim() != 2:
        raise RuntimeError(f"{who}: block_table must be a device int32 tensor [B, max_pages] (it is never read back); got "
                           f"{getattr(bt, 'dtype', type(bt))} {tuple(getattr(bt, 'shape', ()))} on {getattr(bt, 'device', 'the host')}")
    if bt.shape[0] != B or bt.shape[1] < 1:
        raise RuntimeError(f"{who}: block_table has shape {tuple(bt.shape)} for B = {B} sequences: expected [B, max_pages >= 1]")
    if bt.stride(1) != 1:
        raise RuntimeError(f"{who}: block_table must have a contiguous last dimension (stride {bt.stride(1)})")
    t_pos, t_max, host = _ragged_positions(who, t_pos, t_max, B, S)
    dev = _need_gpu(Q, Kc_pool, K_pool, V_pool, bt)
    if host is None and t_pos.device != dev:
        raise RuntimeError("all tensors must be on the same device")
    (Kc, *cs), (Kk, *ks), (Vv, *vs) = (_unit_rows_pool(who, "Kc_pool", Kc_pool, PAGE_TOKENS // 16), _unit_rows_pool(who, "K_pool", K_pool, PAGE_TOKENS),
                                      _unit_rows_pool(who, "V_pool", V_pool, PAGE_TOKENS))
    n_pages, max_pages, Dv = Kk.shape[0], bt.shape[1], Vv.shape[3]
    if Kc.shape[0] != n_pages or Vv.shape[0] != n_pages or not (Kc.shape[1] == Kk.shape[1] == Vv.shape[1] == G) or Kk.shape[3] != Dk or Kc.shape[3] != Dk:
        raise RuntimeError(f"{who}: the three pools must share n_pages and G = {G}, with Dk = {Dk} columns in Kc_pool and K_pool")
    S_cmp, S_sel = min(int(meta.S_cmp), max_pages * (PAGE_TOKENS // 16)), meta.S_sel
    O = out if out is not None else torch.empty((B, S, G, h, Dv), dtype=V_pool.dtype, device=dev)
    rg = ranges_out if ranges_out is not None else torch.empty((B, S, G, n_top, 2), dtype=torch.int32, device=dev)
    if O.numel() == 0:
        return O, rg
    L = _lib.lib()
    dt = _DT[Q.dtype]
    Qc = Q.contiguous()
    pos = _positions_to(dev, t_pos, host)
    cptr, crows, cvals = meta.device_csc(dev)
    ws = workspace(dev, L.nsa_sel_decode_paged_workspace(B, S, G, h, Dk, Dv, S_cmp, S_sel, n_top, dt), "decode_paged")
    rc = L.nsa_sel_decode_paged(Qc.data_ptr(), Kc.data_ptr(), Kk.data_ptr(), Vv.data_ptr(), bt.data_ptr(), bt.stride(0), n_pages, max_pages, PAGE_TOKENS,
                                cptr.data_ptr(), crows.data_ptr(), cvals.data_ptr(), rg.data_ptr(), O.data_ptr(), pos.data_ptr(), t_max, B, S, G, h, Dk, Dv,
                                S_cmp, S_sel, int(meta.l), int(meta.d), int(meta.l_sel), int(n_top), *cs, *ks, *vs, dt, _scale_arg(scale), *_ws_args(ws),
                                _stream(dev))
    _lib.check(rc, "nsa_sel_decode_paged")
    return O, rg


def select_and_attend(p_grp: torch.Tensor, Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, meta, n_top: int, *,
                      mode: str = "batched", t0: int = 0, force_init: bool = True, force_local: int = 2,
                      scale: Optional[float] = None, return_lse: bool = False):
    """Prefill (inference): top-n selection from the group scores and the selection attention in ONE native call
    (nsa_sel_select_attn_fwd: the select kernel and the attention kernel back to back, or -- tuning switch SEL_FUSE = 1 -- the selector
    inside the attention kernel on the MFMA route).  p_grp [B,S,G,S_sel] fp32.
    mode "batched" = select_topn_ranges_batched semantics (selection_scorer.py:255-362), "sequential" = select_topn_ranges per
    row at token t0 + s (:124-249).  Returns (ranges [B,S,G,W,2] int32, O [B,S,G,h,Dv]) -- bit-identical to
    select_topn_ranges_batched / select_topn_ranges_rows followed by selection_attention_hip."""
    dev = _need_gpu(p_grp, Q, K, V)
    if _needs_grad(Q, K, V):
        raise RuntimeError("select_and_attend is the inference form; with autograd use select_topn_ranges_* + selection_attention_hip")
    B, S, G, h, Dk = Q.shape
    S_kv, Dv, S_sel = K.shape[2], V.shape[3], p_grp.shape[-1]
    if p_grp.shape[:3] != (B, S, G) or p_grp.dtype != torch.float32:
        raise RuntimeError("select_and_attend: p_grp must be fp32 [B,S,G,S_sel]")
    md, W = _sel_mode(mode, S_sel, meta.l_sel, n_top, S, force_init, force_local)
    Qc, (Kc, *ks), (Vc, *vs), pg = Q.contiguous(), _unit_rows(K), _unit_rows(V), p_grp.contiguous()
    ranges = torch.empty((B, S, G, W, 2), dtype=torch.int32, device=dev)
    O = torch.empty((B, S, G, h, Dv), dtype=V.dtype, device=dev)
    lse = torch.empty((B, S, G, h), dtype=torch.float32, device=dev) if return_lse else None
    if O.numel() == 0 or W == 0:
        O.zero_()
        return (ranges, O, lse) if return_lse else (ranges, O)
    L = _lib.lib()
    dt = _DT[Q.dtype]
    ws = workspace(dev, L.nsa_sel_attn_fwd_workspace_kv(B, S, G, h, Dk, Dv, S_kv, W, dt), "attn")
    rc = L.nsa_sel_select_attn_fwd(pg.data_ptr(), int(t0), None, S_sel, int(meta.l_sel), int(n_top), int(bool(force_init)), int(force_local),
                                   md, S, ranges.data_ptr(), W, Qc.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), O.data_ptr(),
                                   lse.data_ptr() if lse is not None else None, B, S, G, h, Dk, Dv, S_kv, *ks, *vs,
                                   dt, _scale_arg(scale), *_ws_args(ws), _stream(dev))
    _lib.check(rc, "nsa_sel_select_attn_fwd")
    return (ranges, O, lse) if return_lse else (ranges, O)


# the reference's executor names, bound to the HIP implementation
grouped_selection_attention_masked = selection_attention_hip
selection_attention_cuda = selection_attention_hip
# the "merged-range varlen gather" executors (attention_kernels.py:391-542, 545-702) compute the same masked softmax through an FA-2
# varlen pack; here the gather is what the kernels do anyway
selection_attention_varlen_all = selection_attention_hip
selection_attention_varlen_all_v2 = selection_attention_hip
# the default packed / gather executors are first-gathered-key functions (see selection_attention_first_key_parity): their names are
# bound to that parity mode, NOT to the semantic executor, so that code calling them by name keeps the reference's numbers
grouped_selection_attention_packed = selection_attention_first_key_parity
grouped_selection_attention = selection_attention_first_key_parity


def hip_sel_available() -> bool:
    """Counterpart of cuda_sel_available() (nsa/kernels/cuda_sel_kernel/__init__.py:43-44)."""
    try:
        _lib.lib()
    except (ImportError, OSError, AttributeError):
        return False
    return torch.cuda.is_available()
