"""Host idioms of the calls into the C ABI (include/nsa_sel_hip.h), shared by every module of the package: dtype codes, device and stream,
the workspace pool, and the argument runs that recur in the signatures."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from . import _lib

_DT = {torch.float32: _lib.NSA_DT_F32, torch.bfloat16: _lib.NSA_DT_BF16, torch.float16: _lib.NSA_DT_F16}
_WS: Dict[tuple, torch.Tensor] = {}


def _need_gpu(*ts: torch.Tensor) -> torch.device:
    dev = ts[0].device
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("nsa_vibe_amd kernels need HIP device tensors (no CPU fallback exists)")
        if t.device != dev:
            raise RuntimeError("all tensors must be on the same device")
    return dev


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev: torch.device) -> int:
    """raw handle of torch's current stream on dev (a decode step makes this call once per layer: the Stream object of
    torch.cuda.current_stream costs tens of microseconds of host time, the raw getter about one)"""
    if _raw_stream is not None:
        idx = dev.index if isinstance(dev, torch.device) else None
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(dev).cuda_stream


def workspace(dev: torch.device, nbytes: int, tag: str = "ws") -> Optional[torch.Tensor]:
    """Grow-on-demand scratch per (device, stream) (the reference keeps process-global workspaces too,
    nsa/core/attention_kernels.py:25-26,64-103; keyed by stream here so concurrent streams cannot race on it)."""
    if nbytes <= 0:
        return None
    key = (tag, dev.index, _stream(dev))  # per stream: two streams never share scratch
    buf = _WS.get(key)
    # grown on demand; given back when a much smaller shape follows a big one (the key-split records of a 64k prefill are gigabytes)
    if buf is None or buf.numel() < nbytes or buf.numel() > max(4 * nbytes, 256 << 20):
        _WS.pop(key, None)
        buf = None
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _WS[key] = buf
    return buf


def workspace_at(dev: torch.device, nbytes: int, tag: str, align: int):
    """workspace() of nbytes from an `align`-byte boundary on -> (pointer, bytes behind it, the buffer)"""
    ws = workspace(dev, nbytes + align, tag)
    ptr = (ws.data_ptr() + align - 1) & ~(align - 1)
    return ptr, ws.numel() - (ptr - ws.data_ptr()), ws


def _ws_args(ws: Optional[torch.Tensor]):
    """(pointer, bytes) of an optional workspace as the C ABI takes them"""
    return (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)


def _scale_arg(scale: Optional[float]) -> float:
    """the C ABI's scale: 0 asks for 1/sqrt(Dk)"""
    return float(scale) if scale else 0.0


def _unit_rows(X: torch.Tensor):
    """a [B,G,S,D] cache view as the C ABI takes it -> (X with unit last stride: itself, or a copy; its batch, group and row strides)"""
    if X.stride(-1) != 1:
        X = X.contiguous()
    return X, X.stride(0), X.stride(1), X.stride(2)


def _sel_mode(mode: str, S_sel: int, l_sel: int, n_top: int, S: int, force_init=True, force_local: int = 2):
    """selector name -> (NSA_SEL_* code, width of its ranges: n_top, or what nsa_batched_ranges_width answers for the batched converter)"""
    if mode == "batched":
        return _lib.NSA_SEL_BATCHED, int(_lib.lib().nsa_batched_ranges_width(int(S), int(S_sel), int(l_sel), int(n_top), int(bool(force_init)),
                                                                             int(force_local)))
    if mode == "sequential":
        return _lib.NSA_SEL_SEQUENTIAL, n_top
    raise ValueError("mode must be 'batched' or 'sequential'")


def _plan_ints(name: str, n_out: int, *args):
    """a *_plan entry point (no device work): `args`, then n_out int results by reference -> their values"""
    outs = [ctypes.c_int(0) for _ in range(n_out)]
    _lib.check(getattr(_lib.lib(), name)(*args, *[ctypes.byref(o) for o in outs]), name)
    return [o.value for o in outs]


def _needs_grad(*ts) -> bool:
    """whether autograd has to see this call: recording is on and one of the tensors asks for a gradient"""
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)
