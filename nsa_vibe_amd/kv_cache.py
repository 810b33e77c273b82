"""NSA_KV with preallocated storage.

Same field names and layouts as the reference cache (nsa/cache/kv_cache.py:8-26: K_sel/V_sel/K_win/V_win/
K_cmp_raw_seq/V_cmp_raw_seq [B,G,S,D], K_cmp/V_cmp [B,G,S_cmp,D], meta, read counters) -- but the tensors are
views into buffers allocated once for `S_max` tokens, so appending a decode token is a row write instead of the
reference's O(S) `torch.cat` copy per step (kv_cache.py:28-30).  The selection kernels take the element strides
of these views through the C ABI, so nothing is ever re-packed.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _lib
from .block_index import BlockMeta, build_block_meta


_META_CACHE: dict = {}


def n_cmp_at(n_tokens: int, l: int, d: int) -> int:
    """compressed tokens emitted once n_tokens are cached (the emission schedule of the reference, nsa_attention.py:588-604)"""
    return 0 if n_tokens < l else (n_tokens - l) // d + 1


class NSA_KV:
    def __init__(self, B: int, G: int, d_k: int, d_v: int, S_max: int, l: int, d: int, l_sel: int, n_sel: int, w: int,
                 device, dtype, auto_grow: bool = True):
        self.B, self.G, self.d_k, self.d_v, self.S_max = B, G, d_k, d_v, S_max
        self.auto_grow = auto_grow
        self.l, self.d, self.l_sel, self.n_sel, self.w = l, d, l_sel, n_sel, w
        n_cmp_max = n_cmp_at(S_max, l, d)
        mk = lambda n, dim: torch.empty((B, G, max(n, 1), dim), device=device, dtype=dtype)  # noqa: E731
        self._K_sel, self._V_sel = mk(S_max, d_k), mk(S_max, d_v)
        self._K_win, self._V_win = mk(S_max, d_k), mk(S_max, d_v)
        self._K_raw, self._V_raw = mk(S_max, d_k), mk(S_max, d_v)
        self._K_cmp, self._V_cmp = mk(n_cmp_max, d_k), mk(n_cmp_max, d_v)
        self.t = 0  # tokens stored
        self.n_cmp = 0  # compressed tokens emitted
        self.meta: BlockMeta = build_block_meta(0, l, d, l_sel, n_sel, w)
        self.meta_seq_len = 0
        # decode read counters (reference: kv_cache.py:22-26,51-65) kept on the host: no device sync per step
        self.reads_pred: List[int] = []
        self.reads_act_total: List[int] = []
        self.reads_act_sel: List[int] = []
        self.reads_act_cmp: List[int] = []
        self.reads_act_win: List[int] = []
        # what the native routes keep per cache: "desc" (native_desc) and the context of each single-step route under its workspace tag;
        # all of it names the buffers, so reserve() empties it
        self._native: dict = {}

    def __copy__(self):
        """a shallow copy shares the buffers until its holder replaces them (a test's clone does): it must not share _native, whose
        descriptor and step contexts carry the addresses of the original's buffers"""
        c = object.__new__(type(self))
        c.__dict__.update(self.__dict__)
        c._native = {}
        return c

    def sequence_view(self, b: int, t: int = 0) -> "NSA_KV":
        """slab b of these buffers as a cache of its own: a B = 1 NSA_KV that SHARES the storage (a write through the view lands in the
        pool) and holds t tokens, n_cmp_at(t) compressed ones and empty read counters.  It has its own native descriptor and does not
        grow (auto_grow = False: growing would detach it from the pool).  What NSAAttention.decode_ragged's pool of slabs is filled
        through -- m(x_b, kv.sequence_view(b), prefill=True) -- and what its per-sequence route runs on."""
        b, t = int(b), int(t)
        if not 0 <= b < self.B:
            raise IndexError(f"NSA_KV.sequence_view: sequence {b} outside [0, {self.B})")
        cap = self._K_sel.shape[2]
        if not 0 <= t <= cap:
            raise ValueError(f"NSA_KV.sequence_view: t = {t} outside [0, {cap}]")
        v = object.__new__(type(self))
        v.__dict__.update(self.__dict__)
        v.B, v.auto_grow, v.S_max = 1, False, cap
        for name in ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp"):
            setattr(v, name, getattr(self, name)[b:b + 1])  # (a leading-axis slice: contiguous, the same memory)
        v.t, v.n_cmp = t, self.n_cmp_at(t)
        v.meta, v.meta_seq_len = build_block_meta(0, self.l, self.d, self.l_sel, self.n_sel, self.w), 0
        v.reads_pred, v.reads_act_total, v.reads_act_sel, v.reads_act_cmp, v.reads_act_win = [], [], [], [], []
        v._native = {}
        return v

    # ---- reference field names as views -------------------------------------------------
    @property
    def K_sel(self):
        return self._K_sel[:, :, : self.t]

    @property
    def V_sel(self):
        return self._V_sel[:, :, : self.t]

    @property
    def K_win(self):  # the reference keeps only the last w tokens; the window is applied by the reader here
        return self._K_win[:, :, max(0, self.t - self.w): self.t]

    @property
    def V_win(self):
        return self._V_win[:, :, max(0, self.t - self.w): self.t]

    @property
    def K_cmp_raw_seq(self):
        return self._K_raw[:, :, : self.t]

    @property
    def V_cmp_raw_seq(self):
        return self._V_raw[:, :, : self.t]

    @property
    def K_cmp(self):
        return self._K_cmp[:, :, : self.n_cmp]

    @property
    def V_cmp(self):
        return self._V_cmp[:, :, : self.n_cmp]

    # ---- capacity -------------------------------------------------------------------------
    def reserve(self, S_max: int) -> None:
        """grow the buffers to hold S_max tokens, keeping what is stored (the one O(S) copy the reference pays on every step,
        kv_cache.py:28-30, paid here once per doubling).  Cached native descriptors of the old buffers are dropped."""
        if S_max <= self._K_sel.shape[2]:
            return
        n_cmp_max = self.n_cmp_at(S_max)

        def grow(buf, n, used):
            new = torch.empty((self.B, self.G, max(n, 1), buf.shape[3]), device=buf.device, dtype=buf.dtype)
            if used:
                new[:, :, :used] = buf[:, :, :used]
            return new

        for name in ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw"):
            setattr(self, name, grow(getattr(self, name), S_max, self.t))
        self._K_cmp, self._V_cmp = grow(self._K_cmp, n_cmp_max, self.n_cmp), grow(self._V_cmp, n_cmp_max, self.n_cmp)
        self.S_max = S_max
        self._native.clear()

    def ensure_capacity(self, n_tokens: int) -> None:
        """room for n_tokens in total: grows geometrically (auto_grow) or raises"""
        cap = self._K_sel.shape[2]
        if n_tokens <= cap:
            return
        if not self.auto_grow:
            raise RuntimeError(f"NSA_KV capacity exceeded: {n_tokens} > S_max={self.S_max}")
        self.reserve(max(n_tokens, 2 * cap))

    # ---- updates --------------------------------------------------------------------------
    def write_tokens(self, K_sel, V_sel, K_win, V_win, K_raw, V_raw) -> None:
        """append S new tokens ([B,G,S,D] each) at position t (update_selection_raw/update_window/append_cmp_raw)."""
        S = K_sel.shape[2]
        self.ensure_capacity(self.t + S)
        sl = slice(self.t, self.t + S)
        self._K_sel[:, :, sl], self._V_sel[:, :, sl] = K_sel, V_sel
        self._K_win[:, :, sl], self._V_win[:, :, sl] = K_win, V_win
        self._K_raw[:, :, sl], self._V_raw[:, :, sl] = K_raw, V_raw
        self.t += S

    def write_compressed(self, K_cmp, V_cmp, at: Optional[int] = None) -> None:
        n = K_cmp.shape[2]
        at = self.n_cmp if at is None else at
        self._K_cmp[:, :, at: at + n], self._V_cmp[:, :, at: at + n] = K_cmp, V_cmp
        self.n_cmp = at + n

    def ensure_meta(self, seq_len: int) -> BlockMeta:
        """block metadata for seq_len tokens; metadata objects are immutable and shared through a small process-wide cache
        (the host build + the upload of the Eq.9 map cost ~0.15 ms, as much as a 4k prefill's attention kernel)"""
        key = (seq_len, self.l, self.d, self.l_sel, self.n_sel, self.w)
        meta = _META_CACHE.get(key)
        if meta is None:
            if len(_META_CACHE) >= 256:
                _META_CACHE.pop(next(iter(_META_CACHE)))
            meta = _META_CACHE[key] = build_block_meta(seq_len, self.l, self.d, self.l_sel, self.n_sel, self.w)
        self.meta = meta
        self.meta_seq_len = seq_len
        return self.meta

    def truncate(self, t: int) -> None:
        """forget every token from position t on (0 <= t <= self.t): what a speculative decoder calls after rejecting draft tokens.
        Sets t and n_cmp = n_cmp(t) and drops the read counters of the forgotten tokens: the last self.t - t entries of the five reads_*
        lists, which leaves t entries where every token was decoded (a prefill appends none, so a list may be shorter than t and then only
        loses what the decode steps behind the prefill added).  The buffers are left as they are: the next append overwrites row t, and
        the emission schedule overwrites compressed row n_cmp when its window completes again."""
        t = int(t)
        if t < 0 or t > self.t:
            raise ValueError(f"NSA_KV.truncate: t = {t} outside [0, {self.t}]")
        drop = self.t - t
        self.t = t
        self.n_cmp = self.n_cmp_at(t)
        for lst in (self.reads_pred, self.reads_act_total, self.reads_act_sel, self.reads_act_cmp, self.reads_act_win):
            del lst[max(0, len(lst) - drop):]

    def append_reads(self, num_cmp: int, S_raw: int) -> None:
        sel, win = self.n_sel * self.l_sel, min(self.w, S_raw)
        total = num_cmp + sel + win  # the reads formula of nsa_attention.py:634-635
        self.reads_pred.append(total)
        self.reads_act_total.append(total)
        self.reads_act_sel.append(sel)
        self.reads_act_cmp.append(num_cmp)
        self.reads_act_win.append(win)

    # ---- bookkeeping of the rows a native call appends ------------------------------------------------------------------------------------
    def n_cmp_at(self, n_tokens: int) -> int:
        return n_cmp_at(n_tokens, self.l, self.d)

    def refresh_meta(self, upto: int) -> None:
        """block metadata refresh policy of the reference (:606-632): rebuilt only when the first `upto` tokens leave the covered blocks"""
        if self.meta.S_sel == 0:
            self.ensure_meta(max(upto, self.l_sel))
        elif upto > self.meta.S_sel * self.l_sel:
            self.ensure_meta(upto)

    def begin_rows(self, S: int):
        """before S tokens are appended at t: capacity, and the block metadata by the decode step's policy -> (t, meta)"""
        t0 = self.t
        self.ensure_capacity(t0 + S)
        self.refresh_meta(t0 + S)
        return t0, self.meta

    def end_rows(self, t0: int, S: int) -> None:
        """after the S tokens t0 .. t0 + S - 1 were appended: token count, compressed count and read counters as S decode steps leave them"""
        for n in range(t0 + 1, t0 + S + 1):
            self.append_reads(self.n_cmp_at(n), n)
        self.t, self.n_cmp = t0 + S, self.n_cmp_at(t0 + S)

    def snapshot(self):
        """what restore() needs to forget the rows appended after this point"""
        return self.t, self.n_cmp, len(self.reads_pred)

    def restore(self, saved) -> None:
        """back to a snapshot(): the rows a failed call appended are written again by the next executor"""
        self.t, self.n_cmp = saved[0], saved[1]
        for lst in (self.reads_pred, self.reads_act_total, self.reads_act_sel, self.reads_act_cmp, self.reads_act_win):
            del lst[saved[2]:]

    def native_desc(self):
        """struct nsa_kv_desc of the buffers (include/nsa_sel_hip.h), built once per set of buffers"""
        d = self._native.get("desc")
        if d is None:
            d = self._native["desc"] = _lib.NsaKvDesc()
            d.K_sel, d.V_sel, d.K_win, d.V_win = self._K_sel.data_ptr(), self._V_sel.data_ptr(), self._K_win.data_ptr(), self._V_win.data_ptr()
            d.K_raw, d.V_raw, d.K_cmp, d.V_cmp = self._K_raw.data_ptr(), self._V_raw.data_ptr(), self._K_cmp.data_ptr(), self._V_cmp.data_ptr()
            d.B, d.S_max, d.n_cmp_max = self.B, self._K_sel.shape[2], self._K_cmp.shape[2]
        return d
