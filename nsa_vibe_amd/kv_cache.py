"""NSA_KV with preallocated storage.

Same field names and layouts as the reference cache (nsa/cache/kv_cache.py:8-26: K_sel/V_sel/K_win/V_win/
K_cmp_raw_seq/V_cmp_raw_seq [B,G,S,D], K_cmp/V_cmp [B,G,S_cmp,D], meta, read counters) -- but the tensors are
views into buffers allocated once for `S_max` tokens, so appending a decode token is a row write instead of the
reference's O(S) `torch.cat` copy per step (kv_cache.py:28-30).  The selection kernels take the element strides
of these views through the C ABI, so nothing is ever re-packed.
"""
from __future__ import annotations

import ctypes
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


PAGE_TOKENS, PAGE_CMP = 1024, 64  # a page: 1024 tokens of the six token caches, 64 rows of K_cmp / V_cmp (d = 16)
CLOSE_LAG = 16  # d: compressed row 64 j + 63, the last of page j, is pooled from raw rows up to 1024 (j + 1) + 15
_POOLS = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp")


class NSA_PagedKV:
    """The eight caches of NSA_KV as POOLS of pages behind a block table (include/nsa_sel_hip.h: nsa_paged_kv_desc): six token pools
    [n_pages, G, 1024, D], K_cmp / V_cmp [n_pages, G, 64, D], a device int32 block_table [B, max_pages] (-1 = no page), a host free
    list and one reference count per page.  One page id serves all eight pools: entry [b, j] holds tokens [1024 j, 1024 j + 1024) and
    compressed rows [64 j, 64 j + 64) of the sequence in slot b.  What NSAAttention.decode_paged (nsa_layer_decode_paged) appends to and
    reads; the lengths of the sequences belong to the caller.
    Sharing.  ensure() hands a page to one slot (count 1).  fork() lets a second slot name the pages of a common prefix, but only the
    CLOSED ones: page j of a sequence of t tokens is closed once t >= 1024 (j + 1) + 16, i.e. n_cmp(t) >= 64 (j + 1) -- until then its
    compressed row 64 j + 63 (pooled from raw rows 1024 j + 1008 .. 1024 j + 1039) is still to be written, and two sequences that diverge
    inside [1024 (j + 1), 1024 (j + 1) + 16) would both write it.  Every page an append can still write is private to its slot:
    own_tail() replaces a shared one by a copy (one nsa_paged_kv_copy_pages launch; torch indexing on CPU tensors), fork(), truncate() and
    load_sequence() call it.  free() returns a page to the free list when its count reaches zero.
    The default block geometry only (l = 32, d = 16, l_sel = 64): the page sizes follow from it."""

    def __init__(self, n_pages: int, B: int, max_pages: int, G: int, d_k: int, d_v: int, l: int, d: int, l_sel: int, n_sel: int, w: int,
                 device, dtype):
        if (l, d, l_sel) != (32, 16, 64):
            raise ValueError(f"NSA_PagedKV: pages of {PAGE_TOKENS} tokens / {PAGE_CMP} compressed rows need the default block geometry "
                             f"(l = 32, d = 16, l_sel = 64), got ({l}, {d}, {l_sel})")
        if n_pages < 1 or B < 1 or max_pages < 1:
            raise ValueError(f"NSA_PagedKV: n_pages = {n_pages}, B = {B}, max_pages = {max_pages} must all be positive")
        self.n_pages, self.B, self.max_pages, self.G, self.d_k, self.d_v = n_pages, B, max_pages, G, d_k, d_v
        self.l, self.d, self.l_sel, self.n_sel, self.w = l, d, l_sel, n_sel, w
        mk = lambda rows, dim: torch.empty((n_pages, G, rows, dim), device=device, dtype=dtype)  # noqa: E731
        self._K_sel, self._V_sel = mk(PAGE_TOKENS, d_k), mk(PAGE_TOKENS, d_v)
        self._K_win, self._V_win = mk(PAGE_TOKENS, d_k), mk(PAGE_TOKENS, d_v)
        self._K_raw, self._V_raw = mk(PAGE_TOKENS, d_k), mk(PAGE_TOKENS, d_v)
        self._K_cmp, self._V_cmp = mk(PAGE_CMP, d_k), mk(PAGE_CMP, d_v)
        self.block_table = torch.full((B, max_pages), -1, dtype=torch.int32, device=device)
        self.pages: List[List[int]] = [[] for _ in range(B)]  # host mirror of the table rows
        self._free: List[int] = list(range(n_pages - 1, -1, -1))  # (a stack: page 0 goes out first)
        self._refs: List[int] = [0] * n_pages  # table entries that name the page; 0: on the free list
        self.meta: BlockMeta = build_block_meta(0, l, d, l_sel, n_sel, w)
        self.meta_seq_len = 0
        self._native: dict = {}

    # the block metadata is NSA_KV's (immutable, shared through the process-wide cache)
    ensure_meta = NSA_KV.ensure_meta
    refresh_meta = NSA_KV.refresh_meta

    @property
    def capacity(self) -> int:
        """tokens a sequence can hold: what stands for S_max"""
        return self.max_pages * PAGE_TOKENS

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def _slot(self, b: int) -> int:
        b = int(b)
        if not 0 <= b < self.B:
            raise IndexError(f"NSA_PagedKV: slot {b} outside [0, {self.B})")
        return b

    def page_refs(self, b: int) -> List[int]:
        """the reference counts of slot b's pages, in table order (1: the slot's own)"""
        return [self._refs[p] for p in self.pages[self._slot(b)]]

    def shared_pages(self, b: int) -> List[int]:
        """the pages of slot b that another table entry names too (count > 1): read-only for every holder"""
        return [p for p in self.pages[self._slot(b)] if self._refs[p] > 1]

    def _set_entries(self, b: int, j0: int, ids: List[int]) -> None:
        self.block_table[b, j0:j0 + len(ids)] = torch.tensor(ids, dtype=torch.int32).to(self.block_table.device)

    def _release(self, ids) -> None:
        """one reference less on each page, in this order; a page whose count reaches zero goes back to the free list"""
        for p in ids:
            self._refs[p] -= 1
            if self._refs[p] == 0:
                self._free.append(p)

    def ensure(self, b: int, n_tokens: int) -> None:
        """pages for slot b until they cover n_tokens (idempotent: pages it holds stay where they are); raises when n_tokens exceed the
        capacity or the pool is exhausted -- then nothing is assigned"""
        b, n_tokens = self._slot(b), int(n_tokens)
        need = (n_tokens + PAGE_TOKENS - 1) // PAGE_TOKENS
        if n_tokens < 0 or need > self.max_pages:
            raise RuntimeError(f"NSA_PagedKV.ensure: {n_tokens} tokens outside the capacity {self.capacity} of a slot (max_pages = {self.max_pages})")
        have = len(self.pages[b])
        if need <= have:
            return
        if need - have > len(self._free):
            raise RuntimeError(f"NSA_PagedKV.ensure: pool exhausted -- slot {b} needs {need - have} more pages, {len(self._free)} of {self.n_pages} are free")
        new = [self._free.pop() for _ in range(need - have)]
        for p in new:
            self._refs[p] = 1
        self.pages[b].extend(new)
        self._set_entries(b, have, new)

    def free(self, b: int) -> None:
        """slot b gives up its pages (each back to the free list once no other slot names it), its table entries go back to -1"""
        b = self._slot(b)
        self._release(reversed(self.pages[b]))
        self.pages[b] = []
        self.block_table[b].fill_(-1)

    # ---- sharing: closed pages by reference, every other page private ----------------------------------------------------------------------
    @staticmethod
    def page_closed(j: int, t: int) -> bool:
        """whether page j of a sequence of t tokens is closed: no append at a position >= t writes it (its 64 compressed rows are emitted)"""
        return t >= PAGE_TOKENS * (j + 1) + CLOSE_LAG

    def _open_pages(self, b: int, t: int) -> List[int]:
        """the table positions j <= t >> 10 of slot b's pages that are not closed at t: the last one, and the one before it while
        t & 1023 < 16 (t >= 1024)"""
        return [j for j in range(max(0, (t >> 10) - 1), min(len(self.pages[b]), (t >> 10) + 1)) if not self.page_closed(j, t)]

    def _copy_pages(self, jobs: List[tuple]) -> None:
        """jobs of (src page, dst page, token rows, compressed rows), all in one nsa_paged_kv_copy_pages launch (torch indexing on CPU)"""
        jobs = [jb for jb in jobs if jb[2] > 0 or jb[3] > 0]
        if not jobs:
            return
        dev = self._K_sel.device
        if dev.type == "cuda":
            from ._native import _stream

            with torch.cuda.device(dev):
                dj = torch.tensor(jobs, dtype=torch.int32).to(dev)
                _lib.check(_lib.lib().nsa_paged_kv_copy_pages(ctypes.byref(self.native_desc()), dj.data_ptr(), len(jobs), self.G, self.d_k, self.d_v,
                                                              self._dtype_code(), _stream(dev)), "nsa_paged_kv_copy_pages")
            return
        for src, dst, n_tok, n_cmp in jobs:
            for name in _POOLS:
                k = n_cmp if name in ("_K_cmp", "_V_cmp") else n_tok
                if k:
                    pool = getattr(self, name)
                    pool[dst, :, :k] = pool[src, :, :k]

    def _dtype_code(self) -> int:
        from ._native import _DT

        code = _DT.get(self._K_sel.dtype)
        if code is None:
            raise RuntimeError(f"NSA_PagedKV: the native page copies take bf16 / f16 pools, not {self._K_sel.dtype}")
        return code

    def own_tail(self, b: int, t: int) -> None:
        """every page of slot b that an append at a position >= t can write becomes the slot's own: a page j <= t >> 10 that is not closed
        at t and has count > 1 is replaced by a fresh page holding its token rows [0, min(1024, t - 1024 j)) and compressed rows
        [0, min(64, n_cmp(t) - 64 j)) (at most two pages, one copy launch); the old page loses a reference.  Raises when the pool cannot
        supply the pages -- then nothing changes."""
        b, t = self._slot(b), int(t)
        if t < 0:
            raise ValueError(f"NSA_PagedKV.own_tail: t = {t} is negative")
        todo = [j for j in self._open_pages(b, t) if self._refs[self.pages[b][j]] > 1]
        if not todo:
            return
        if len(todo) > len(self._free):
            raise RuntimeError(f"NSA_PagedKV.own_tail: pool exhausted -- slot {b} needs {len(todo)} private pages, {len(self._free)} of {self.n_pages} are free")
        n_cmp, jobs = n_cmp_at(t, self.l, self.d), []
        for j in todo:
            old, new = self.pages[b][j], self._free.pop()
            self._refs[new] = 1
            self._refs[old] -= 1  # (stays >= 1: another entry names it)
            self.pages[b][j] = new
            self._set_entries(b, j, [new])
            jobs.append((old, new, max(0, min(PAGE_TOKENS, t - PAGE_TOKENS * j)), max(0, min(PAGE_CMP, n_cmp - PAGE_CMP * j))))
        self._copy_pages(jobs)

    def fork(self, src: int, dst: int, t: int) -> None:
        """slot dst (empty) becomes a sequence of the first t tokens of slot src, 0 <= t <= the tokens src's pages cover: the pages closed
        at t are SHARED (the same table entry, one more reference), the others that hold one of the t tokens -- the last, and the one
        before it while t & 1023 < 16 -- are private copies (own_tail).  src is not modified and may go on decoding on the pages it owns
        alone (own_tail(src, .) first where its open pages are shared from an earlier fork).  Raises when the pool cannot supply the
        private pages -- then nothing is assigned and no count changes."""
        src, dst, t = self._slot(src), self._slot(dst), int(t)
        if src == dst:
            raise RuntimeError(f"NSA_PagedKV.fork: src and dst are both slot {src}")
        if self.pages[dst]:
            raise RuntimeError(f"NSA_PagedKV.fork: slot {dst} is not empty (free it first)")
        if not 0 <= t <= len(self.pages[src]) * PAGE_TOKENS:
            raise ValueError(f"NSA_PagedKV.fork: t = {t} outside the {len(self.pages[src])} pages of slot {src}")
        need = (t + PAGE_TOKENS - 1) // PAGE_TOKENS
        private = sum(1 for j in range(need) if not self.page_closed(j, t))
        if private > len(self._free):
            raise RuntimeError(f"NSA_PagedKV.fork: pool exhausted -- slot {dst} needs {private} private pages, {len(self._free)} of {self.n_pages} are free")
        ids = self.pages[src][:need]
        for p in ids:
            self._refs[p] += 1
        self.pages[dst] = list(ids)
        if ids:
            self._set_entries(dst, 0, ids)
        self.own_tail(dst, t)

    def truncate(self, b: int, t: int) -> None:
        """the page bookkeeping of a rollback of slot b to t tokens (the length itself is the caller's): the pages above the one that holds
        token t - 1 are released and their table entries set to -1, then own_tail(b, t) makes the next append's pages private.  t = 0 is
        free(b).  Raises when own_tail cannot be supplied -- then nothing changes."""
        b, t = self._slot(b), int(t)
        if not 0 <= t <= len(self.pages[b]) * PAGE_TOKENS:
            raise ValueError(f"NSA_PagedKV.truncate: t = {t} outside the {len(self.pages[b])} pages of slot {b}")
        if t == 0:
            return self.free(b)
        keep = (t + PAGE_TOKENS - 1) // PAGE_TOKENS
        gone = self.pages[b][keep:]
        private = sum(1 for j in self._open_pages(b, t) if j < keep and self._refs[self.pages[b][j]] > 1)
        if private > len(self._free) + sum(1 for p in gone if self._refs[p] == 1):
            raise RuntimeError(f"NSA_PagedKV.truncate: pool exhausted -- slot {b} needs {private} private pages")
        if gone:
            self._release(reversed(gone))
            del self.pages[b][keep:]
            self.block_table[b, keep:].fill_(-1)
        self.own_tail(b, t)

    # ---- copies between a contiguous B = 1 cache and a slot's pages ------------------------------------------------------------------------
    def _copy_rows(self, b: int, kv1: "NSA_KV", t0: int, t: int, to_pages: bool) -> None:
        """token rows [t0, t) and compressed rows [n_cmp(t0), n_cmp(t)) between kv1 and slot b's pages: one nsa_paged_kv_store / _load
        launch on HIP device tensors, torch indexing on CPU tensors"""
        if t0 == t:
            return
        dev = self._K_sel.device
        if dev.type == "cuda":
            from ._native import _stream

            fn = _lib.lib().nsa_paged_kv_store if to_pages else _lib.lib().nsa_paged_kv_load
            with torch.cuda.device(dev):
                _lib.check(fn(ctypes.byref(self.native_desc()), ctypes.byref(kv1.native_desc()), 0, b, t0, t, self.G, self.d_k, self.d_v, self._dtype_code(),
                              _stream(dev)), "nsa_paged_kv_store" if to_pages else "nsa_paged_kv_load")
            return
        for name in _POOLS:
            rows, lo, hi = (PAGE_CMP, n_cmp_at(t0, self.l, self.d), n_cmp_at(t, self.l, self.d)) if name in ("_K_cmp", "_V_cmp") else (PAGE_TOKENS, t0, t)
            pool, slab = getattr(self, name), getattr(kv1, name)
            for j in range(lo // rows, (hi + rows - 1) // rows):
                r0, r1 = max(lo, j * rows), min(hi, (j + 1) * rows)
                if r1 <= r0:
                    continue
                if to_pages:
                    pool[self.pages[b][j], :, r0 - j * rows:r1 - j * rows] = slab[0, :, r0:r1]
                else:
                    slab[0, :, r0:r1] = pool[self.pages[b][j], :, r0 - j * rows:r1 - j * rows]

    def _check_kv1(self, who: str, kv1: "NSA_KV") -> None:
        if kv1.B != 1 or (kv1.G, kv1.d_k, kv1.d_v) != (self.G, self.d_k, self.d_v) or kv1._K_sel.dtype != self._K_sel.dtype:
            raise RuntimeError(f"NSA_PagedKV.{who}: a B = 1 NSA_KV of the pool's geometry and dtype is needed")
        if kv1._K_sel.device != self._K_sel.device:
            raise RuntimeError(f"NSA_PagedKV.{who}: the NSA_KV is on {kv1._K_sel.device}, the pools on {self._K_sel.device}")

    def load_sequence(self, b: int, kv1: "NSA_KV", t: int, t0: int = 0) -> None:
        """token rows [t0, t) and compressed rows [n_cmp(t0), n_cmp(t)) of a B = 1 NSA_KV into slot b's pages (assigned here as needed; the
        pages these rows fall into are made private first, own_tail(b, t0)): how a prefilled sequence, or the suffix a forked slot was
        extended by, enters the pool.  One nsa_paged_kv_store launch on HIP device tensors, torch indexing on CPU tensors."""
        b, t, t0 = self._slot(b), int(t), int(t0)
        self._check_kv1("load_sequence", kv1)
        if not 0 <= t <= kv1._K_sel.shape[2]:
            raise ValueError(f"NSA_PagedKV.load_sequence: t = {t} outside [0, {kv1._K_sel.shape[2]}]")
        if not 0 <= t0 <= t:
            raise ValueError(f"NSA_PagedKV.load_sequence: t0 = {t0} outside [0, t = {t}]")
        for j in range((t0 >> 10) + 1, len(self.pages[b])):  # (own_tail looks after the pages up to t0 >> 10)
            if self._refs[self.pages[b][j]] > 1:
                raise RuntimeError(f"NSA_PagedKV.load_sequence: page {j} of slot {b}, above row t0 = {t0}, is shared: truncate(b, t0) first")
        self.own_tail(b, t0)
        self.ensure(b, t)
        self._copy_rows(b, kv1, t0, t, True)

    def gather_sequence(self, b: int, t: int, t0: int = 0) -> "NSA_KV":
        """the reverse: a B = 1 NSA_KV (capacity: the slot's assigned pages, at least one) of t tokens and n_cmp(t) compressed rows holding
        token rows [t0, t) and compressed rows [n_cmp(t0), n_cmp(t)) of slot b.  Every other row is zero.  One nsa_paged_kv_load launch on
        HIP device tensors, torch indexing on CPU tensors."""
        b, t, t0 = self._slot(b), int(t), int(t0)
        if not 0 <= t <= len(self.pages[b]) * PAGE_TOKENS:
            raise ValueError(f"NSA_PagedKV.gather_sequence: t = {t} outside the {len(self.pages[b])} pages of slot {b}")
        if not 0 <= t0 <= t:
            raise ValueError(f"NSA_PagedKV.gather_sequence: t0 = {t0} outside [0, t = {t}]")
        cap = max(1, len(self.pages[b])) * PAGE_TOKENS
        kv1 = NSA_KV(1, self.G, self.d_k, self.d_v, cap, self.l, self.d, self.l_sel, self.n_sel, self.w, self._K_sel.device, self._K_sel.dtype,
                     auto_grow=False)
        for name in _POOLS:
            getattr(kv1, name).zero_()
        self._copy_rows(b, kv1, t0, t, False)
        kv1.t, kv1.n_cmp = t, n_cmp_at(t, self.l, self.d)
        return kv1

    def native_desc(self):
        """struct nsa_paged_kv_desc of the pools and the table (include/nsa_sel_hip.h), built once"""
        d = self._native.get("desc")
        if d is None:
            d = self._native["desc"] = _lib.NsaPagedKvDesc()
            for name in _POOLS:
                setattr(d, name[1:], getattr(self, name).data_ptr())
            d.block_table, d.table_stride = self.block_table.data_ptr(), self.block_table.stride(0)
            d.n_pages, d.B, d.max_pages = self.n_pages, self.B, self.max_pages
        return d
