"""GPU: the native page copies -- nsa_paged_kv_store / nsa_paged_kv_load / nsa_paged_kv_copy_pages (include/nsa_sel_hip.h), called through
the C ABI so that the table and the jobs can hold anything.

Reference: torch indexing on a clone, page by page, as NSA_PagedKV.load_sequence did before the native calls existed (`indexed_store`).
Pools and slabs are poisoned with +-3e4 and every comparison is on bit patterns (int16 views) over EVERY byte of every pool and slab: the
rows a call must write, and the poison everywhere it must not.  G = 2, n_pages = 7, max_pages = 3, a permuted table; slot 1 of 2, slab 1
of 2, so that a call that ignores either index fails."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

POOLS = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp")
G, N_PAGES, MAX_PAGES, S_MAX = 2, 7, 3, 3072
TABLE = [[3, -1, -1], [5, 2, 6]]
SLOT, B_SRC = 1, 1
RANGES = [(0, t) for t in (0, 1, 31, 32, 1023, 1024, 1039, 1040, 1500, 2049)] + [(1000, 1040), (1024, 1030), (1500, 2049)]
CONFIGS = [(64, torch.bfloat16), (128, torch.bfloat16), (64, torch.float16), (128, torch.float16)]
IDS = ["d64-bf16", "d128-bf16", "d64-f16", "d128-f16"]


def ncmp(t):
    return 0 if t < 32 else (t - 32) // 16 + 1


def bits(x):
    return x.contiguous().view(torch.int16)


def poison(t):
    n = t.numel()
    v = torch.where(torch.arange(n, device=t.device) % 2 == 0, 3e4, -3e4)
    t.copy_(v.to(t.dtype).view_as(t))


def make(D, dtype, table=TABLE, seed=0):
    """poisoned pools behind `table`, and a two-slab NSA_KV of random rows"""
    from nsa_vibe_amd.kv_cache import NSA_KV, NSA_PagedKV

    pkv = NSA_PagedKV(N_PAGES, 2, MAX_PAGES, G, D, D, 32, 16, 64, 16, 512, "cuda", dtype)
    kv = NSA_KV(2, G, D, D, S_MAX, 32, 16, 64, 16, 512, "cuda", dtype, auto_grow=False)
    g = torch.Generator(device="cuda").manual_seed(seed)
    for name in POOLS:
        poison(getattr(pkv, name))
        buf = getattr(kv, name)
        buf.copy_(torch.randn(buf.shape, generator=g, device="cuda").to(dtype))
    pkv.block_table.copy_(torch.tensor(table, dtype=torch.int32))
    torch.cuda.synchronize()
    return pkv, kv


def snapshot(obj):
    return {n: getattr(obj, n).clone() for n in POOLS}


def same(obj, snap):
    return [n for n in POOLS if not torch.equal(bits(getattr(obj, n)), bits(snap[n]))]


def call(name, pkv, kv, t0, t1, b_src=B_SRC, slot=SLOT, G_=G, Dk=None, Dv=None, dtype=None, pd=None, kd=None):
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd._native import _DT, _stream

    dev = pkv._K_sel.device
    pd, kd = pd or pkv.native_desc(), kd or kv.native_desc()
    rc = getattr(_lib.lib(), name)(ctypes.byref(pd), ctypes.byref(kd), b_src, slot, t0, t1, G_, pkv.d_k if Dk is None else Dk,
                                  pkv.d_v if Dv is None else Dv, _DT[pkv._K_sel.dtype] if dtype is None else dtype, _stream(dev))
    torch.cuda.synchronize()
    return rc


def copy_pages(pkv, jobs, n_jobs=None, **kw):
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd._native import _DT, _stream

    dev = pkv._K_sel.device
    dj = torch.tensor(jobs, dtype=torch.int32, device=dev).reshape(-1, 4) if jobs is not None else None
    rc = _lib.lib().nsa_paged_kv_copy_pages(ctypes.byref(kw.get("pd") or pkv.native_desc()), kw.get("ptr", dj.data_ptr() if dj is not None else None),
                                            len(jobs) if n_jobs is None else n_jobs, kw.get("G_", G), kw.get("Dk", pkv.d_k), kw.get("Dv", pkv.d_v),
                                            kw.get("dtype", _DT[pkv._K_sel.dtype]), _stream(dev))
    torch.cuda.synchronize()
    return rc


def row_runs(name, t0, t1):
    """(page position j, first row in the page, first row of the sequence, count) of the rows [t0, t1) of a token tensor, or of the
    compressed rows [n_cmp(t0), n_cmp(t1)) of a compressed one"""
    rows, lo, hi = (64, ncmp(t0), ncmp(t1)) if name in POOLS[6:] else (1024, t0, t1)
    out = []
    for j in range(lo // rows, (hi + rows - 1) // rows):
        r0, r1 = max(lo, j * rows), min(hi, (j + 1) * rows)
        if r1 > r0:
            out.append((j, r0 - j * rows, r0, r1 - r0))
    return out


def indexed_store(pools, kv, table_row, t0, t1, n_pages=N_PAGES):
    """torch indexing: rows of slab B_SRC into the pages of table_row; a page id outside [0, n_pages) skips its rows"""
    for name in POOLS:
        for j, r, s, k in row_runs(name, t0, t1):
            if 0 <= table_row[j] < n_pages:
                pools[name][table_row[j], :, r:r + k] = getattr(kv, name)[B_SRC, :, s:s + k]


def indexed_load(slabs, pools, table_row, t0, t1, n_pages=N_PAGES):
    for name in POOLS:
        for j, r, s, k in row_runs(name, t0, t1):
            if 0 <= table_row[j] < n_pages:
                slabs[name][B_SRC, :, s:s + k] = pools[name][table_row[j], :, r:r + k]


@pytest.mark.parametrize("D, dtype", CONFIGS, ids=IDS)
def test_store_and_load_round_trip_every_byte(D, dtype):
    pkv, kv = make(D, dtype)
    clean = snapshot(pkv)
    src = snapshot(kv)
    for t0, t1 in RANGES:
        for name in POOLS:
            getattr(pkv, name).copy_(clean[name])
        exp = {n: v.clone() for n, v in clean.items()}
        indexed_store(exp, kv, TABLE[SLOT], t0, t1)
        assert call("nsa_paged_kv_store", pkv, kv, t0, t1) == 0, (t0, t1)
        assert same(pkv, exp) == [], (t0, t1, "the pools after store: the indexed copy's rows, the poison everywhere else")
        assert same(kv, src) == [], (t0, t1, "store does not write the slab")
        # load into a poisoned two-slab cache: exactly the rows, nothing else
        for name in POOLS:
            poison(getattr(kv, name))
        exp_slab = snapshot(kv)
        for name in POOLS:
            for _, _, s, k in row_runs(name, t0, t1):
                exp_slab[name][B_SRC, :, s:s + k] = src[name][B_SRC, :, s:s + k]
        assert call("nsa_paged_kv_load", pkv, kv, t0, t1) == 0, (t0, t1)
        assert same(kv, exp_slab) == [], (t0, t1, "the slab after load: the stored rows, the poison everywhere else")
        assert same(pkv, exp) == [], (t0, t1, "load does not write the pools")
        for name in POOLS:
            getattr(kv, name).copy_(src[name])


def test_load_sequence_and_gather_sequence_take_the_native_path_bit_for_bit():
    """the methods on HIP tensors against the torch-indexing path on a clone; the slot's own allocation (pages 0, 1, 2 after a spare)"""
    pkv, kv = make(64, torch.bfloat16, table=[[-1] * 3, [-1] * 3])
    kv1 = kv.sequence_view(B_SRC)
    pkv.ensure(0, 1)
    for t0, t1 in [(0, 1500), (1500, 2049), (1024, 1030)]:
        pkv.ensure(1, t1)
        exp = snapshot(pkv)
        for name in POOLS:
            for j, r, s, k in row_runs(name, t0, t1):
                exp[name][pkv.pages[1][j], :, r:r + k] = getattr(kv, name)[B_SRC, :, s:s + k]
        pkv.load_sequence(1, kv1, t1, t0=t0)
        torch.cuda.synchronize()
        assert same(pkv, exp) == [], (t0, t1)
    back = pkv.gather_sequence(1, 2049)
    part = pkv.gather_sequence(1, 2049, t0=1030)
    torch.cuda.synchronize()
    assert (back.t, back.n_cmp, back.S_max) == (2049, 127, 3072)
    for name in POOLS:
        n, lo = (127, ncmp(1030)) if name in POOLS[6:] else (2049, 1030)
        assert torch.equal(bits(getattr(back, name)[:, :, :n]), bits(getattr(kv, name)[B_SRC:B_SRC + 1, :, :n])), name
        assert int(torch.count_nonzero(getattr(back, name)[:, :, n:])) == 0, name
        assert torch.equal(bits(getattr(part, name)[:, :, lo:n]), bits(getattr(kv, name)[B_SRC:B_SRC + 1, :, lo:n])), name
        assert int(torch.count_nonzero(getattr(part, name)[:, :, :lo])) == 0 and int(torch.count_nonzero(getattr(part, name)[:, :, n:])) == 0, name


@pytest.mark.parametrize("bad", [-1, N_PAGES, -(1 << 31), (1 << 31) - 1])
def test_a_bad_table_entry_skips_its_page_only(bad):
    table = [TABLE[0], [5, bad, 6]]
    pkv, kv = make(128, torch.bfloat16, table=table)
    exp = snapshot(pkv)
    indexed_store(exp, kv, table[SLOT], 0, 2049)
    src = snapshot(kv)
    assert call("nsa_paged_kv_store", pkv, kv, 0, 2049) == 0
    assert same(pkv, exp) == [] and same(kv, src) == []
    assert torch.equal(bits(pkv._K_raw[6, :, 0]), bits(kv._K_raw[B_SRC, :, 2048]))  # (the page behind the bad entry got its row)
    for name in POOLS:
        poison(getattr(kv, name))
    exp_slab = snapshot(kv)
    indexed_load(exp_slab, exp, table[SLOT], 0, 2049)
    assert call("nsa_paged_kv_load", pkv, kv, 0, 2049) == 0
    assert same(kv, exp_slab) == [] and same(pkv, exp) == []
    # rows 1024 .. 2047 and compressed rows 64 .. 126 of the slab kept their poison; rows around them arrived
    assert torch.equal(bits(kv._V_win[B_SRC, :, 1023]), bits(src["_V_win"][B_SRC, :, 1023])) and torch.equal(bits(kv._V_win[B_SRC, :, 2048]), bits(src["_V_win"][B_SRC, :, 2048]))


def test_copy_pages_counts_and_poison_beyond_them():
    pkv, kv = make(64, torch.float16)
    g = torch.Generator(device="cuda").manual_seed(5)
    for name in POOLS:
        pool = getattr(pkv, name)
        pool[:3] = torch.randn(pool[:3].shape, generator=g, device="cuda").to(pool.dtype)
    jobs = [(0, 3, 0, 64), (1, 4, 7, 0), (2, 5, 1024, 1)]
    exp = snapshot(pkv)
    for s, d, nt, nc in jobs:
        for name in POOLS:
            k = nc if name in POOLS[6:] else nt
            exp[name][d, :, :k] = exp[name][s, :, :k]
    assert copy_pages(pkv, jobs) == 0
    assert same(pkv, exp) == []
    assert torch.equal(bits(pkv._K_sel[4, :, :7]), bits(pkv._K_sel[1, :, :7])) and not torch.equal(bits(pkv._K_sel[4, :, 7]), bits(pkv._K_sel[1, :, 7]))
    assert torch.equal(bits(pkv._V_raw[5]), bits(pkv._V_raw[2])) and torch.equal(bits(pkv._V_cmp[3]), bits(pkv._V_cmp[0]))


def test_copy_pages_skips_a_bad_job_and_copies_its_neighbours():
    pkv, kv = make(128, torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(6)
    for name in POOLS:
        pool = getattr(pkv, name)
        pool[:3] = torch.randn(pool[:3].shape, generator=g, device="cuda").to(pool.dtype)
    good = [(0, 3, 1000, 63), (1, 4, 1024, 64), (2, 5, 16, 0)]
    jobs = [good[0], (N_PAGES, 6, 10, 1), (-1, 6, 10, 1), good[1], (1, N_PAGES, 10, 1), (1, -1, 10, 1), (1, 6, 1025, 1), (1, 6, 10, 65), (1, 6, -1, 1),
            (1, 6, 10, -1), (1 << 30, 6, 10, 1), good[2]]
    exp = snapshot(pkv)
    for s, d, nt, nc in good:
        for name in POOLS:
            k = nc if name in POOLS[6:] else nt
            exp[name][d, :, :k] = exp[name][s, :, :k]
    assert copy_pages(pkv, jobs) == 0
    assert same(pkv, exp) == []  # page 6, the bad jobs' destination, kept its poison; pages 3, 4, 5 got their rows


def test_bad_arguments_are_declined_with_the_limit_named():
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.kv_cache import NSA_KV

    pkv, kv = make(64, torch.bfloat16)
    before, src = snapshot(pkv), snapshot(kv)
    small = NSA_KV(2, G, 64, 64, 1024, 32, 16, 64, 16, 512, "cuda", torch.bfloat16, auto_grow=False)

    def desc(obj, **fields):
        d = type(obj.native_desc())()
        ctypes.memmove(ctypes.byref(d), ctypes.byref(obj.native_desc()), ctypes.sizeof(d))
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    cases = [
        (dict(t0=5, t1=4), "0 <= t0 <= t1"),
        (dict(t0=-1, t1=4), "0 <= t0 <= t1"),
        (dict(t0=0, t1=S_MAX + 1), f"S_max = {S_MAX}"),
        (dict(t0=0, t1=1025, kd=small.native_desc()), "S_max = 1024"),
        (dict(t0=0, t1=2049, pd=desc(pkv, max_pages=2)), "max_pages * 1024 = 2048"),
        (dict(t0=0, t1=10, dtype=_lib.NSA_DT_F32), "bf16 / f16"),
        (dict(t0=0, t1=10, Dk=192), "{64, 128}"),
        (dict(t0=0, t1=10, Dv=32), "{64, 128}"),
        (dict(t0=0, t1=10, slot=2), "slot = 2 outside [0, B = 2)"),
        (dict(t0=0, t1=10, slot=-1), "slot = -1 outside"),
        (dict(t0=0, t1=10, b_src=2), "b_src = 2 outside [0, B = 2)"),
        (dict(t0=0, t1=10, b_src=-1), "b_src = -1 outside"),
        (dict(t0=0, t1=10, G_=0), "G = 0"),
        (dict(t0=0, t1=10, pd=desc(pkv, K_win=None)), "null pool pointer"),
        (dict(t0=0, t1=10, pd=desc(pkv, V_cmp=pkv._V_cmp.data_ptr() + 2)), "16-byte aligned"),
        (dict(t0=0, t1=10, kd=desc(kv, V_raw=None)), "null cache pointer"),
        (dict(t0=0, t1=10, kd=desc(kv, K_sel=kv._K_sel.data_ptr() + 8)), "16-byte aligned"),
        (dict(t0=0, t1=10, pd=desc(pkv, block_table=None)), "null block table"),
        (dict(t0=0, t1=10, pd=desc(pkv, block_table=pkv.block_table.data_ptr() + 2)), "4-byte aligned"),
        (dict(t0=0, t1=10, pd=desc(pkv, table_stride=2)), "max_pages = 3"),
        (dict(t0=0, t1=10, pd=desc(pkv, n_pages=0)), "n_pages = 0"),
        (dict(t0=0, t1=10, pd=desc(pkv, max_pages=0)), "max_pages = 0"),
    ]
    for name in ("nsa_paged_kv_store", "nsa_paged_kv_load"):
        for kw, needle in cases:
            assert call(name, pkv, kv, **kw) == -1, (name, kw)
            assert needle in _lib.last_error() and name[4:] in _lib.last_error(), (name, kw, _lib.last_error())
        assert call(name, pkv, kv, 700, 700) == 0  # t0 == t1: NSA_OK and nothing done
    jobs = [(0, 1, 5, 1)]
    for kw, needle in [(dict(ptr=None), "null job array"), (dict(n_jobs=-1), "n_jobs = -1"), (dict(dtype=_lib.NSA_DT_F32), "bf16 / f16"),
                       (dict(Dk=96), "{64, 128}"), (dict(G_=-1), "G = -1"), (dict(pd=desc(pkv, V_sel=None)), "null pool pointer"),
                       (dict(pd=desc(pkv, K_cmp=pkv._K_cmp.data_ptr() + 4)), "16-byte aligned")]:
        assert copy_pages(pkv, jobs, **kw) == -1, kw
        assert needle in _lib.last_error() and "paged_kv_copy_pages" in _lib.last_error(), (kw, _lib.last_error())
    assert copy_pages(pkv, [], n_jobs=0, ptr=None) == 0  # n_jobs == 0: NSA_OK and nothing done
    assert same(pkv, before) == [] and same(kv, src) == []
