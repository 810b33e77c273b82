"""NSA_PagedKV under sharing, on CPU tensors (no GPU): reference counts, fork, own_tail, truncate and the t0 forms of the two copy methods.

The closed-page rule restated here, independently of the code under test: page j of a sequence of t tokens may be shared iff
t >= 1024 (j + 1) + 16 -- from then on no append writes it (its last compressed row, 64 j + 63, is pooled from raw rows up to
1024 (j + 1) + 15).  Every expectation below follows from that rule and from the layout (token row r in row r & 1023 of page r >> 10,
compressed row c in row c & 63 of page c >> 6)."""
import pytest
import torch

POOLS = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp")
BOUNDARIES = [0, 1, 1023, 1024, 1039, 1040, 2048, 2063, 2064]


def ncmp(t):
    return 0 if t < 32 else (t - 32) // 16 + 1


def closed(j, t):
    return t >= 1024 * (j + 1) + 16


def paged(n_pages=9, B=3, max_pages=3, dtype=torch.bfloat16):
    from nsa_vibe_amd.kv_cache import NSA_PagedKV

    p = NSA_PagedKV(n_pages, B, max_pages, 2, 64, 64, 32, 16, 64, 16, 512, "cpu", dtype)
    for i, name in enumerate(POOLS):
        getattr(p, name).fill_(-3e4 if i & 1 else 3e4)
    return p


def sequence(t_cap=3072, seed=3):
    from nsa_vibe_amd.kv_cache import NSA_KV

    kv1 = NSA_KV(1, 2, 64, 64, t_cap, 32, 16, 64, 16, 512, "cpu", torch.bfloat16)
    g = torch.Generator().manual_seed(seed)
    for name in POOLS:
        buf = getattr(kv1, name)
        buf.copy_(torch.randn(buf.shape, generator=g).to(torch.bfloat16))
    return kv1


def fill_of(name):
    """what paged() filled the pool with, as bf16 rounds it"""
    return torch.tensor(-3e4 if POOLS.index(name) & 1 else 3e4, dtype=torch.bfloat16).float()


def bits(x):
    return x.contiguous().view(torch.int16)


def state(p):
    return (p.block_table.clone(), [list(v) for v in p.pages], list(p._free), list(p._refs), {n: getattr(p, n).clone() for n in POOLS})


def unchanged(p, s):
    return (torch.equal(p.block_table, s[0]) and p.pages == s[1] and p._free == s[2] and p._refs == s[3]
            and all(torch.equal(bits(getattr(p, n)), bits(s[4][n])) for n in POOLS))


def invariant(p):
    """every page is in exactly one place: on the free list with count 0, or named by as many table entries as its count says"""
    named = [0] * p.n_pages
    for b in range(p.B):
        row = p.block_table[b].tolist()
        assert row[:len(p.pages[b])] == p.pages[b] and all(v == -1 for v in row[len(p.pages[b]):]), (b, row, p.pages[b])
        for pg in p.pages[b]:
            named[pg] += 1
    assert sorted(p._free) == [pg for pg in range(p.n_pages) if named[pg] == 0], (p._free, named)
    assert len(set(p._free)) == len(p._free)
    assert p._refs == named, (p._refs, named)


def slot_rows(p, b, name, lo, hi):
    """rows [lo, hi) of slot b's sequence, read through its table -> [G, hi - lo, D]"""
    rows = 64 if name in POOLS[6:] else 1024
    parts = [getattr(p, name)[p.pages[b][j], :, max(lo, j * rows) - j * rows:min(hi, (j + 1) * rows) - j * rows]
             for j in range(lo // rows, (hi + rows - 1) // rows)]
    return torch.cat(parts, dim=1)


@pytest.mark.parametrize("t", BOUNDARIES)
def test_fork_shares_closed_pages_and_copies_the_open_ones(t):
    p, kv1 = paged(), sequence()
    p.ensure(2, 1)  # slot 0's pages are not the first of the pools
    p.load_sequence(0, kv1, 3072)
    src_pages = list(p.pages[0])
    before = state(p)
    p.fork(0, 1, t)
    invariant(p)
    need = (t + 1023) // 1024
    assert len(p.pages[1]) == need and p.pages[0] == src_pages
    private = [j for j in range(need) if not closed(j, t)]
    # the rule's consequence, spelled out: the last page, and the one before it while t & 1023 < 16
    assert private == ([] if t == 0 else sorted({(t - 1) >> 10} | ({(t >> 10) - 1} if t >= 1024 and (t & 1023) < 16 else set())))
    assert len(private) <= 2
    for j in range(need):
        if j in private:
            assert p.pages[1][j] != src_pages[j] and p._refs[p.pages[1][j]] == 1 and p._refs[src_pages[j]] == 1, (t, j)
        else:
            assert p.pages[1][j] == src_pages[j] and p._refs[src_pages[j]] == 2, (t, j)
    assert p.page_refs(1) == [1 if j in private else 2 for j in range(need)]
    assert p.shared_pages(1) == [src_pages[j] for j in range(need) if j not in private] == p.shared_pages(0)
    assert p.free_pages == len(before[2]) - len(private)
    # the fork reads as the first t tokens of the source, bit for bit; the copies end at the counts (the fill pattern stays behind them)
    for name in POOLS:
        n = ncmp(t) if name in POOLS[6:] else t
        if n:
            assert torch.equal(bits(slot_rows(p, 1, name, 0, n)), bits(getattr(kv1, name)[0, :, :n])), (t, name)
        rows = 64 if name in POOLS[6:] else 1024
        fill = fill_of(name)
        for j in private:
            k = max(0, min(rows, n - rows * j))
            assert bool((getattr(p, name)[p.pages[1][j], :, k:].float() == fill).all()), (t, name, j, k)
    # the source's pages hold what they held
    for name in POOLS:
        for pg in src_pages:
            assert torch.equal(bits(getattr(p, name)[pg]), bits(before[4][name][pg])), (t, name, pg)
    back = p.gather_sequence(1, t)
    for name in POOLS:
        n = ncmp(t) if name in POOLS[6:] else t
        assert torch.equal(bits(getattr(back, name)[:, :, :n]), bits(getattr(kv1, name)[:, :, :n])), (t, name)


@pytest.mark.parametrize("t", BOUNDARIES)
def test_own_tail_makes_the_pages_an_append_writes_private(t):
    p, kv1 = paged(), sequence()
    p.load_sequence(0, kv1, 3072)
    p.fork(0, 1, 3072)  # pages 0 and 1 shared (closed at 3072), page 2 private
    assert p.page_refs(1) == [2, 2, 1]
    was = list(p.pages[1])
    p.own_tail(1, t)
    invariant(p)
    todo = [j for j in range(3) if j <= t >> 10 and not closed(j, t) and j < 2]  # (page 2 is the fork's own already)
    for j in range(3):
        assert (p.pages[1][j] != was[j]) == (j in todo), (t, j)
        assert p._refs[p.pages[1][j]] == (1 if j in todo or j == 2 else 2), (t, j)
    for name in POOLS:  # the rows below t read as before
        n = ncmp(t) if name in POOLS[6:] else t
        if n:
            assert torch.equal(bits(slot_rows(p, 1, name, 0, n)), bits(getattr(kv1, name)[0, :, :n])), (t, name)
    p.own_tail(1, t)  # idempotent
    assert [p._refs[pg] for pg in p.pages[1]] == [1 if j in todo or j == 2 else 2 for j in range(3)]
    invariant(p)


def test_exhaustion_in_fork_and_own_tail_raises_and_changes_nothing():
    p, kv1 = paged(n_pages=4), sequence()
    p.load_sequence(0, kv1, 3072)  # three of four pages
    s = state(p)
    with pytest.raises(RuntimeError, match="pool exhausted"):
        p.fork(0, 1, 1030)  # pages 0 and 1 both open at 1030: two private pages, one is free
    assert unchanged(p, s)
    p.fork(0, 1, 1040)  # page 0 shared, one private page: fits
    invariant(p)
    assert p.free_pages == 0 and p.page_refs(1) == [2, 1]
    s = state(p)
    with pytest.raises(RuntimeError, match="pool exhausted"):
        p.own_tail(1, 1000)  # would need a private copy of page 0
    with pytest.raises(RuntimeError, match="pool exhausted"):
        p.own_tail(0, 1000)
    with pytest.raises(RuntimeError, match="pool exhausted"):
        p.truncate(1, 1030)  # releases nothing, and page 0 (open at 1030, shared) would need a private copy
    assert unchanged(p, s)


def test_truncate_supplies_its_private_page_from_what_it_releases():
    p, kv1 = paged(n_pages=4), sequence()
    p.load_sequence(0, kv1, 3072)
    p.fork(0, 1, 1040)
    assert p.free_pages == 0
    p.truncate(1, 1000)  # page 1 of the fork goes back, and comes out again as the private copy of page 0
    invariant(p)
    assert len(p.pages[1]) == 1 and p.page_refs(1) == [1] and p.page_refs(0) == [1, 1, 1] and p.free_pages == 0
    for name in POOLS:
        n = ncmp(1000) if name in POOLS[6:] else 1000
        assert torch.equal(bits(slot_rows(p, 1, name, 0, n)), bits(getattr(kv1, name)[0, :, :n])), name
    s = state(p)
    p.fork(0, 2, 0)  # an empty fork takes nothing
    assert unchanged(p, s) and p.pages[2] == []
    with pytest.raises(RuntimeError, match="pool exhausted"):
        p.fork(0, 2, 5)
    assert unchanged(p, s)


def test_free_order_with_shared_pages_and_truncate_to_zero():
    p, kv1 = paged(), sequence()
    p.load_sequence(0, kv1, 2100)  # pages 0, 1, 2
    p.fork(0, 1, 2100)  # shares 0 and 1 (2100 >= 2064), copies page 2 into page 3
    p.fork(0, 2, 2100)  # ... into page 4
    invariant(p)
    assert p.pages == [[0, 1, 2], [0, 1, 3], [0, 1, 4]] and [p._refs[i] for i in range(5)] == [3, 3, 1, 1, 1] and p.free_pages == 4
    p.free(0)  # only its own page 2 comes back
    invariant(p)
    assert p.free_pages == 5 and p._free[-1] == 2 and [p._refs[i] for i in range(3)] == [2, 2, 0]
    with pytest.raises(RuntimeError, match="not empty"):
        p.fork(1, 2, 100)
    with pytest.raises(RuntimeError, match="both slot"):
        p.fork(1, 1, 100)
    with pytest.raises(ValueError):
        p.fork(1, 0, 3073)  # beyond the source's pages
    p.truncate(1, 0)  # = free(1)
    invariant(p)
    assert p.pages[1] == [] and p.free_pages == 6 and [p._refs[i] for i in range(2)] == [1, 1] and p.block_table[1].tolist() == [-1, -1, -1]
    assert p.page_refs(2) == [1, 1, 1] and p.shared_pages(2) == []
    p.free(2)  # the last holder: pages 0 and 1 come back now, and not before
    invariant(p)
    assert p.free_pages == 9 and sorted(p._free) == list(range(9))


def test_truncate_releases_pages_and_owns_the_tail():
    p, kv1 = paged(), sequence()
    p.load_sequence(0, kv1, 2100)
    p.fork(0, 1, 2100)
    assert p.pages[1] == [0, 1, 3]
    other = {n: getattr(p.gather_sequence(0, 2100), n).clone() for n in POOLS}
    p.truncate(1, 1500)  # page 2 of the fork released; page 1 (open at 1500) was shared: now a private copy of its rows below 1500
    invariant(p)
    assert p.pages[1][0] == 0 and p.pages[1][1] != 1
    assert len(p.pages[1]) == 2 and p.page_refs(1) == [2, 1] and p.block_table[1].tolist()[2] == -1
    assert p.page_refs(0) == [2, 1, 1]
    for name in POOLS:
        n = ncmp(1500) if name in POOLS[6:] else 1500
        assert torch.equal(bits(slot_rows(p, 1, name, 0, n)), bits(getattr(kv1, name)[0, :, :n])), name
        assert torch.equal(bits(getattr(p.gather_sequence(0, 2100), name)), bits(other[name])), name
    with pytest.raises(ValueError):
        p.truncate(1, 2049)  # beyond the slot's pages
    p.truncate(1, 1500)  # idempotent
    invariant(p)
    assert p.page_refs(1) == [2, 1]


def test_partial_load_and_gather_copy_only_their_rows():
    p, kv1 = paged(), sequence()
    p.load_sequence(0, kv1, 1000)
    before = state(p)
    p.load_sequence(0, kv1, 1040, t0=1000)  # rows 1000 .. 1039 in two pages, compressed rows 61 .. 63
    invariant(p)
    assert len(p.pages[0]) == 2
    for name in POOLS:
        cmp = name in POOLS[6:]
        n = ncmp(1040) if cmp else 1040
        assert torch.equal(bits(slot_rows(p, 0, name, 0, n)), bits(getattr(kv1, name)[0, :, :n])), name
        pool = getattr(p, name)
        fill = fill_of(name)
        if cmp:
            assert ncmp(1000) == 61 and n == 64
            assert bool((pool[p.pages[0][1]].float() == fill).all()), name  # no compressed row in the second page yet
        else:
            assert bool((pool[p.pages[0][1], :, 16:].float() == fill).all()), name
        assert torch.equal(bits(pool[p.pages[0][0], :, :(61 if cmp else 1000)]), bits(before[4][name][p.pages[0][0], :, :(61 if cmp else 1000)])), name
    part = p.gather_sequence(0, 1040, t0=1024)
    for name in POOLS:
        lo, hi = (ncmp(1024), ncmp(1040)) if name in POOLS[6:] else (1024, 1040)
        got = getattr(part, name)
        assert torch.equal(bits(got[:, :, lo:hi]), bits(getattr(kv1, name)[:, :, lo:hi])), name
        assert int(torch.count_nonzero(got[:, :, :lo])) == 0 and int(torch.count_nonzero(got[:, :, hi:])) == 0, name
    with pytest.raises(ValueError):
        p.load_sequence(0, kv1, 1000, t0=1001)


def test_load_sequence_refuses_to_write_a_shared_page():
    p, kv1 = paged(), sequence()
    p.load_sequence(0, kv1, 2100)
    p.fork(0, 1, 2100)  # pages 0 and 1 shared
    s = state(p)
    with pytest.raises(RuntimeError, match="shared"):
        p.load_sequence(1, kv1, 2100, t0=100)  # page 1 lies above row 100 and is shared: a rollback goes through truncate
    assert unchanged(p, s)
    p.truncate(1, 100)
    p.load_sequence(1, sequence(seed=5), 2100, t0=100)  # page 0 is private now (own_tail), pages 1 and 2 fresh
    invariant(p)
    assert p.page_refs(1) == [1, 1, 1] and p.page_refs(0) == [1, 1, 1]
    back = p.gather_sequence(0, 2100)  # the source still reads as it did
    for name in POOLS:
        n = ncmp(2100) if name in POOLS[6:] else 2100
        assert torch.equal(bits(getattr(back, name)[:, :, :n]), bits(getattr(kv1, name)[:, :, :n])), name


def test_host_check_program_of_the_native_copies_passes():
    """csrc/paged_kv_copy_check.cpp (built beside the library): every decline path and the grid sizes of nsa_paged_kv_store / _load /
    _copy_pages as a host program of its own, no HIP and no GPU"""
    import os
    import subprocess

    from nsa_vibe_amd import _lib

    _lib.lib()  # (built with the library)
    exe = os.path.join(os.path.dirname(_lib.LIB_PATH), "paged_kv_copy_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "checks passed" in r.stdout, r.stdout + r.stderr
