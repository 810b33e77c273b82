"""NSA_PagedKV on CPU tensors (no GPU): the page allocator, the block table, the two copy methods, the native descriptor, and what
NSAAttention.decode_paged refuses before any native call."""
import pytest
import torch

POOLS = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp")


def paged(n_pages=5, B=3, max_pages=3, dtype=torch.float32):
    from nsa_vibe_amd.kv_cache import NSA_PagedKV

    return NSA_PagedKV(n_pages, B, max_pages, 2, 64, 64, 32, 16, 64, 16, 512, "cpu", dtype)


def test_layout_and_initial_table():
    p = paged()
    for name in POOLS[:6]:
        assert tuple(getattr(p, name).shape) == (5, 2, 1024, 64) and getattr(p, name).is_contiguous(), name
    for name in POOLS[6:]:
        assert tuple(getattr(p, name).shape) == (5, 2, 64, 64) and getattr(p, name).is_contiguous(), name
    assert p.block_table.dtype == torch.int32 and tuple(p.block_table.shape) == (3, 3) and bool((p.block_table == -1).all())
    assert (p.capacity, p.free_pages, p.pages) == (3072, 5, [[], [], []])
    with pytest.raises(ValueError, match="default block geometry"):
        from nsa_vibe_amd.kv_cache import NSA_PagedKV

        NSA_PagedKV(5, 3, 3, 2, 64, 64, 32, 16, 128, 16, 512, "cpu", torch.float32)


def test_ensure_is_idempotent_and_the_table_is_as_assigned():
    p = paged()
    p.ensure(0, 1)
    assert p.pages[0] == [0] and p.block_table[0].tolist() == [0, -1, -1] and p.free_pages == 4
    p.ensure(0, 1024)  # still one page
    p.ensure(0, 0)
    assert p.pages[0] == [0] and p.free_pages == 4
    p.ensure(1, 1025)  # two pages
    assert p.pages[1] == [1, 2] and p.block_table[1].tolist() == [1, 2, -1]
    p.ensure(0, 1025)  # slot 0 grows: its first page stays where it is
    assert p.pages[0] == [0, 3] and p.block_table[0].tolist() == [0, 3, -1] and p.free_pages == 1
    p.ensure(0, 2048)
    p.ensure(1, 7)
    assert p.block_table.tolist() == [[0, 3, -1], [1, 2, -1], [-1, -1, -1]] and p.free_pages == 1
    assert sorted(p.pages[0] + p.pages[1] + p._free) == [0, 1, 2, 3, 4]  # every page is in exactly one place


def test_exhaustion_raises_and_assigns_nothing():
    p = paged()
    p.ensure(0, 3072)
    p.ensure(1, 1)
    before = (p.block_table.clone(), [list(v) for v in p.pages], p.free_pages)
    with pytest.raises(RuntimeError, match="pool exhausted"):
        p.ensure(1, 3072)  # needs two more, one is free
    with pytest.raises(RuntimeError, match="capacity"):
        p.ensure(2, 3073)  # beyond max_pages
    with pytest.raises(IndexError):
        p.ensure(3, 1)
    assert torch.equal(p.block_table, before[0]) and p.pages == before[1] and p.free_pages == before[2] == 1


def test_free_returns_the_pages_and_resets_the_entries():
    p = paged()
    p.ensure(0, 2048)
    p.ensure(1, 2048)
    p.free(0)
    assert p.block_table.tolist() == [[-1, -1, -1], [2, 3, -1], [-1, -1, -1]] and p.pages[0] == [] and p.free_pages == 3
    p.free(0)  # an empty slot: nothing to return
    assert p.free_pages == 3
    p.ensure(2, 3072)  # the returned pages are handed out again
    assert sorted(p.pages[2]) == [0, 1, 4] and p.free_pages == 0
    p.free(1)
    p.free(2)
    assert p.free_pages == 5 and bool((p.block_table == -1).all()) and sorted(p._free) == [0, 1, 2, 3, 4]


def test_load_then_gather_round_trips_bit_for_bit():
    from nsa_vibe_amd.kv_cache import NSA_KV

    p = paged(dtype=torch.bfloat16)
    for name in POOLS:
        getattr(p, name).fill_(float("nan"))
    kv1 = NSA_KV(1, 2, 64, 64, 2048, 32, 16, 64, 16, 512, "cpu", torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    for name in POOLS:
        buf = getattr(kv1, name)
        buf.copy_(torch.randn(buf.shape, generator=g).to(torch.bfloat16))
    p.ensure(0, 1)  # slot 1's pages are not the first ones of the pools
    t = 1500  # 1500 tokens in two pages, n_cmp = 92 compressed rows in two compressed pages
    p.load_sequence(1, kv1, t)
    assert p.pages[1] == [1, 2] and p.block_table[1].tolist() == [1, 2, -1]
    assert torch.equal(p._K_win[1, :, :1024], kv1._K_win[0, :, :1024]) and torch.equal(p._K_win[2, :, :476], kv1._K_win[0, :, 1024:1500])
    assert torch.equal(p._V_cmp[1], kv1._V_cmp[0, :, :64]) and torch.equal(p._V_cmp[2, :, :28], kv1._V_cmp[0, :, 64:92])
    assert bool(torch.isnan(p._K_win[2, :, 476:]).all()) and bool(torch.isnan(p._V_cmp[2, :, 28:]).all()) and bool(torch.isnan(p._K_sel[0]).all())
    back = p.gather_sequence(1, t)
    assert (back.B, back.t, back.n_cmp, back.S_max) == (1, t, 92, 2048)
    for name in POOLS:
        n = 92 if name in POOLS[6:] else t
        assert torch.equal(getattr(back, name)[:, :, :n], getattr(kv1, name)[:, :, :n]), name
        assert int(torch.count_nonzero(getattr(back, name)[:, :, n:])) == 0, name
    with pytest.raises(ValueError):
        p.gather_sequence(1, 2049)  # beyond the slot's pages
    with pytest.raises(RuntimeError, match="B = 1"):
        p.load_sequence(0, NSA_KV(2, 2, 64, 64, 64, 32, 16, 64, 16, 512, "cpu", torch.bfloat16), 10)


def test_native_desc_names_the_pools_and_the_table():
    p = paged()
    d = p.native_desc()
    assert d is p.native_desc()
    for name in POOLS:
        assert getattr(d, name[1:]) == getattr(p, name).data_ptr(), name
    assert (d.block_table, d.table_stride, d.n_pages, d.B, d.max_pages) == (p.block_table.data_ptr(), 3, 5, 3, 3)


def test_decode_paged_refuses_before_any_native_call(monkeypatch):
    from nsa_vibe_amd import NSA_PagedKV, _lib
    from nsa_vibe_amd.nsa_attention import NSAAttention

    m = NSAAttention(768, 12, 2, 64, 64, l=32, d=16, l_sel=64, n_sel=16, w=512, selector="sequential").eval()
    p = m.new_paged_kv(5, 3, 3, "cpu", torch.float32)
    assert isinstance(p, NSA_PagedKV) and (p.n_pages, p.B, p.max_pages, p.G, p.d_k) == (5, 3, 3, 2, 64)

    def no_native():
        raise AssertionError("a native call was made")

    monkeypatch.setattr(_lib, "lib", no_native)
    x = torch.zeros(3, 4, 768)
    pos = torch.tensor([10, 20, -1], dtype=torch.int32)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="HIP device tensors"):
            m.decode_paged(x, p, pos, t_max=30)
        with pytest.raises(ValueError, match="int32"):
            m.decode_paged(x, p, pos.long(), t_max=30)
        with pytest.raises(ValueError, match="int32"):
            m.decode_paged(x, p, [10, 20, -1], t_max=30)  # host positions: the lengths and the table live on the device
        with pytest.raises(ValueError, match="negative"):
            m.decode_paged(x, p, pos, t_max=-1)
        with pytest.raises(ValueError, match="1 to 16"):
            m.decode_paged(torch.zeros(3, 17, 768), p, pos, t_max=30)
    assert bool((p.block_table == -1).all())
