"""GPU: prefix sharing between paged decode slots end to end -- NSA_PagedKV.fork / own_tail / truncate / free under reference counts, and
NSAAttention.prefill_paged, around the unchanged NSAAttention.decode_paged.

The oracle of every decode here is the SAME public calls on a second, unshared NSA_PagedKV into which every sequence was loaded separately:
sharing must not change one bit of y, of the selected ranges, or of any of the eight cache tensors of any slot.  Pools are poisoned with
+-3e4; comparisons are on bit patterns (int16 views).  t = 1024 and t = 1030 are the cases an unclosed shared page fails: all three
sequences emit compressed row 63 (raw rows 1008 .. 1039) into page 0 with different values."""
import pytest
import torch

from test_hip_layer_decode_paged import model
from test_hip_layer_decode_ragged import seq

pytestmark = pytest.mark.gpu

POOLS = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp")
N_PAGES, MAX_PAGES, CAP = 12, 3, 3072
MODELS = ["m7c", "d128"]  # D = 64 and D = 128


def ncmp(t):
    return 0 if t < 32 else (t - 32) // 16 + 1


def closed(j, t):
    return t >= 1024 * (j + 1) + 16


def bits(x):
    return x.contiguous().view(torch.int16)


def poison(t):
    n = t.numel()
    v = torch.where(torch.arange(n, device=t.device) % 2 == 0, 3e4, -3e4)
    t.copy_(v.to(t.dtype).view_as(t))


def pool(m, B=3):
    dtype = m.W_Q.weight.dtype
    p = m.new_paged_kv(N_PAGES, B, MAX_PAGES, "cuda", dtype)
    for name in POOLS:
        poison(getattr(p, name))
    return p


def tokens(m, B, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, S, m.dim, generator=g, device="cuda").to(m.W_Q.weight.dtype)


def step(m, p, x, positions, S):
    """one decode_paged call of S tokens per slot at `positions` (host list; -1: an idle slot) -> y, ranges"""
    live = [q for q in positions if q >= 0]
    for b, q in enumerate(positions):
        if q >= 0:
            p.ensure(b, q + S)
    t_pos = torch.tensor(positions, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        y, _ = m.decode_paged(x, p, t_pos, t_max=max(live) + S - 1)
    torch.cuda.synchronize()
    return y.clone(), m._last_ranges.clone()


def gathered(p, b, t):
    kv1 = p.gather_sequence(b, t)
    torch.cuda.synchronize()
    return {n: getattr(kv1, n)[:, :, :(ncmp(t) if n in POOLS[6:] else t)].clone() for n in POOLS}


def same_cache(a, b):
    return [n for n in POOLS if not torch.equal(bits(a[n]), bits(b[n]))]


def forked_and_plain(name, t):
    """one prompt of t tokens in slot 0 forked into slots 1 and 2 of a shared pool; the same three sequences loaded one by one into a
    second pool"""
    m = model(name)
    _, kv1 = seq(name, t, CAP)
    shared, plain = pool(m), pool(m)
    shared.load_sequence(0, kv1, t)
    shared.fork(0, 1, t)
    shared.fork(0, 2, t)
    for b in range(3):
        plain.load_sequence(b, kv1, t)
    return m, shared, plain


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("t", [1000, 1024, 1030, 1040, 2100])
def test_diverging_decode_after_a_fork(name, t):
    m, shared, plain = forked_and_plain(name, t)
    # what is shared is what the closed-page rule allows, and nothing else
    for j in range((t + 1023) // 1024):
        ids = [shared.pages[b][j] for b in range(3)]
        if closed(j, t):
            assert ids[0] == ids[1] == ids[2] and shared._refs[ids[0]] == 3, (t, j, ids)
        else:
            assert len(set(ids)) == 3 and all(shared._refs[i] == 1 for i in ids), (t, j, ids)
    if t in (1024, 1030):
        assert shared.shared_pages(0) == [], "page 0 is not closed before t = 1040"
    if t == 1040:
        assert shared.shared_pages(1) == [shared.pages[0][0]] and shared.page_refs(2) == [3, 1]
    assert plain.shared_pages(0) == [] and plain.page_refs(1) == [1] * len(plain.pages[1])
    x = tokens(m, 3, 20, seed=t)  # different tokens per slot
    assert ncmp(t + 20) > ncmp(t) and (t not in (1024, 1030) or t < 1040 <= t + 20)  # every case emits; the two cross position 1040
    for t0, S in ((t, 16), (t + 16, 4)):
        ys, rs = step(m, shared, x[:, t0 - t:t0 - t + S], [t0] * 3, S)
        yp, rp = step(m, plain, x[:, t0 - t:t0 - t + S], [t0] * 3, S)
        assert torch.isfinite(yp.float()).all()
        assert torch.equal(bits(ys), bits(yp)), (name, t, t0, "y", (ys.float() - yp.float()).abs().max().item())
        assert torch.equal(rs, rp), (name, t, t0, "ranges")
    assert not torch.equal(ys[0], ys[1]) and not torch.equal(ys[1], ys[2])  # (the sequences did diverge)
    for b in range(3):
        assert same_cache(gathered(shared, b, t + 20), gathered(plain, b, t + 20)) == [], (name, t, b)


@pytest.mark.parametrize("name", MODELS)
def test_counts_free_and_truncate_copy_on_write(name):
    t = 2100
    m, shared, plain = forked_and_plain(name, t)
    assert [shared.page_refs(b) for b in range(3)] == [[3, 3, 1]] * 3
    x = tokens(m, 3, 10, seed=1)
    ys, rs = step(m, shared, x, [t] * 3, 10)  # every slot decoded to 2110
    yp, rp = step(m, plain, x, [t] * 3, 10)
    assert torch.equal(bits(ys), bits(yp)) and torch.equal(rs, rp)
    fork2 = gathered(shared, 2, t + 10)
    # truncate(1, 1500): the last page goes, page 1 (open at 1500, shared) becomes a private copy of its rows below 1500
    own = shared.pages[1][2]
    free_before = shared.free_pages
    shared.truncate(1, 1500)
    assert len(shared.pages[1]) == 2 and shared.block_table[1].tolist()[2] == -1 and shared._refs[own] in (0, 1)
    assert shared.page_refs(1) == [3, 1] and shared.page_refs(0) == [3, 2, 1] and shared.page_refs(2) == [3, 2, 1]
    assert shared.pages[1][1] != shared.pages[0][1] and shared.free_pages == free_before  # (one page back, one page out)
    assert same_cache(gathered(shared, 2, t + 10), fork2) == [], "the other fork reads what it read"
    _, kv1 = seq(name, t, CAP)
    plain.free(1)
    plain.load_sequence(1, kv1, 1500)
    assert same_cache(gathered(shared, 1, 1500), gathered(plain, 1, 1500)) == []
    x2 = tokens(m, 3, 8, seed=2)
    ys, rs = step(m, shared, x2, [-1, 1500, -1], 8)  # decoding from 1500 writes rows 1500 .. 1507 of page 1: the private copy
    yp, rp = step(m, plain, x2, [-1, 1500, -1], 8)
    assert torch.equal(bits(ys), bits(yp)) and torch.equal(rs, rp)
    assert same_cache(gathered(shared, 1, 1508), gathered(plain, 1, 1508)) == []
    assert same_cache(gathered(shared, 2, t + 10), fork2) == [] and same_cache(gathered(shared, 0, t + 10), gathered(plain, 0, t + 10)) == []
    # free: a page returns to the free list only when its last holder lets go, and the forks read on
    fork1 = gathered(shared, 1, 1508)
    n = shared.free_pages
    shared.free(0)
    assert shared.free_pages == n + 1 and shared.page_refs(1) == [2, 1] and shared.page_refs(2) == [2, 1, 1]
    assert same_cache(gathered(shared, 1, 1508), fork1) == [] and same_cache(gathered(shared, 2, t + 10), fork2) == []
    x3 = tokens(m, 3, 4, seed=3)
    ys, rs = step(m, shared, x3, [-1, 1508, t + 10], 4)  # the forks decode on without the source
    yp, rp = step(m, plain, x3, [-1, 1508, t + 10], 4)
    assert torch.equal(bits(ys), bits(yp)) and torch.equal(rs, rp)
    shared.free(1)
    assert shared.free_pages == n + 2 and shared.page_refs(2) == [1, 1, 1]
    shared.free(2)
    assert shared.free_pages == N_PAGES and sorted(shared._free) == list(range(N_PAGES)) and shared._refs == [0] * N_PAGES


@pytest.mark.parametrize("name", MODELS)
def test_prefill_paged_from_an_empty_slot(name):
    """t0 = 0: y and every byte of the pools as a prefill followed by the torch-indexing copy into the same pages"""
    m, t = model(name), 1500
    x, _ = seq(name, t, CAP)
    x = x[:, :t].contiguous()
    got, exp = pool(m), pool(m)
    for p in (got, exp):
        p.ensure(0, 1)  # slot 1's pages are not the first of the pools
    kv1 = m.new_kv(1, 2048, "cuda", x.dtype)
    with torch.no_grad():
        y_ref, _ = m(x, kv1, prefill=True)
        y = m.prefill_paged(x, got, 1)
    torch.cuda.synchronize()
    exp.ensure(1, t)
    for n in POOLS:  # the copy as NSA_PagedKV.load_sequence made it before the native call: torch indexing, page by page
        rows, k = (64, ncmp(t)) if n in POOLS[6:] else (1024, t)
        for j in range((k + rows - 1) // rows):
            c = min(rows, k - j * rows)
            getattr(exp, n)[exp.pages[1][j], :, :c] = getattr(kv1, n)[0, :, j * rows:j * rows + c]
    assert tuple(y.shape) == (1, t, m.dim) and torch.equal(bits(y), bits(y_ref))
    assert got.pages == exp.pages and torch.equal(got.block_table, exp.block_table)
    for n in POOLS:
        assert torch.equal(bits(getattr(got, n)), bits(getattr(exp, n))), n
    with pytest.raises(RuntimeError, match="inference only"):
        m.prefill_paged(x.clone().requires_grad_(), got, 2)
    with pytest.raises(ValueError, match="one sequence"):
        m.prefill_paged(torch.cat([x, x]), got, 2)


@pytest.mark.parametrize("name", MODELS)
def test_prefill_paged_extends_a_forked_slot(name):
    """t0 = 1030, S = 40 on a fork: the extend route on the gathered contiguous cache, and the source slot untouched.  The suffix crosses
    position 1040, so the fork writes compressed row 63 into ITS page 0"""
    m, t0, S = model(name), 1030, 40
    _, kv1 = seq(name, t0, CAP)
    p = pool(m)
    p.load_sequence(0, kv1, t0)
    p.fork(0, 1, t0)
    assert p.page_refs(1) == [1, 1] and p.shared_pages(0) == []
    source = gathered(p, 0, t0)
    ref = p.gather_sequence(0, t0)  # capacity 2048: the two pages
    x = tokens(m, 1, S, seed=4)
    with torch.no_grad():
        y_ref, _ = m(x, ref, prefill=True)  # kv.t = 1030: the extend route, decode-step semantics
        r_ref = m._last_ranges.clone()
        y = m.prefill_paged(x, p, 1, t0=t0)
    torch.cuda.synchronize()
    assert ref.t == t0 + S and torch.equal(bits(y), bits(y_ref)) and torch.equal(m._last_ranges, r_ref)
    want = {n: getattr(ref, n)[:, :, :(ncmp(t0 + S) if n in POOLS[6:] else t0 + S)] for n in POOLS}
    assert same_cache(gathered(p, 1, t0 + S), want) == []
    assert same_cache(gathered(p, 0, t0), source) == [], "the source slot reads what it read"
    assert ncmp(t0) == 63 and ncmp(t0 + S) == 65
    # and the slot decodes on from there like a sequence that was never forked
    plain = pool(m)
    plain.load_sequence(1, ref, t0 + S)
    x2 = tokens(m, 3, 4, seed=5)
    ys, rs = step(m, p, x2, [-1, t0 + S, -1], 4)
    yp, rp = step(m, plain, x2, [-1, t0 + S, -1], 4)
    assert torch.equal(bits(ys), bits(yp)) and torch.equal(rs, rp)
