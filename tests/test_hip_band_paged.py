"""GPU parity: the sliding and the compressed branch of a ragged decode step over PAGED caches (nsa_band_attn_fwd_paged; the keyword
block_table= of sliding_window_attention, batched_causal_attention_compressed and band_attention_hip).

The specification is an equality and needs no tolerance: for a table that scatters contiguous caches into pool pages, in any order, O and
lse are those of nsa_band_attn_fwd_ragged on the contiguous caches bit for bit (torch.equal) -- the same tiles of 32 keys, masks, split
shares and epilogue on the same values.  The ragged call is itself pinned to the oracle by tests/test_hip_band_ragged.py, whose make_case
and run are reused here; its results are computed once per case.

Nothing is hidden in the inputs: every pool page that belongs to no sequence, every row of a page behind a sequence's own keys and the
spare pages hold +-3e4, and the table entries a sequence does not NEED -- those outside the key rows from the window start of its first
query row to the end of its last -- point at a valid, poisoned page: a kernel that follows them gets wrong values, never an address
outside the pools."""
import numpy as np
import pytest
import torch

from test_hip_band_ragged import BIG, D_, G, H, L, SETS, W, make_case, ncmp, run
from test_hip_selection import dev, nv  # noqa: F401

pytestmark = pytest.mark.gpu

BANDS = {"sliding": dict(a=0, dd=1, c=0, w=W), "compressed": dict(a=L, dd=D_, c=1, w=2 ** 30)}
PAGE = {"sliding": 1024, "compressed": 64}  # the sizes that share their page ids with selection_decode_paged


def key_rows(band, t0, S):
    """[lo_b, hi_b): the key rows a live sequence at t0 needs -- from the window start of its first row to the (unclamped) hi of its last"""
    hi = lambda t: 0 if t + 1 - band["a"] < 0 else (t + 1 - band["a"]) // band["dd"] + band["c"]  # noqa: E731
    return max(0, hi(t0) - band["w"]), hi(t0 + S - 1)


def scatter(K, V, t_pos, S, band, rows, slots=None, seed=0, spare=3, guard=0):
    """contiguous caches K / V [B, G, n, D] as pools: slot i of the paged batch holds the caches of sequence slots[i] (None: an empty slot),
    cut into pages of `rows` rows that a seeded permutation places in pools of (pages needed + spare) pages.  Only the pages a sequence
    NEEDS are placed and entered in the table; every other entry points at a spare page.  guard > 0: the pools are views that start
    `guard` pages into a larger allocation and end as many before its end -> pools, the table as nested lists, max_pages, n_pages"""
    D, dt = K.shape[-1], K.dtype
    slots = list(range(len(t_pos))) if slots is None else slots
    spans = [key_rows(band, t_pos[s], S) if s is not None and t_pos[s] >= 0 else (0, 0) for s in slots]
    pages = [list(range(lo // rows, (hi - 1) // rows + 1)) if hi > lo else [] for lo, hi in spans]
    max_pages = max([p[-1] + 1 for p in pages if p] + [0]) + 1
    n_pages = sum(len(p) for p in pages) + spare
    perm = [int(p) for p in np.random.default_rng(seed).permutation(n_pages)]

    def pool(val):
        return torch.full((n_pages + 2 * guard, G, rows, D), val, dtype=dt, device="cuda")[guard:guard + n_pages]

    Kp, Vp = pool(BIG), pool(-BIG)
    table = [[perm[-1]] * max_pages for _ in slots]  # entries nobody needs: a spare page -- valid, poisoned
    k = 0
    for i, (s, (lo, hi)) in enumerate(zip(slots, spans)):
        for j in pages[i]:
            p = table[i][j] = perm[k]
            k += 1
            r = min(rows, hi - rows * j)  # rows behind the sequence's last key keep the poison
            Kp[p, :, :r] = K[s, :, rows * j:rows * j + r]
            Vp[p, :, :r] = V[s, :, rows * j:rows * j + r]
    return dict(K=Kp, V=Vp, table=table, max_pages=max_pages, n_pages=n_pages)


def pools_of(c, branch, rows=None):
    """the pools of a case and branch, scattered once and never modified"""
    rows = rows or PAGE[branch]
    key = ("pools", branch, rows)
    if key not in c:
        K, V = c["kv"][branch]
        c[key] = scatter(K, V, c["t_pos"], c["S"], BANDS[branch], rows, seed=len(c["t_pos"]) + c["S"] + rows)
    return c[key]


def ragged_ref(nv, c, branch):
    """nsa_band_attn_fwd_ragged on the contiguous caches, once per case and branch"""
    key = ("ragged", branch)
    if key not in c:
        c[key] = run(nv, c, branch, lse=True)
    return c[key]


def paged(nv, c, pl, band, table=None, pos=None, t_max=None, Q=None):
    tb = torch.tensor(pl["table"] if table is None else table, dtype=torch.int32, device="cuda")
    return nv.band_attention_hip(c["Q"] if Q is None else Q, pl["K"], pl["V"], return_lse=True, t_pos=c["pos"] if pos is None else pos,
                                 t_max=c["t_max"] if t_max is None else t_max, block_table=tb, **band)


def assert_equal_bits(got, ref):
    torch.cuda.synchronize()
    assert torch.isfinite(got[0].float()).all()
    assert torch.equal(got[1], ref[1])
    assert torch.equal(got[0], ref[0])


def groups(B, S, D, nt):
    """token groups of the plan at nt column tiles (h = 6, G = 2): band_plan's count"""
    tpw = 16 * nt // H
    return B * G * ((S + tpw - 1) // tpw)


def workspace_bytes(nv, B, S, D, dtype=torch.bfloat16):
    from nsa_vibe_amd import _lib

    return _lib.lib().nsa_band_attn_fwd_paged_workspace(B, S, G, H, D, D, {torch.bfloat16: _lib.NSA_DT_BF16, torch.float16: _lib.NSA_DT_F16}[dtype])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("branch", ["sliding", "compressed"])
@pytest.mark.parametrize("name", list(SETS))
def test_split_form_equals_ragged_bit_for_bit(nv, name, branch, D, dtype):
    """few rows: the split form.  At h = 6 a wave holds 2 tokens: position 1052 walks from klo = 541, its 16th tile [1021, 1053) straddles
    row 1024 and its 17th is a tail tile; 4100 straddles 4096 at [4069, 4101); 1055 (klo = 544) meets the boundary tile-aligned"""
    t_pos, S = SETS[name]
    c = make_case(t_pos, S, D, dtype)
    assert workspace_bytes(nv, c["B"], S, D, dtype) > 0  # the split form
    assert_equal_bits(paged(nv, c, pools_of(c, branch), BANDS[branch]), ragged_ref(nv, c, branch))


def test_page_edges_and_entries_below_the_window(nv):
    """rows at the last / first token of a page; 1535's window starts exactly on a page start (row 1024) and 1536's one row behind it, so
    entry 0 of both is not needed: it is set to -1 and the sequences stay live with equal bits"""
    c = make_case([1023, 1024, 1535, 1536, 2047], 3, 64, torch.bfloat16)
    pl = pools_of(c, "sliding")
    assert key_rows(BANDS["sliding"], 1535, 3)[0] == 1024
    table = [row[:] for row in pl["table"]]
    table[2][0] = table[3][0] = -1
    O, lse = paged(nv, c, pl, BANDS["sliding"], table=table)
    assert bool((lse > -float("inf")).all())
    assert_equal_bits((O, lse), ragged_ref(nv, c, "sliding"))


@pytest.mark.parametrize("name", list(SETS))
def test_pages_of_32_rows_every_unaligned_tile_straddles(nv, name):
    t_pos, S = SETS[name]
    c = make_case(t_pos, S, 64, torch.bfloat16)
    assert_equal_bits(paged(nv, c, pools_of(c, "sliding", 32), BANDS["sliding"]), ragged_ref(nv, c, "sliding"))


def test_windowed_compressed_band_on_pages_of_64_rows(nv):
    """a general band (a = 32, dd = 16, c = 1, w = 100) over the compressed caches: unaligned tiles that straddle 64-row pages, and table
    entries below the window that are not needed"""
    t_pos, S = SETS["S3_boundaries"]
    c = make_case(t_pos, S, 64, torch.bfloat16)
    band = dict(a=L, dd=D_, c=1, w=100)
    K, V = c["kv"]["compressed"]
    pl = scatter(K, V, c["t_pos"], S, band, 64, seed=5)
    assert pl["table"][4][0] == pl["table"][4][-1]  # 5000: rows [211, 311) -- entries 0 .. 2 are not needed and point at the spare page
    ref = nv.band_attention_hip(c["Q"], K, V, return_lse=True, t_pos=c["pos"], t_max=c["t_max"], **band)
    assert_equal_bits(paged(nv, c, pl, band), ref)


_UNSPLIT = {}


def unsplit_case(S, D):
    """B = 32 sequences at positions drawn with a fixed seed from [600, 1500]"""
    if (S, D) not in _UNSPLIT:
        t_pos = [int(t) for t in np.random.default_rng(32 + S).integers(600, 1501, size=32)]
        _UNSPLIT[(S, D)] = make_case(t_pos, S, D, torch.bfloat16)
    return _UNSPLIT[(S, D)]


@pytest.mark.parametrize("branch", ["sliding", "compressed"])
@pytest.mark.parametrize("S,D,nt", [(32, 64, 1), (32, 128, 1), (256, 64, 3), (256, 128, 2)])
def test_unsplit_forms_equal_ragged_bit_for_bit(nv, S, D, nt, branch):
    """B = 32, S = 32: 1024 groups of 2 tokens, unsplit NT = 1.  S = 256: 2048 groups of 8 tokens, NT = 3 (D = 128: NT = 2, 5 tokens a wave)"""
    ntw = 3 if D == 64 else 2
    assert workspace_bytes(nv, 32, S, D) == 0  # unsplit
    assert (groups(32, S, D, ntw) >= 2048) == (nt == ntw) and (nt == ntw or groups(32, S, D, 1) >= 1024)  # band_plan's form
    c = unsplit_case(S, D)
    assert_equal_bits(paged(nv, c, pools_of(c, branch), BANDS[branch]), ragged_ref(nv, c, branch))


def test_more_than_64_table_entries_per_wave(nv):
    """compressed branch near 70,000 tokens on 64-row pages: 4,374 compressed rows = 69 pages, the unsplit walk of every wave crosses the
    window of 64 checked entries"""
    B, S, D, dt = 32, 32, 64, torch.bfloat16
    t_pos = [int(t) for t in np.random.default_rng(70).integers(69900, 69969, size=B)]
    t_max = max(t_pos) + S - 1
    n = ncmp(t_max)
    assert n > 64 * 64 + 32 and workspace_bytes(nv, B, S, D) == 0
    g = torch.Generator(device="cuda").manual_seed(70)
    Q = torch.randn((B, S, G, H, D), generator=g, device="cuda").to(dt)
    K = torch.randn((B, G, n, D), generator=g, device="cuda").to(dt)
    V = torch.randn((B, G, n, D), generator=g, device="cuda").to(dt)
    for b, t0 in enumerate(t_pos):
        K[b, :, ncmp(t0 + S - 1):], V[b, :, ncmp(t0 + S - 1):] = BIG, -BIG
    pos = torch.tensor(t_pos, dtype=torch.int32, device="cuda")
    band = BANDS["compressed"]
    pl = scatter(K, V, t_pos, S, band, 64, seed=70)
    assert pl["max_pages"] == 70
    c = dict(Q=Q, pos=pos, t_max=t_max)
    ref = nv.band_attention_hip(Q, K, V, return_lse=True, t_pos=pos, t_max=t_max, **band)
    assert_equal_bits(paged(nv, c, pl, band), ref)


@pytest.mark.parametrize("branch", ["sliding", "compressed"])
@pytest.mark.parametrize("S", [1, 2])
def test_inactive_slots(nv, S, branch):
    """a slot is inactive -- zero rows, lse = -inf -- with t_pos = -1, t_pos + S - 1 > t_max, a last row beyond max_pages * page_rows, a
    needed table entry equal to n_pages and one equal to -1; the other slots keep their bits.  The pools are views that start one page
    into a larger allocation and end one page before its end, and the smaller n_pages is passed: even an unguarded kernel stays inside
    it.  B S G is small, so this is the split form: the entry equal to n_pages is the second page of a sequence at 1055, which holds the
    keys of the LAST tiles only (S = 1, 16 splits -- sliding: rows [1024, 1056) of [544, 1056), the last split's one tile; compressed: row
    64 of [0, 65), the last split's tile) -- the whole row is zero, not a merge of the other splits"""
    base = make_case([1055, 40, 1190, 9], S, 64, torch.bfloat16)
    band, rows = BANDS[branch], PAGE[branch]
    O_ref, lse_ref = ragged_ref(nv, base, branch)
    sel = [0, 0, 2, 0, 0, 1, 3]  # the inputs of slot b are those of sequence sel[b] of the base case
    K, V = base["kv"][branch]
    pl = scatter(K, V, base["t_pos"], S, band, rows, slots=sel, seed=7 + S, guard=1)
    assert pl["max_pages"] == 3 and workspace_bytes(nv, len(sel), S, 64) > 0
    table = [row[:] for row in pl["table"]]
    table[3][1] = pl["n_pages"]  # one past the pools
    table[4][0] = -1
    Q = base["Q"][sel].contiguous()
    past_capacity = 2 * 1024 - S + 1 if branch == "sliding" else L + D_ * 2 * 64  # the first position whose last row needs key row 2 * rows
    assert key_rows(band, past_capacity, S)[1] == 2 * rows + 1
    # (max_pages, t_max, the position of slot 2): past the capacity of two pages; past t_max
    for max_pages, t_max, bad in ((2, past_capacity + S, past_capacity), (3, 1100, 1100 - S + 2)):
        pos = torch.tensor([1055, -1, bad, 1055, 1055, 40, 9], dtype=torch.int32, device="cuda")
        O, lse = paged(nv, base, pl, band, table=[row[:max_pages] for row in table], Q=Q, pos=pos, t_max=t_max)
        torch.cuda.synchronize()
        for b in (1, 2, 3, 4):
            assert not O[b].any() and bool((lse[b] == -float("inf")).all()), (max_pages, t_max, b)
        for b in (0, 5, 6):
            assert torch.equal(O[b], O_ref[sel[b]]) and torch.equal(lse[b], lse_ref[sel[b]]), (max_pages, t_max, b)


def test_pool_beyond_2_gib(nv):
    """pools that start 4 GiB into 7 GiB buffers, the case's pages at pool indices >= 8192 (a page of K is 256 KiB at D = 64, G = 2: byte
    offsets of 2 GiB and more), and +-3e4 where a sign-wrapped 32-bit offset would land (buffer + 2 .. 3 GiB): a wrong offset width reads
    poison inside the allocation.  Sliding branch, equal to the ragged call bit for bit"""
    c = make_case([1055, 2100], 1, 64, torch.bfloat16)
    D, dt, GiB, rows = 64, torch.bfloat16, 1 << 30, 1024
    n_pages, first, ps = 12288, 8192, G * rows * D
    K, V = c["kv"]["sliding"]
    src = scatter(K, V, c["t_pos"], 1, BANDS["sliding"], rows, seed=11, spare=1)

    def big_pool(val):
        flat = torch.empty(7 * GiB, dtype=torch.uint8, device="cuda").view(dt)
        flat[GiB:3 * GiB // 2].fill_(val)  # bytes + 2 GiB .. + 3 GiB
        return torch.as_strided(flat, (n_pages, G, rows, D), (ps, rows * D, D, 1), 2 * GiB)

    Kp, Vp = big_pool(BIG), big_pool(-BIG)
    assert Kp.stride(0) * 2 * first == 2 * GiB and Kp.data_ptr() - Kp.untyped_storage().data_ptr() == 4 * GiB
    for dst, s in ((Kp, src["K"]), (Vp, src["V"])):
        dst[first:first + src["n_pages"]] = s  # (the spare page, poisoned, comes along: the table entries nobody needs point at it)
    got = paged(nv, c, dict(K=Kp, V=Vp), BANDS["sliding"], table=[[first + p for p in row] for row in src["table"]])
    assert_equal_bits(got, ragged_ref(nv, c, "sliding"))


@pytest.mark.parametrize("branch", ["sliding", "compressed"])
def test_paged_run_to_run(nv, branch):
    t_pos, S = SETS["S3_boundaries"]
    c = make_case(t_pos, S, 64, torch.bfloat16)
    a = paged(nv, c, pools_of(c, branch), BANDS[branch])
    b = paged(nv, c, pools_of(c, branch), BANDS[branch])
    assert_equal_bits(a, b)


@pytest.mark.parametrize("branch", ["sliding", "compressed"])
def test_existing_entry_points_keep_their_bits(nv, branch):
    """the ragged call at equal positions and the scalar call on the same buffers are still bit-equal to each other, with a paged call
    over pools of the same caches between them (it equals both)"""
    t0 = 1052
    c = make_case([t0] * 3, 3, 64, torch.bfloat16)
    ref = ragged_ref(nv, c, branch)
    assert_equal_bits(paged(nv, c, pools_of(c, branch), BANDS[branch]), ref)
    assert_equal_bits(run(nv, c, branch, lse=True), run(nv, c, branch, t0=t0, lse=True))
    assert_equal_bits(ref, run(nv, c, branch, t0=t0, lse=True))


@pytest.mark.parametrize("branch", ["sliding", "compressed"])
def test_identity_table_over_a_reshaped_contiguous_cache(nv, branch):
    """B = 1, a contiguous cache whose capacity is a multiple of the page seen as pages in place (table 0, 1, ..): the scalar call at t0 bit
    for bit"""
    t0, S, D, dt = 1052, 4, 64, torch.bfloat16
    rows = PAGE[branch]
    own = key_rows(BANDS[branch], t0, S)[1]
    cap = (own + rows - 1) // rows * rows
    rng = np.random.default_rng([t0, S, cap])
    Q = dev(rng.standard_normal((1, S, G, H, D), dtype=np.float32), dt)
    K = rng.standard_normal((1, G, cap, D), dtype=np.float32)
    V = rng.standard_normal((1, G, cap, D), dtype=np.float32)
    K[:, :, own:], V[:, :, own:] = BIG, -BIG
    K, V = dev(K, dt), dev(V, dt)
    as_pages = lambda X: X[0].view(G, cap // rows, rows, D).permute(1, 0, 2, 3)  # noqa: E731  ([pages, G, rows, D], no copy)
    table = torch.arange(cap // rows, dtype=torch.int32, device="cuda").view(1, -1)
    band = BANDS[branch]
    got = nv.band_attention_hip(Q, as_pages(K), as_pages(V), return_lse=True, t_pos=[t0], block_table=table, **band)
    ref = nv.band_attention_hip(Q, K[:, :, :own], V[:, :, :own], t0=t0, return_lse=True, **band)
    assert_equal_bits(got, ref)
