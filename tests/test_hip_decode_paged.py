"""GPU parity: the ragged decode step of the selected branch over PAGED caches (nsa_sel_decode_paged: the ragged rows form of
decode_step_kernel with every K_cmp chunk, gathered K/V block and forced block found through a block table, pages of 1024 tokens).

The specification is an equality and needs no tolerance: for a table that scatters contiguous caches into pool pages, in any order, ranges
and O are those of nsa_sel_decode_ragged on the contiguous caches bit for bit -- the same form and waves planned from t_max and B S G, the
same arithmetic on the same values in the same order.  The cases are those of tests/test_hip_decode_ragged.py (its make_case and ragged
are reused, and its references are computed once per case) plus one at the page edges.

Nothing is hidden in the inputs: every pool page that belongs to no sequence, every row of a sequence's last page beyond its own tokens
and every compressed row beyond its n_cmp hold +-3e4, and the table entries beyond the pages a sequence needs point at a valid, poisoned
page -- a kernel that follows them gets wrong values, never an address outside the pools."""
import numpy as np
import pytest
import torch

from test_hip_decode_ragged import BIG, CASES, D_, G, IDS, L, L_SEL, N_TOP, W, make_case, ncmp, ragged
from test_hip_decode_ragged import plan as ragged_plan
from test_hip_selection import dev, nv  # noqa: F401  (nv: the module fixture of the D = 64 tests)

pytestmark = pytest.mark.gpu

PAGE = 1024


def scatter(c, slots=None, seed=0, spare=3, guard=0):
    """the contiguous caches of case c as pools: slot i of the paged batch holds the caches of sequence slots[i] of c (None: an empty
    slot), cut into pages that a seeded random permutation places in pools of (pages needed + spare) pages; guard > 0: the pools are views
    that start `guard` pages into a larger allocation and end as many before its end -> pools, the table as nested lists, max_pages"""
    S, D, dt = c["S"], c["D"], c["dtype"]
    slots = list(range(c["B"])) if slots is None else slots
    own = [c["t_pos"][s] + S if s is not None and c["t_pos"][s] >= 0 else 0 for s in slots]
    need = [(o + PAGE - 1) // PAGE for o in own]
    max_pages, n_pages = max(need) + 1, sum(need) + spare
    perm = [int(p) for p in np.random.default_rng(seed).permutation(n_pages)]

    def pool(rows, val):
        return torch.full((n_pages + 2 * guard, G, rows, D), val, dtype=dt, device="cuda")[guard:guard + n_pages]

    Kc, K, V = pool(PAGE // 16, BIG), pool(PAGE, BIG), pool(PAGE, -BIG)
    table = [[perm[-1]] * max_pages for _ in slots]  # entries nobody needs: a spare page -- valid, poisoned
    k = 0
    for i, (s, o) in enumerate(zip(slots, own)):
        nc = ncmp(o - 1) if o else 0
        for j in range(need[i]):
            p = table[i][j] = perm[k]
            k += 1
            r, rc = min(PAGE, o - PAGE * j), min(PAGE // 16, nc - 64 * j)
            K[p, :, :r] = c["K"][s, :, PAGE * j:PAGE * j + r]
            V[p, :, :r] = c["V"][s, :, PAGE * j:PAGE * j + r]
            if rc > 0:
                Kc[p, :, :rc] = c["Kc"][s, :, 64 * j:64 * j + rc]
    return dict(Kc=Kc, K=K, V=V, table=table, max_pages=max_pages, n_pages=n_pages)


def pools_of(c):
    """the pools of a case, scattered once and never modified"""
    if "pools" not in c:
        c["pools"] = scatter(c, seed=len(c["t_pos"]) + c["S"])
    return c["pools"]


def ragged_ref(nv, c):
    """nsa_sel_decode_ragged on the contiguous caches, once per case"""
    if "ragged" not in c["refs"]:
        c["refs"]["ragged"] = ragged(nv, c)
    return c["refs"]["ragged"]


def paged(nv, c, pl, table=None, **kw):
    tb = torch.tensor(pl["table"] if table is None else table, dtype=torch.int32, device="cuda")
    kw.setdefault("t_max", c["t_max"])
    return nv.selection_decode_paged(kw.pop("Q", c["Q"]), pl["Kc"], pl["K"], pl["V"], tb, kw.pop("meta", c["meta"]), N_TOP, kw.pop("pos", c["pos"]), **kw)


EDGES = dict(t_pos=[1022, 1023, 1024, 2047, 2048], S=3)  # rows at the last / first token of a page, S rows across two pages, forced blocks in two pages
PAGED_CASES = [CASES[IDS.index(i)] for i in ("S1_mixed", "S3_boundaries", "form1", "B33_waves8", "d128", "f16", "h1")] + [EDGES]
PAGED_IDS = ["S1_mixed", "S3_boundaries", "form1", "B33_waves8", "d128", "f16", "h1", "page_edges"]


@pytest.mark.parametrize("case", PAGED_CASES, ids=PAGED_IDS)
def test_paged_equals_ragged_bit_for_bit(nv, case):
    """pages in a random order == the contiguous caches: torch.equal on O and on ranges; ONE launch in the ragged call's form"""
    c = make_case(nv, **case)
    pl = pools_of(c)
    m = c["meta"]
    p = nv.selection_decode_paged_plan(c["B"], c["S"], G, c["h"], c["D"], c["D"], m.S_cmp, m.S_sel, pl["max_pages"], N_TOP, c["t_max"], c["dtype"])
    assert p["launches"] == 1 and p == ragged_plan(nv, c), p
    assert p["form"] == (1 if c["t_max"] > 32768 else 0), p
    O, rg = paged(nv, c, pl)
    O1, r1 = ragged_ref(nv, c)
    torch.cuda.synchronize()
    assert torch.isfinite(O.float()).all()
    assert torch.equal(rg, r1)
    assert torch.equal(O, O1)


def test_identity_table_over_a_reshaped_contiguous_cache(nv):
    """B = 1, a contiguous cache whose capacity is a multiple of 1024 seen as pages in place (table 0, 1): selection_decode_rows(t0) bit for bit"""
    t0, S, D, h, cap = 1052, 4, 64, 6, 2 * PAGE
    rng = np.random.default_rng([t0, S, cap])
    n_tok = t0 + S
    m = nv.build_block_meta(n_tok, L, D_, L_SEL, N_TOP, W)
    Q = dev(rng.standard_normal((1, S, G, h, D), dtype=np.float32), torch.bfloat16)
    Kc = rng.standard_normal((1, G, cap // 16, D), dtype=np.float32)
    K = rng.standard_normal((1, G, cap, D), dtype=np.float32)
    V = rng.standard_normal((1, G, cap, D), dtype=np.float32)
    K[:, :, n_tok:], V[:, :, n_tok:], Kc[:, :, m.S_cmp:] = BIG, -BIG, BIG
    Kc, K, V = dev(Kc, torch.bfloat16), dev(K, torch.bfloat16), dev(V, torch.bfloat16)
    as_pages = lambda X, rows: X[0].view(G, cap // PAGE, rows, D).permute(1, 0, 2, 3)  # noqa: E731  ([pages, G, rows, D], no copy)
    table = torch.tensor([[0, 1]], dtype=torch.int32, device="cuda")
    O, rg = nv.selection_decode_paged(Q, as_pages(Kc, 64), as_pages(K, PAGE), as_pages(V, PAGE), table, m, N_TOP, [t0])
    O1, r1 = nv.selection_decode_rows(Q, Kc[:, :, :m.S_cmp], K[:, :, :n_tok], V[:, :, :n_tok], m, N_TOP, t0)
    torch.cuda.synchronize()
    assert torch.equal(rg, r1) and torch.equal(O, O1)


@pytest.mark.parametrize("S", [1, 2])
def test_inactive_slots(nv, S):
    """a slot is inactive -- all-zero O and ranges -- with t_pos = -1, t_pos + S - 1 > t_max, t_pos + S - 1 >= max_pages * 1024, a needed
    table entry equal to n_pages and one equal to -1; the other slots keep their bits.  The pools are views that start one page into a
    larger allocation and end one page before its end, and the smaller n_pages is passed: even an unguarded kernel stays inside it"""
    base = make_case(nv, [1055, 40, 1190, 9], S)
    O_ref, r_ref = ragged_ref(nv, base)
    sel = [0, 0, 2, 0, 0, 1, 3]  # the inputs of slot b are those of sequence sel[b] of the base case
    pl = scatter(base, slots=sel, seed=7 + S, guard=1)
    assert pl["max_pages"] == 3
    m = nv.build_block_meta(3 * PAGE, L, D_, L_SEL, N_TOP, W)  # (at least the tokens of min(t_max, capacity - 1) + 1 in every call below)
    table = [row[:] for row in pl["table"]]
    table[3][1] = pl["n_pages"]  # the second page of a sequence at 1055: one past the pools
    table[4][0] = -1
    Q = base["Q"][sel].contiguous()
    # (max_pages, t_max, the position of slot 2): past the capacity of two pages; past t_max
    for max_pages, t_max, bad in ((2, 2100, 2 * PAGE - S + 1), (3, 1100, 1100 - S + 2)):
        pos = torch.tensor([1055, -1, bad, 1055, 1055, 40, 9], dtype=torch.int32, device="cuda")
        O = torch.ones((len(sel), S, G, base["h"], base["D"]), dtype=base["dtype"], device="cuda")
        rg = torch.ones((len(sel), S, G, N_TOP, 2), dtype=torch.int32, device="cuda")
        paged(nv, base, pl, table=[row[:max_pages] for row in table], Q=Q, meta=m, pos=pos, t_max=t_max, out=O, ranges_out=rg)
        torch.cuda.synchronize()
        for b in (1, 2, 3, 4):
            assert not O[b].any() and not rg[b].any(), (max_pages, t_max, b)
        for b in (0, 5, 6):
            assert torch.equal(O[b], O_ref[sel[b]]) and torch.equal(rg[b], r_ref[sel[b]]), (max_pages, t_max, b)


def test_pool_beyond_2_gib(nv):
    """pools that start 4 GiB into 7 GiB buffers, the case's pages at pool indices >= 8192 (a page of K is 256 KiB at D = 64, G = 2: byte
    offsets of 2 GiB and more), and +-3e4 where a sign-wrapped 32-bit offset would land (buffer + 2 .. 3 GiB): a wrong offset width reads
    poison inside the allocation.  The compressed pool gets the same page stride.  Equal to the ragged call bit for bit"""
    c = make_case(nv, [1055, 2100], 1)
    D, dt, GiB = c["D"], c["dtype"], 1 << 30
    n_pages, first, ps = 12288, 8192, G * PAGE * D
    src = scatter(c, seed=11, spare=1)

    def big_pool(rows, val):
        flat = torch.empty(7 * GiB, dtype=torch.uint8, device="cuda").view(dt)
        flat[GiB:3 * GiB // 2].fill_(val)  # bytes + 2 GiB .. + 3 GiB
        return torch.as_strided(flat, (n_pages, G, rows, D), (ps, rows * D, D, 1), 2 * GiB)

    Kc, K, V = big_pool(PAGE // 16, BIG), big_pool(PAGE, BIG), big_pool(PAGE, -BIG)
    assert K.stride(0) * 2 * first == 2 * GiB and K.data_ptr() - K.untyped_storage().data_ptr() == 4 * GiB
    for dst, s in ((Kc, src["Kc"]), (K, src["K"]), (V, src["V"])):
        dst[first:first + src["n_pages"]] = s  # (the spare page, poisoned, comes along: the table entries nobody needs point at it)
    O, rg = paged(nv, c, dict(Kc=Kc, K=K, V=V), table=[[first + p for p in row] for row in src["table"]])
    O1, r1 = ragged_ref(nv, c)
    torch.cuda.synchronize()
    assert torch.equal(rg, r1) and torch.equal(O, O1)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], EDGES], ids=["S1_mixed", "form1", "page_edges"])
def test_paged_run_to_run(nv, case):
    c = make_case(nv, **case)
    O, rg = paged(nv, c, pools_of(c))
    O2, rg2 = paged(nv, c, pools_of(c))
    torch.cuda.synchronize()
    assert torch.equal(O, O2) and torch.equal(rg, rg2)


def test_existing_entry_points_keep_their_bits(nv):
    """selection_decode_ragged at equal positions and selection_decode_rows(t0) on the same buffers are still bit-equal to each other"""
    t0 = 1052
    c = make_case(nv, [t0] * 3, 8)
    O, rg = ragged_ref(nv, c)
    O1, r1 = nv.selection_decode_rows(c["Q"], c["Kc"], c["K"], c["V"], c["meta"], N_TOP, t0)
    torch.cuda.synchronize()
    assert torch.equal(rg, r1) and torch.equal(O, O1)
