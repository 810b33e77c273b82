"""GPU parity: the ragged layer decode over PAGED caches (nsa_layer_decode_paged, NSAAttention.decode_paged, NSA_PagedKV).

Every expectation comes from the existing nsa_layer_decode_ragged on contiguous slabs: sequences are B = 1 prefills copied into the slabs of
a pool (test_hip_layer_decode_ragged.pool_of), the ragged call runs on a clone of the slabs, and the same slabs -- as they were BEFORE the
call -- are scattered into pages.  The paged call must append the ragged call's rows and pool its compressed rows bit for bit, select its
ranges, and leave every other row of every page as it was.

Poison: the pools are filled with a pattern of NaN, +3e4 and -3e4 before the sequences go in, so every page that belongs to nobody, every
row of a sequence's last page beyond its tokens, and the page that unneeded table entries point at (a valid page of the pools) hold it.  A
kernel that lets such a row into its arithmetic, even under a zero weight, fails the finiteness and parity assertions; a stray store shows
up in the whole-pool comparison (with `guard`, in the guard pages around the pools instead of outside the allocation).

Bars.  Cache rows, ranges: equal bits.  y at D = 64: 1e-2 max(1, max|ref|), the project's bar -- not zero because the ragged layer merges
the band branches' splits in its finish kernel while the paged call combines per branch; gates: test_hip_layer_decode_ragged's bar.  At
D = 128 both layers run one band launch per branch and the gate kernel: everything is torch.equal.  Figures are printed (pytest -s); seen
on the MI355X at these shapes: max|y - ragged| = 0 and max|gates - ragged| = 0 at D = 64 as well, bf16 and f16."""
import ctypes
import random

import pytest
import torch

from test_hip_extend import _clone_kv
from test_hip_gate import ULP1
from test_hip_layer_decode_ragged import CACHES, _MODS, mod, pool_of, ragged_cabi, same_bits, seq
from test_hip_layer_decode_rows import module, ncmp
from test_hip_selection import norm

pytestmark = pytest.mark.gpu

PAGE, CPAGE = 1024, 64
MAX_PAGES, CAP = 2, 2048
# 1022: rows 1022-1025 across two pages; 1036: emits j = 63 (window 1008-1039 straddles pages) into the last row of compressed page 0;
# 1052: emits j = 64 into row 0 of compressed page 1; 28: emits j = 0; 0: the first token; -1: a padding slot
POSITIONS, S, T_MAX = [1022, 1036, 1052, 28, 0, -1], 4, 1055


def model(name):
    if name == "f16" and name not in _MODS:
        _MODS[name] = module(dtype=torch.float16)
    return mod(name)


def rows_of(name):
    return CPAGE if name in ("_K_cmp", "_V_cmp") else PAGE


def poison(t):
    """NaN, +3e4, -3e4 in turn"""
    n = t.numel()
    i = torch.arange(n, device=t.device) % 3
    v = torch.where(i == 0, torch.full((n,), float("nan"), device=t.device), torch.where(i == 1, torch.full((n,), 3e4, device=t.device),
                                                                                         torch.full((n,), -3e4, device=t.device)))
    t.copy_(v.to(t.dtype).view_as(t))


def paged_of(m, slabs, positions, rows, n_pages=12, order=None, guard=False, bad=None):
    """slabs (an NSA_KV pool BEFORE the call, sequence b of positions[b] tokens in slab b) scattered into a poisoned NSA_PagedKV: sequence b
    gets the pages its `rows` new rows need, in the order of the page ids (`order`: a seed, None = ascending); every other entry points at a
    poisoned page nobody owns.  bad: {(b, j): value} entries overwritten afterwards.  guard: every pool is a view one page inside a larger
    allocation (pkv.big).  -> pkv; pkv.assigned[b] = the pages of sequence b"""
    B = len(positions)
    dtype = slabs._K_sel.dtype
    pkv = m.new_paged_kv(n_pages, B, MAX_PAGES, "cuda", dtype)
    pkv.big = {}
    for name in CACHES:
        pool = getattr(pkv, name)
        if guard:
            big = torch.empty((n_pages + 2,) + tuple(pool.shape[1:]), device="cuda", dtype=dtype)
            poison(big)
            pkv.big[name] = big
            setattr(pkv, name, big[1:-1])
        else:
            poison(pool)
    pkv._native.clear()
    ids = list(range(n_pages))
    if order is not None:
        random.Random(order).shuffle(ids)
    junk = ids.pop()
    table = [[junk] * MAX_PAGES for _ in range(B)]
    pkv.assigned = []
    for b, p in enumerate(positions):
        need = 0 if p < 0 or p + rows > CAP else ((p + rows - 1) >> 10) + 1
        pages = [ids.pop(0) for _ in range(need)]
        pkv.assigned.append(pages)
        table[b][:need] = pages
        for name in CACHES:
            r = rows_of(name)
            n = 0 if need == 0 else (ncmp(p) if r == CPAGE else p)
            for j in range((n + r - 1) // r):
                k = min(r, n - j * r)
                getattr(pkv, name)[pages[j], :, :k] = getattr(slabs, name)[b, :, j * r:j * r + k]
    for (b, j), v in (bad or {}).items():
        table[b][j] = v
    pkv.block_table.copy_(torch.tensor(table, dtype=torch.int32))
    pkv.table = table
    torch.cuda.synchronize()
    return pkv


def pools(pkv):
    return {name: (pkv.big[name] if pkv.big else getattr(pkv, name)).clone() for name in CACHES}


def paged_cabi(m, x, pkv, t_pos, t_max):
    """one nsa_layer_decode_paged call through the C ABI on pkv (modified in place) -> y, ranges, gates"""
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _stream

    B, S_, _ = x.shape
    L, dev = _lib.lib(), x.device
    desc, _ = m._layer_desc()
    kd = pkv.native_desc()
    te = min(t_max, kd.max_pages * PAGE - 1)
    pkv.refresh_meta(te + 1)
    meta = pkv.meta
    assert m.decode_paged_plan(B, S_, kd.max_pages, t_max, int(meta.S_sel)) == {"launches": 10, "route": 1}
    ranges = torch.full((B, S_, m.n_kv_groups, m.n_sel, 2), -7, dtype=torch.int32, device=dev)
    gates = torch.full((B, S_, m.n_kv_groups, 3), float("nan"), dtype=torch.float32, device=dev)
    y = torch.full((B, S_, m.dim), float("nan"), dtype=x.dtype, device=dev)
    nb = L.nsa_layer_decode_paged_workspace(ctypes.byref(desc), B, S_, kd.max_pages)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
    wptr = (ws.data_ptr() + 255) & ~255
    cptr, crows, cvals = meta.device_csc(dev)
    xc = x.contiguous()
    rc = L.nsa_layer_decode_paged(ctypes.byref(desc), ctypes.byref(kd), xc.data_ptr(), y.data_ptr(), t_pos.data_ptr(), t_max, S_, cptr.data_ptr(),
                                  crows.data_ptr(), cvals.data_ptr(), int(meta.S_sel), ranges.data_ptr(), gates.data_ptr(), wptr, nb, _stream(dev))
    _lib.check(rc, "nsa_layer_decode_paged")
    torch.cuda.synchronize()
    return y, ranges, gates


def is_live(pkv, b, p, rows, te):
    """the verdict of the pre-pass, restated: the ragged rule, and every needed entry inside [0, n_pages)"""
    if p < 0 or p + rows - 1 > te:
        return False
    return all(0 <= pkv.table[b][j] < pkv.n_pages for j in range(((p + rows - 1) >> 10) + 1))


def expected_pools(pkv, before, slabs_after, positions, rows, te):
    """the pools before the call with, for every live sequence, the rows the ragged call appended and pooled on the slabs"""
    exp = {k: v.clone() for k, v in before.items()}
    off = 1 if pkv.big else 0
    for b, p in enumerate(positions):
        if not is_live(pkv, b, p, rows, te):
            continue
        for name in CACHES:
            r = rows_of(name)
            lo, hi = (ncmp(p), ncmp(p + rows)) if r == CPAGE else (p, p + rows)
            for row in range(lo, hi):
                exp[name][pkv.table[b][row // r] + off, :, row % r] = getattr(slabs_after, name)[b, :, row]
    return exp


def check(tag, m, pkv, before, slabs_after, positions, rows, te, got, ref, exact):
    """got / ref: (y, ranges, gates) of the paged call and of the ragged call on the slabs.  Live sequences: ranges equal, y and gates within
    their bars (exact: torch.equal); inactive ones: zero y and ranges rows.  All eight pools: the expected bits, guard pages included"""
    (y, r, g), (yr, rr, gr) = got, ref
    dtype = y.dtype
    ey = eg = 0.0
    for b, p in enumerate(positions):
        if not is_live(pkv, b, p, rows, te):
            assert torch.count_nonzero(y[b]) == 0 and torch.count_nonzero(r[b]) == 0, (tag, b, "an inactive slot's y and ranges rows are zero")
            continue
        assert torch.isfinite(y[b].float()).all() and torch.isfinite(g[b]).all(), (tag, b)
        assert norm(r[b].cpu().numpy()) == norm(rr[b].cpu().numpy()), (tag, b, "ranges")
        err = (y[b].float() - yr[b].float()).abs().max().item()
        dg = (g[b] - gr[b]).abs().max().item()
        ey, eg = max(ey, err), max(eg, dg)
        if exact:
            assert torch.equal(y[b], yr[b]) and torch.equal(g[b], gr[b]) and torch.equal(r[b], rr[b]), (tag, b, err, dg)
        else:
            bar = 1e-2 * max(1.0, yr[b].float().abs().max().item())
            assert err <= bar and dg <= ULP1[dtype] + 1e-7, (tag, b, err, bar, dg)
    print(f"{tag}: max|y - ragged| {ey:.3e} ({'torch.equal' if exact else 'bar 1e-2 max(1, max|ref|)'}), max|gates - ragged| {eg:.3e}")
    after = pools(pkv)
    exp = expected_pools(pkv, before, slabs_after, positions, rows, te)
    for name in CACHES:
        assert same_bits(after[name], exp[name]), (tag, name, "appended and pooled rows as the ragged call's, every other row of every page untouched")


# ---- the mixed batch: one ragged reference per model, one paged call per (model, table order); shared, never modified -----------------------
_REF, _RUN = {}, {}


def reference(name):
    if name not in _REF:
        m = model(name)
        _, slabs, x = pool_of(name, POSITIONS, CAP, S)
        after = _clone_kv(slabs)
        t_pos = torch.tensor(POSITIONS, dtype=torch.int32, device="cuda")
        _REF[name] = dict(m=m, slabs=slabs, x=x, after=after, t_pos=t_pos, out=ragged_cabi(m, x, after, t_pos, T_MAX))
    return _REF[name]


def mixed(name, order):
    if (name, order) not in _RUN:
        R = reference(name)
        pkv = paged_of(R["m"], R["slabs"], POSITIONS, S, order=order)
        before = pools(pkv)
        out = paged_cabi(R["m"], R["x"], pkv, R["t_pos"], T_MAX)
        _RUN[(name, order)] = dict(pkv=pkv, before=before, out=out)
    return _RUN[(name, order)]


def check_mixed(name, order, exact):
    R, P = reference(name), mixed(name, order)
    assert ncmp(1036) == 63 and ncmp(1040) == 64 and ncmp(1052) == 64 and ncmp(1056) == 65 and ncmp(28) == 0 and ncmp(32) == 1
    check(f"mixed {name} order {order}", R["m"], P["pkv"], P["before"], R["after"], POSITIONS, S, T_MAX, P["out"], R["out"], exact)


def test_mixed_positions_d64_bf16():
    check_mixed("m7c", 5, exact=False)


def test_mixed_positions_d128_bit_for_bit():
    check_mixed("d128", 5, exact=True)


def test_mixed_positions_f16():
    check_mixed("f16", 5, exact=False)


def test_table_order_does_not_change_a_bit():
    a, b = mixed("m7c", None), mixed("m7c", 5)
    assert a["pkv"].table != b["pkv"].table
    for u, v in zip(a["out"][:2], b["out"][:2]):
        assert torch.equal(u, v)
    assert torch.equal(a["out"][2][:5], b["out"][2][:5])  # (the gates of the padding slot are unspecified)


# ---- inactive sequences: zero rows and not one byte written, with the pools one page inside a larger allocation -----------------------------
@pytest.mark.parametrize("positions, t_max, bad, dead", [
    # slot 0: a needed entry of -1; 1: a needed entry of n_pages; 2: entry 0 bad while the position lies in page 1; 3: beyond t_max;
    # 4: live, with a bad entry BEHIND its last needed page; 5: padding
    ([1036, 28, 1052, 1060, 28, -1], 1055, {(0, 1): -1, (1, 0): 12, (2, 0): -1, (4, 1): -1}, [0, 1, 2, 3, 5]),
    # slot 0: beyond max_pages * 1024 (rows 2046 .. 2049) under a bound that allows it; 1: live, entry 1 = n_pages behind its needed page
    ([2046, 28, -1], 5000, {(1, 1): 12}, [0, 2]),
])
def test_inactive_sequences_write_nothing(positions, t_max, bad, dead):
    m = model("m7c")
    te = min(t_max, CAP - 1)
    _, slabs, x = pool_of("m7c", positions, CAP, S)
    slabs_after = _clone_kv(slabs)
    t_pos = torch.tensor(positions, dtype=torch.int32, device="cuda")
    ref = ragged_cabi(m, x, slabs_after, t_pos, t_max)
    pkv = paged_of(m, slabs, positions, S, order=9, guard=True, bad=bad)
    before = pools(pkv)
    got = paged_cabi(m, x, pkv, t_pos, t_max)
    assert [b for b, p in enumerate(positions) if not is_live(pkv, b, p, S, te)] == dead
    after = pools(pkv)
    for b in dead:
        assert torch.count_nonzero(got[0][b]) == 0 and torch.count_nonzero(got[1][b]) == 0, b
        for name in CACHES:  # its own pages, bit for bit
            for pg in pkv.assigned[b]:
                assert same_bits(after[name][pg + 1], before[name][pg + 1]), (b, name, pg)
    check(f"inactive t_max {t_max}", m, pkv, before, slabs_after, positions, S, te, got, ref, exact=False)


# ---- two steps with identical arguments, the positions advanced on the device: 1023 -> 1024 crosses into page 1 -----------------------------
def test_two_device_advanced_steps():
    positions, t_max = [1023, 1039, 31], 1040  # 1039 emits j = 63 in step 1, 31 emits j = 0 in step 1
    m = model("m7c")
    _, slabs, x = pool_of("m7c", positions, CAP, 1, steps=2)
    slabs_after = _clone_kv(slabs)
    pkv = paged_of(m, slabs, positions, 2, order=3)  # the pages of both steps assigned beforehand
    assert len(pkv.assigned[0]) == 2
    before = pools(pkv)
    t_ref = torch.tensor(positions, dtype=torch.int32, device="cuda")
    t_pos = t_ref.clone()
    outs = []
    for k in range(2):
        ref = ragged_cabi(m, x[:, k:k + 1], slabs_after, t_ref, t_max)
        got = paged_cabi(m, x[:, k:k + 1], pkv, t_pos, t_max)
        outs.append((got, ref))
        t_ref += 1
        t_pos += 1  # on the device: the second call's arguments are the first one's
    for k, (got, ref) in enumerate(outs):
        for b in range(3):
            assert norm(got[1][b].cpu().numpy()) == norm(ref[1][b].cpu().numpy()), (k, b)
            bar = 1e-2 * max(1.0, ref[0][b].float().abs().max().item())
            assert (got[0][b].float() - ref[0][b].float()).abs().max().item() <= bar, (k, b)
    after = pools(pkv)
    exp = expected_pools(pkv, before, slabs_after, positions, 2, t_max)
    for name in CACHES:
        assert same_bits(after[name], exp[name]), name


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
def clone_pkv(p):
    c = object.__new__(type(p))
    c.__dict__.update(p.__dict__)
    for name in CACHES:
        setattr(c, name, getattr(p, name).clone())
    c.block_table, c.pages, c._free, c._native = p.block_table.clone(), [list(v) for v in p.pages], list(p._free), {}
    return c


def test_module_route_equals_the_cabi_call():
    from nsa_vibe_amd import _lib

    m = model("m7c")
    R = reference("m7c")
    pkv = m.new_paged_kv(12, len(POSITIONS), MAX_PAGES, "cuda", torch.bfloat16)
    for name in CACHES:
        poison(getattr(pkv, name))
    assert int((pkv.block_table != -1).sum()) == 0
    for b, p in enumerate(POSITIONS):
        if p < 0:
            continue
        _, kv1 = seq("m7c", p, CAP)
        pkv.load_sequence(b, kv1, p)
        back = pkv.gather_sequence(b, p)  # the round trip, bit for bit
        for name in CACHES:
            n = ncmp(p) if name in CACHES[6:] else p
            assert torch.equal(getattr(back, name)[:, :, :n], getattr(kv1, name)[:, :, :n]), (b, name)
        pkv.ensure(b, p + S)
    twin = clone_pkv(pkv)
    y_c, r_c, g_c = paged_cabi(m, R["x"], twin, R["t_pos"], T_MAX)
    with torch.no_grad():
        y, out = m.decode_paged(R["x"], pkv, R["t_pos"], t_max=T_MAX)
    torch.cuda.synchronize()
    assert out is pkv and tuple(y.shape) == (6, S, m.dim)
    assert tuple(m._last_ranges.shape) == (6, S, 2, 16, 2) and tuple(m._last_gates.shape) == (6, S, 2, 3)
    assert torch.equal(y, y_c) and torch.equal(m._last_ranges, r_c) and torch.equal(m._last_gates[:5], g_c[:5])
    assert torch.equal(y, mixed("m7c", 5)["out"][0])  # and the poisoned, permuted pools of test 1 gave the same bits
    for name in CACHES:
        assert same_bits(getattr(pkv, name), getattr(twin, name)), name
    with pytest.raises(RuntimeError, match="inference only"):
        m.decode_paged(R["x"].clone().requires_grad_(), pkv, R["t_pos"], t_max=T_MAX)
    saved = _lib.get_tuning("DECODE_UNFUSED")
    _lib.set_tuning("DECODE_UNFUSED", 1)  # a declined shape: the library's message, no other route
    try:
        assert m.decode_paged_plan(6, S, MAX_PAGES, T_MAX, 17) == {"launches": 0, "route": -1}
        with torch.no_grad(), pytest.raises(RuntimeError, match="DECODE_UNFUSED = 1"):
            m.decode_paged(R["x"], pkv, R["t_pos"], t_max=T_MAX)
    finally:
        _lib.set_tuning("DECODE_UNFUSED", saved)
    for name in CACHES:  # the declined call wrote nothing
        assert same_bits(getattr(pkv, name), getattr(twin, name)), name
