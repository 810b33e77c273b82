"""GPU parity: the decode step of the whole layer for a RAGGED batch -- every sequence at its own position, read on the device
(nsa_layer_decode_ragged, NSAAttention.decode_ragged).

The reference of every comparison is existing code only, never the call under test.  Caches come from B = 1 prefills, copied into the
slots of a pool by plain tensor indexing.  Expected results come from the existing nsa_layer_decode_rows on a REPLICA batch: sequence b's
slab and tokens copied into all B slots, the call run at t0 = t_pos[b], slot b read.  The replica has the same B S rows, so it takes the
same projection form, waves per row and band split count.  Rows of a slab beyond its own sequence are nobody's: NSA_KV allocates with
torch.empty.  The pools here hold NaN there (a finite sentinel in the guards test, which compares whole slabs), so a kernel that lets
such a row into its arithmetic -- even under a zero weight -- fails the finiteness and parity assertions.  Slabs are compared as bits.

Figures seen on the MI355X are printed by every comparison (pytest -s)."""
import ctypes

import pytest
import torch

from test_hip_extend import _clone_kv
from test_hip_gate import ULP1
from test_hip_layer_decode_rows import case, module, ncmp, rows_cabi
from test_hip_selection import norm

pytestmark = pytest.mark.gpu

CACHES = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp")
TOKEN_CACHES = CACHES[:6]


def ragged_cabi(m, x, kv, t_pos, t_max):
    """one nsa_layer_decode_ragged call through the C ABI on the pool kv (modified in place) -> y, ranges, gates"""
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _stream

    B, S, _ = x.shape
    L, dev = _lib.lib(), x.device
    desc, _ = m._layer_desc()
    kd = kv.native_desc()
    te = min(t_max, kd.S_max - 1)
    kv.refresh_meta(te + 1)
    meta = kv.meta
    assert m.decode_ragged_plan(B, S, kd.S_max, t_max, int(meta.S_sel))["route"] == 1
    ranges = torch.full((B, S, m.n_kv_groups, m.n_sel, 2), -7, dtype=torch.int32, device=dev)
    gates = torch.full((B, S, m.n_kv_groups, 3), float("nan"), dtype=torch.float32, device=dev)
    y = torch.full((B, S, m.dim), float("nan"), dtype=x.dtype, device=dev)
    nb = L.nsa_layer_decode_ragged_workspace(ctypes.byref(desc), B, S, kd.S_max)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
    wptr = (ws.data_ptr() + 255) & ~255
    cptr, crows, cvals = meta.device_csc(dev)
    xc = x.contiguous()
    rc = L.nsa_layer_decode_ragged(ctypes.byref(desc), ctypes.byref(kd), xc.data_ptr(), y.data_ptr(), t_pos.data_ptr(), t_max, S, cptr.data_ptr(),
                                   crows.data_ptr(), cvals.data_ptr(), int(meta.S_sel), ranges.data_ptr(), gates.data_ptr(), wptr, nb, _stream(dev))
    _lib.check(rc, "nsa_layer_decode_ragged")
    torch.cuda.synchronize()
    return y, ranges, gates


# ---- sequences: a B = 1 prefill each, built once per (module, length) and never modified ------------------------------------------------------
_MODS, _SEQS = {}, {}


def mod(name):
    if name not in _MODS:
        _MODS[name] = case("m7c", 3, 1052, 8)["m"] if name == "m7c" else module(dim=1536, H=12, G=2, D=128)
    return _MODS[name]


def seq(name, length, cap):
    """(x [1, length + 16, dim], the cache of capacity cap holding x[:, :length]: a plain prefill on a fresh cache)"""
    key = (name, length, cap)
    if key not in _SEQS:
        m = mod(name)
        dtype = m.W_Q.weight.dtype
        torch.manual_seed(7000 + length)
        x = torch.randn(1, length + 16, m.dim, device="cuda").to(dtype)
        kv = m.new_kv(1, cap, "cuda", dtype)
        if length:
            with torch.no_grad():
                m(x[:, :length], kv, prefill=True)
        assert kv._K_sel.shape[2] == cap and kv.t == length
        torch.cuda.synchronize()
        _SEQS[key] = (x, kv)
    return _SEQS[key]


def pool_of(name, positions, cap, S, steps=1, fill=None):
    """a pool with sequence b (of t_pos[b] tokens) in slot b, and the tokens x [B, steps S, dim] of its next rows.  A slot without a sequence
    (negative position) or `fill`-ed slots keep the fill pattern; their x rows are random.  fill = None: every row that belongs to no
    sequence holds NaN"""
    m = mod(name)
    dtype = m.W_Q.weight.dtype
    B = len(positions)
    kv = m.new_kv(B, cap, "cuda", dtype)
    for c in CACHES:
        buf = getattr(kv, c)
        if fill is None:
            buf.fill_(float("nan"))
        else:  # a finite pattern that differs from row to row and column to column
            n = buf.numel()
            buf.copy_(((torch.arange(n, device="cuda") % 251).float() / 64 - 2).to(dtype).view_as(buf))
    torch.manual_seed(99)
    x = torch.randn(B, steps * S, m.dim, device="cuda").to(dtype)
    for b, p in enumerate(positions):
        if p < 0 or p + steps * S > cap or (fill is not None and b in fill):
            continue
        xs, kvs = seq(name, p, cap)
        for c in TOKEN_CACHES:
            getattr(kv, c)[b, :, :p] = getattr(kvs, c)[0, :, :p]
        for c in CACHES[6:]:
            getattr(kv, c)[b, :, :ncmp(p)] = getattr(kvs, c)[0, :, :ncmp(p)]
        x[b] = xs[0, p:p + steps * S]
    torch.cuda.synchronize()
    return m, kv, x


def replica(m, pool, x, b, p, S, steps=1):
    """the existing rows call on a batch whose B slots all hold slot b of `pool` (as it is now) and its tokens -> per step (y, ranges,
    gates) of slot b, and the replica cache"""
    B = pool.B
    rep = m.new_kv(B, pool._K_sel.shape[2], "cuda", pool._K_sel.dtype)
    for c in CACHES:
        getattr(rep, c)[:] = getattr(pool, c)[b:b + 1]
    rep.t, rep.n_cmp = p, ncmp(p)
    outs = []
    for k in range(steps):
        xr = x[b:b + 1, k * S:(k + 1) * S].expand(B, S, m.dim).contiguous()
        y, r, g, _ = rows_cabi(m, xr, rep)
        outs.append((y[b].clone(), r[b].clone(), g[b].clone()))
    return outs, rep


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    """equal as stored, NaN rows included"""
    return torch.equal(bits(a), bits(b))


def live(p, S, te):
    return p >= 0 and p + S - 1 <= te


def check_against_replicas(tag, m, before, after, x, positions, S, te, outs, steps=1):
    """before / after: the pool before the first and after the last of `steps` ragged calls; outs: per step (y, ranges, gates) of the calls.
    Per live sequence against its replica: appended cache rows and pooled tokens bit-equal, ranges equal, y and gates within their bars;
    every other row of every slab -- old rows, padding slots, slots beyond the bound -- as before the call, bit for bit."""
    dtype = before._K_sel.dtype
    expect = _clone_kv(before)
    ey, eg = 0.0, 0.0
    for b, p in enumerate(positions):
        if not live(p, steps * S, te):
            for k in range(steps):
                y, r, _ = outs[k]
                assert torch.count_nonzero(y[b]) == 0 and torch.count_nonzero(r[b]) == 0, (tag, b, "an inactive slot's y and ranges rows are zero")
            continue
        ref, rep = replica(m, before, x, b, p, S, steps)
        for c in TOKEN_CACHES:
            getattr(expect, c)[b, :, p:p + steps * S] = getattr(rep, c)[b, :, p:p + steps * S]
        for c in CACHES[6:]:
            getattr(expect, c)[b, :, ncmp(p):ncmp(p + steps * S)] = getattr(rep, c)[b, :, ncmp(p):ncmp(p + steps * S)]
        for k in range(steps):
            y, r, g = outs[k]
            yr, rr, gr = ref[k]
            assert norm(r[b].cpu().numpy()) == norm(rr.cpu().numpy()), (tag, b, k, "ranges")
            bar = 1e-2 * max(1.0, yr.float().abs().max().item())
            err = (y[b].float() - yr.float()).abs().max().item()
            assert torch.isfinite(y[b].float()).all() and err <= bar, (tag, b, k, err, bar)
            dg = (g[b] - gr).abs().max().item()
            assert dg <= ULP1[dtype] + 1e-7, (tag, b, k, dg)
            ey, eg = max(ey, err), max(eg, dg)
    print(f"{tag}: max|y - replica| {ey:.3e} (bar 1e-2 max(1, max|ref|)), max|gates - replica| {eg:.3e} (bar {ULP1[dtype] + 1e-7:.3e})")
    for c in CACHES:
        assert same_bits(getattr(after, c), getattr(expect, c)), (tag, c, "appended rows and pooled tokens as the replicas', every other row untouched")


# ---- 1. equal positions: the rows call's bits ---------------------------------------------------------------------------------------------
def test_equal_positions_bit_for_bit():
    c = case("m7c", 3, 1052, 8)
    m, t0, S = c["m"], c["t0"], c["S"]
    ref = _clone_kv(c["kv0"])
    y_r, r_r, g_r, plan = rows_cabi(m, c["xn"], ref)
    assert plan == {"launches": 6, "route": 1}
    kv = _clone_kv(c["kv0"])
    t_pos = torch.tensor([t0] * 3, dtype=torch.int32, device="cuda")
    y, r, g = ragged_cabi(m, c["xn"], kv, t_pos, t0 + S - 1)
    assert ncmp(t0) == 64 and ncmp(t0 + S) == 65  # a compressed token is emitted inside the call
    for name in TOKEN_CACHES:
        assert torch.equal(getattr(kv, name)[:, :, t0:t0 + S], getattr(ref, name)[:, :, t0:t0 + S]), name
        assert torch.equal(getattr(kv, name)[:, :, :t0], getattr(c["kv0"], name)[:, :, :t0]), name
    for name in ("_K_cmp", "_V_cmp"):
        assert torch.equal(getattr(kv, name)[:, :, 64:65], getattr(ref, name)[:, :, 64:65]), name
        assert torch.equal(getattr(kv, name)[:, :, :64], getattr(c["kv0"], name)[:, :, :64]), name
    for s in range(S):
        assert norm(r[:, s].cpu().numpy()) == norm(r_r[:, s].cpu().numpy()), s
    assert torch.equal(g, g_r) and torch.equal(y, y_r)
    assert (kv.t, kv.n_cmp) == (t0, 64)  # the pool's own length is not the call's business


# ---- 2. mixed positions -------------------------------------------------------------------------------------------------------------------
MIXED = dict(positions=[1052, 1056, 28, 0, -1], cap=1072, S=8, t_max=1063)
_MIXED = {}


def mixed():
    """test 2's pool, tokens, and its one ragged call through the C ABI: shared with the module test, never modified"""
    if not _MIXED:
        m, kv, x = pool_of("m7c", MIXED["positions"], MIXED["cap"], MIXED["S"])
        after = _clone_kv(kv)
        t_pos = torch.tensor(MIXED["positions"], dtype=torch.int32, device="cuda")
        y, r, g = ragged_cabi(m, x, after, t_pos, MIXED["t_max"])
        _MIXED.update(m=m, before=kv, x=x, after=after, y=y, r=r, g=g, t_pos=t_pos)
    return _MIXED


def test_mixed_positions():
    """a token emitted inside the call (1052), none due (1056), the first compressed token appearing mid-call with rows before it having
    none (28), an empty cache (0) and a padding slot (-1)"""
    M = mixed()
    check_against_replicas("mixed", M["m"], M["before"], M["after"], M["x"], MIXED["positions"], MIXED["S"], MIXED["t_max"], [(M["y"], M["r"], M["g"])])


# ---- 3. guards: nothing is written for a sequence that is not live ---------------------------------------------------------------------------
def test_guards_leave_inactive_slabs_untouched():
    cap, S, t_max = 1072, 8, 1063
    positions = [cap - 3, -1, 1052, 1068]  # slot 0: its last rows lie beyond the buffers (a missing guard would write into slot 1's slab, where
    # the comparison below sees it -- never outside the allocation); slot 1: padding; slot 3: beyond t_max
    m, kv, x = pool_of("m7c", positions, cap, S, fill={0, 1, 3})
    before = _clone_kv(kv)
    t_pos = torch.tensor(positions, dtype=torch.int32, device="cuda")
    y, r, g = ragged_cabi(m, x, kv, t_pos, t_max)
    for b in (0, 1, 3):
        for c in CACHES:
            assert same_bits(getattr(kv, c)[b], getattr(before, c)[b]), (b, c)
        assert torch.count_nonzero(y[b]) == 0 and torch.count_nonzero(r[b]) == 0, b
    check_against_replicas("guards", m, before, kv, x, positions, S, t_max, [(y, r, g)])


# ---- 4. two steps with identical arguments, the positions advanced on the device ---------------------------------------------------------------
def test_two_steps_device_advanced():
    positions, cap, S = [1040, 77, 300], 1072, 4
    t_max = max(positions) + 2 * S - 1
    m, kv, x = pool_of("m7c", positions, cap, S, steps=2)
    before = _clone_kv(kv)
    t_pos = torch.tensor(positions, dtype=torch.int32, device="cuda")
    outs = [ragged_cabi(m, x[:, :S], kv, t_pos, t_max)]
    t_pos += S  # on the device: the second call's arguments are the first one's
    outs.append(ragged_cabi(m, x[:, S:], kv, t_pos, t_max))
    assert ncmp(77) == 3 and ncmp(81) == 4 and ncmp(300) == 17 and ncmp(304) == 18  # the second step reads the token the first one pooled
    check_against_replicas("two steps", m, before, kv, x, positions, S, t_max, outs, steps=2)


# ---- 5. D = 128: one ragged launch per band branch, the gate kernel ----------------------------------------------------------------------------
def test_d128():
    positions, cap, S, t_max = [300, 77, -1], 320, 4, 303
    m, kv, x = pool_of("d128", positions, cap, S)
    before = _clone_kv(kv)
    assert m.decode_ragged_plan(3, S, cap, t_max, 5) == {"launches": 7, "route": 1}
    y, r, g = ragged_cabi(m, x, kv, torch.tensor(positions, dtype=torch.int32, device="cuda"), t_max)
    check_against_replicas("D128", m, before, kv, x, positions, S, t_max, [(y, r, g)])


# ---- 6. the module ---------------------------------------------------------------------------------------------------------------------------
def test_module_device_positions_equal_the_cabi_call():
    M = mixed()
    m, S = M["m"], MIXED["S"]
    kv = _clone_kv(M["before"])
    kv.t, kv.n_cmp = 5, 0
    kv.append_reads(0, 5)
    state = (kv.t, kv.n_cmp, list(kv.reads_pred), list(kv.reads_act_total), list(kv.reads_act_sel), list(kv.reads_act_cmp), list(kv.reads_act_win))
    with torch.no_grad():
        y, kv2 = m.decode_ragged(M["x"], kv, M["t_pos"], t_max=MIXED["t_max"])
    torch.cuda.synchronize()
    assert kv2 is kv and tuple(y.shape) == (5, S, m.dim)
    assert tuple(m._last_ranges.shape) == (5, S, 2, 16, 2) and tuple(m._last_gates.shape) == (5, S, 2, 3)
    assert torch.equal(y, M["y"]) and torch.equal(m._last_ranges, M["r"]) and torch.equal(m._last_gates[:4], M["g"][:4])
    for c in CACHES:
        assert same_bits(getattr(kv, c), getattr(M["after"], c)), c
    assert (kv.t, kv.n_cmp, kv.reads_pred, kv.reads_act_total, kv.reads_act_sel, kv.reads_act_cmp, kv.reads_act_win) == state
    with pytest.raises(RuntimeError, match="inference only"):
        m.decode_ragged(M["x"].clone().requires_grad_(), kv, M["t_pos"], t_max=MIXED["t_max"])


def test_module_per_sequence_route_when_the_plan_declines():
    from nsa_vibe_amd import _lib

    M = mixed()
    m, S, te = M["m"], MIXED["S"], MIXED["t_max"]
    kv = _clone_kv(M["before"])
    saved = _lib.get_tuning("DECODE_UNFUSED")
    _lib.set_tuning("DECODE_UNFUSED", 1)  # the ragged call declines: no one-launch selected branch
    try:
        assert m.decode_ragged_plan(5, S, MIXED["cap"], te, 17)["route"] == -1
        with torch.no_grad():
            y, _ = m.decode_ragged(M["x"], kv, MIXED["positions"])  # host positions: one decode_rows per live sequence, on its slab
            r, g = m._last_ranges.clone(), m._last_gates.clone()
            with pytest.raises(RuntimeError, match="DECODE_UNFUSED = 1"):
                m.decode_ragged(M["x"], kv, M["t_pos"], t_max=te)  # device positions: the native message
    finally:
        _lib.set_tuning("DECODE_UNFUSED", saved)
    torch.cuda.synchronize()
    assert (kv.t, kv.n_cmp) == (0, 0)
    # test 2's bars, against the one native call (itself held to the replicas there): y and gates of the live slots, equal ranges, zero padding
    dtype = y.dtype
    ey = eg = 0.0
    for b, p in enumerate(MIXED["positions"]):
        if not live(p, S, te):
            assert torch.count_nonzero(y[b]) == 0 and torch.count_nonzero(r[b]) == 0
            continue
        ref = replica(m, M["before"], M["x"], b, p, S)[0][0]
        assert norm(r[b].cpu().numpy()) == norm(ref[1].cpu().numpy()), b
        bar = 1e-2 * max(1.0, ref[0].float().abs().max().item())
        err = (y[b].float() - ref[0].float()).abs().max().item()
        dg = (g[b] - ref[2]).abs().max().item()
        assert err <= bar and dg <= ULP1[dtype] + 1e-7, (b, err, bar, dg)
        ey, eg = max(ey, err), max(eg, dg)
        # the appended rows and the pooled tokens landed in the pool's slab, through the view.  Not bit for bit, as in test 2: the B = 1
        # call projects its S rows on another form than the B S rows of the ragged call (another summation order), so a cached value is the
        # same dot product of up to 768 bf16 terms rounded once more: the bar is test_hip_extend.py's for cached rows, 1e-2 max(1, max|ref|)
        for c, lo, hi in [(c, p, p + S) for c in TOKEN_CACHES] + [(c, ncmp(p), ncmp(p + S)) for c in CACHES[6:]]:
            got, want = getattr(kv, c)[b, :, lo:hi].float(), getattr(M["after"], c)[b, :, lo:hi].float()
            assert torch.isfinite(got).all() and (hi == lo or (got - want).abs().max().item() <= 1e-2 * max(1.0, want.abs().max().item())), (b, c)
    print(f"per-sequence route: max|y - replica| {ey:.3e}, max|gates - replica| {eg:.3e}")


# ---- 7. a bound below S - 1: no sequence can be live, every row is a zero row ----------------------------------------------------------------
def test_bound_below_the_rows_gives_zero_rows():
    positions, cap, S, t_max = [0, -1, 0], 1072, 8, 3  # 0 + 7 > 3: the bound leaves nobody live
    m, kv, x = pool_of("m7c", positions, cap, S)
    before = _clone_kv(kv)
    y, r, _ = ragged_cabi(m, x, kv, torch.tensor(positions, dtype=torch.int32, device="cuda"), t_max)
    assert torch.count_nonzero(y) == 0 and torch.count_nonzero(r) == 0
    for c in CACHES:
        assert same_bits(getattr(kv, c), getattr(before, c)), c
