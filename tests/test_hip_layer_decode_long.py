"""GPU parity: the ragged and the paged layer decode (NSAAttention.decode_ragged / decode_paged) on rows beyond the unsplit forms of the
selected branch -- switch DECODE_LONG = 1, the long-row form -- with every other launch of the layer as it is.

Caches come from B = 1 prefills copied into the slabs of a pool (test_hip_layer_decode_ragged.pool_of: rows that belong to no sequence
hold NaN).  The expectation of decode_ragged is existing code only: NSAAttention.decode_rows per live sequence on kv.sequence_view(b, t) of
a clone of the pool -- single layer steps where its own plan declines.  Ranges equal; the appended token rows and the pooled compressed
rows equal as bits; every other row of every slab untouched; y within the project's 1e-2 max(1, max|ref|); a padding slot's rows zero.
decode_paged on the same sequences loaded into pages: caches and ranges bit for bit those of the long decode_ragged, y at the bar of
tests/test_hip_layer_decode_paged.py for the head dimension (D = 64: 1e-2 max(1, max|ref|); D = 128: torch.equal).

Figures seen on the MI355X are printed by every comparison (pytest -s)."""
import pytest
import torch

from test_hip_extend import _clone_kv
from test_hip_layer_decode_ragged import CACHES, TOKEN_CACHES, live, mod, pool_of, same_bits
from test_hip_layer_decode_rows import ncmp
from test_hip_selection import norm

pytestmark = pytest.mark.gpu

# name -> (module, positions, S): D = 128 rows at 16 chunks (S = 1) and across 16 -> 17 chunks (S = 4: t = 16415 sees 1025 compressed
# tokens); m7c rows across 64 -> 65 chunks (t = 65567 sees 4097)
SHAPES = {
    "d128_S1": ("d128", [16413, 1052, -1], 1),
    "d128_S4": ("d128", [16413, 1052, -1], 4),
    "m7c_S4": ("m7c", [65565, 1052], 4),
}
_RUNS = {}


def run(name, tune):
    """the pool before the call, one long decode_ragged on a clone, the per-sequence expectation on another clone: once per shape"""
    tune("DECODE_LONG", 1)
    if name not in _RUNS:
        mname, positions, S = SHAPES[name]
        t_max = max(positions) + S - 1
        cap = (max(positions) + 16 + 63) // 64 * 64 + 64  # (one capacity per module: the S = 1 and S = 4 shapes share their prefills)
        m, before, x = pool_of(mname, positions, cap, S)
        B = len(positions)
        plan = m.decode_ragged_plan(B, S, cap, t_max, (t_max + 64) // 64)
        assert plan == m.decode_ragged_plan(B, S, 1072, 1052 + S - 1, 17) and plan["route"] == 1, plan  # the launch count of today's in-range plan
        after = _clone_kv(before)
        t_pos = torch.tensor(positions, dtype=torch.int32, device="cuda")
        with torch.no_grad():
            y, _ = m.decode_ragged(x, after, t_pos, t_max=t_max)
        r, g = m._last_ranges.clone(), m._last_gates.clone()
        torch.cuda.synchronize()
        # the expectation: decode_rows per live sequence on its slab of another clone
        exp = _clone_kv(before)
        ref = {}
        for b, p in enumerate(positions):
            if not live(p, S, t_max):
                continue
            with torch.no_grad():
                yb, _ = m.decode_rows(x[b:b + 1], exp.sequence_view(b, p))
            ref[b] = (yb[0].clone(), m._last_ranges.reshape(1, S, m.n_kv_groups, m.n_sel, 2)[0].clone())
        torch.cuda.synchronize()
        _RUNS[name] = dict(m=m, before=before, x=x, after=after, t_pos=t_pos, t_max=t_max, cap=cap, positions=positions, S=S, y=y.clone(), r=r, g=g,
                           exp=exp, ref=ref)
    return _RUNS[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_long_decode_ragged_equals_decode_rows_per_sequence(tune, name):
    R = run(name, tune)
    S, te = R["S"], R["t_max"]
    worst = 0.0
    for b, p in enumerate(R["positions"]):
        if not live(p, S, te):
            assert torch.count_nonzero(R["y"][b]) == 0 and torch.count_nonzero(R["r"][b]) == 0, (b, "a padding slot's y and ranges rows are zero")
            continue
        yr, rr = R["ref"][b]
        for s in range(S):
            assert norm(R["r"][b, s].cpu().numpy()) == norm(rr[s].cpu().numpy()), (b, s, "ranges")
        bar = 1e-2 * max(1.0, yr.float().abs().max().item())
        err = (R["y"][b].float() - yr.float()).abs().max().item()
        worst = max(worst, err)
        assert torch.isfinite(R["y"][b].float()).all() and err <= bar, (b, err, bar)
    print(f"{name}: max|y - decode_rows per sequence| {worst:.3e} (bar 1e-2 max(1, max|ref|))")
    # the appended token rows and the pooled compressed rows as the per-sequence calls wrote them, every other row of every slab untouched:
    # exp is the pool before the call plus exactly those rows
    for c in CACHES:
        got, want = getattr(R["after"], c), getattr(R["exp"], c)
        for b, p in enumerate(R["positions"]):
            lo, hi = (p, p + S) if c in TOKEN_CACHES else (ncmp(p), ncmp(p + S))
            if live(p, S, te) and hi > lo:
                d = (got[b, :, lo:hi].float() - want[b, :, lo:hi].float()).abs().max().item()
                assert same_bits(got[b, :, lo:hi], want[b, :, lo:hi]), (c, b, f"rows [{lo}, {hi}): max|d| = {d:.3e}")
        assert same_bits(got, want), (c, "every other row of every slab untouched")


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_long_decode_paged_equals_long_decode_ragged(tune, name):
    R = run(name, tune)
    m, S, te, positions = R["m"], R["S"], R["t_max"], R["positions"]
    B = len(positions)
    max_pages = te // 1024 + 1
    need = [((p + S - 1) >> 10) + 1 if live(p, S, te) else 0 for p in positions]
    pkv = m.new_paged_kv(sum(need) + 2, B, max_pages, "cuda", R["x"].dtype)
    for c in CACHES:
        getattr(pkv, c).fill_(float("nan"))
    for b, p in enumerate(positions):
        if need[b]:
            pkv.load_sequence(b, R["before"].sequence_view(b, p), p)
            pkv.ensure(b, p + S)
    plan = m.decode_paged_plan(B, S, max_pages, te, (te + 64) // 64)
    assert plan == m.decode_paged_plan(B, S, 2, 1052 + S - 1, 17) == {"launches": 10, "route": 1}, plan  # the launch count of today's in-range plan
    with torch.no_grad():
        y, _ = m.decode_paged(R["x"], pkv, R["t_pos"], t_max=te)
    r = m._last_ranges
    torch.cuda.synchronize()
    worst = 0.0
    for b, p in enumerate(positions):
        if not need[b]:
            assert torch.count_nonzero(y[b]) == 0 and torch.count_nonzero(r[b]) == 0, b
            continue
        assert torch.equal(r[b], R["r"][b]), (b, "ranges")
        err = (y[b].float() - R["y"][b].float()).abs().max().item()
        worst = max(worst, err)
        if m.d_k == 128:
            assert torch.equal(y[b], R["y"][b]), (b, err)
        else:
            assert torch.isfinite(y[b].float()).all() and err <= 1e-2 * max(1.0, R["y"][b].float().abs().max().item()), (b, err)
        got = pkv.gather_sequence(b, p + S)
        for c in CACHES:
            n = p + S if c in TOKEN_CACHES else ncmp(p + S)
            assert same_bits(getattr(got, c)[0, :, :n], getattr(R["after"], c)[b, :, :n]), (b, c, "the sequence's rows as the ragged call left them")
    print(f"{name}: max|y paged - y ragged| {worst:.3e} ({'torch.equal' if m.d_k == 128 else 'bar 1e-2 max(1, max|ref|)'})")
