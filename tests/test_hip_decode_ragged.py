"""GPU parity: the ragged-batch decode step of the selected branch (nsa_sel_decode_ragged: the rows form of decode_step_kernel with the
position of every sequence read from a device array).  Row (b, s, g) of one call must be what the per-sequence calls return for sequence b
alone at t = t_pos[b] + s: ranges equal, O bit for bit wherever both sides run the same waves per row; against the oracle's selector and
masked attention; zeros for slots that hold no sequence or whose position passes the bounds; a decline where t_max passes the unsplit
forms; and the existing entry points keep their bits.

Nothing is hidden in the inputs: every K/V row beyond a sequence's own tokens and every K_cmp row beyond its n_cmp holds large finite values
(+-3e4), so a row that reads past its bound cannot pass.

As in tests/test_hip_decode_rows.py one deviation from bit equality is structural: a launch of more than 256 rows at D = 64 runs 8 waves per
row where the per-sequence calls run 16; that case is compared bit for bit with references run at DECODE_WAVES = 8 and to the bf16 bound
(1e-2) with the default ones."""
import numpy as np
import pytest
import torch

from test_hip_selection import dev, norm, nv  # noqa: F401  (nv: the module fixture of the D = 64 tests)

pytestmark = pytest.mark.gpu

G, N_TOP = 2, 16
L, D_, L_SEL, W = 32, 16, 64, 512
BIG = 3.0e4


def ncmp(t):
    return 0 if t + 1 < L else (t + 1 - L) // D_ + 1


def active(t0, S, t_max, S_kv):
    return t0 >= 0 and t0 + S - 1 <= min(t_max, S_kv - 1)


_CASES = {}


def make_case(nv, t_pos, S, D=64, h=6, dtype=torch.bfloat16):
    """inputs of one call (cached per shape and never modified): caches allocated 37 rows beyond t_max + S, sequence b's K/V rows from
    t_pos[b] + S on and its K_cmp rows from n_cmp(t_pos[b] + S - 1) on poisoned (all of them for an empty slot)"""
    key = (tuple(t_pos), S, D, h, dtype)
    if key not in _CASES:
        B = len(t_pos)
        t_max = max(t for t in t_pos if t >= 0) + S - 1
        rng = np.random.default_rng([abs(t) for t in t_pos] + [S, D, h])
        cap = t_max + S + 37
        m = nv.build_block_meta(t_max + 1, L, D_, L_SEL, N_TOP, W)
        assert m.S_cmp == ncmp(t_max)
        Q = rng.standard_normal((B, S, G, h, D), dtype=np.float32)
        Kc = rng.standard_normal((B, G, max(m.S_cmp, 1), D), dtype=np.float32)
        K = rng.standard_normal((B, G, cap, D), dtype=np.float32)
        V = rng.standard_normal((B, G, cap, D), dtype=np.float32)
        for b, t0 in enumerate(t_pos):
            own = t0 + S if t0 >= 0 else 0
            K[b, :, own:] = BIG
            V[b, :, own:] = -BIG
            Kc[b, :, ncmp(own - 1) if own else 0:] = BIG
        c = dict(t_pos=list(t_pos), t_max=t_max, S=S, B=B, D=D, h=h, dtype=dtype, meta=m, Q=dev(Q, dtype), Kc=dev(Kc, dtype)[:, :, :m.S_cmp],
                 K=dev(K, dtype)[:, :, :t_max + 1], V=dev(V, dtype)[:, :, :t_max + 1], refs={})
        c["pos"] = torch.tensor(t_pos, dtype=torch.int32, device="cuda")
        _CASES[key] = c
    return _CASES[key]


def plan(nv, c):
    m = c["meta"]
    return nv.selection_decode_ragged_plan(c["B"], c["S"], G, c["h"], c["D"], c["D"], m.S_cmp, m.S_sel, c["K"].shape[2], N_TOP, c["t_max"], c["dtype"])


def ragged(nv, c, pos=None, **kw):
    return nv.selection_decode_ragged(c["Q"], c["Kc"], c["K"], c["V"], c["meta"], N_TOP, c["pos"] if pos is None else pos, t_max=c["t_max"], **kw)


def per_sequence(nv, c, tag="default"):
    """what a caller runs today, computed once per case and tag: for every live sequence b one selection_decode_rows call on its B = 1
    views truncated to its own tokens (t0 = t_pos[b]), or -- where n_cmp(t_pos[b]) < 1, which the rows form declines -- one
    selection_decode_step per token -> {b: (O [1,S,G,h,D], ranges [1,S,G,n,2])}"""
    if tag not in c["refs"]:
        out = {}
        S = c["S"]
        for b, t0 in enumerate(c["t_pos"]):
            if not active(t0, S, c["t_max"], c["K"].shape[2]):
                continue
            sl = slice(b, b + 1)
            if ncmp(t0) >= 1:
                m = nv.build_block_meta(t0 + S, L, D_, L_SEL, N_TOP, W)
                out[b] = nv.selection_decode_rows(c["Q"][sl], c["Kc"][sl, :, :ncmp(t0 + S - 1)], c["K"][sl, :, :t0 + S], c["V"][sl, :, :t0 + S], m, N_TOP, t0)
            else:
                Os, rs = [], []
                for s in range(S):
                    t = t0 + s
                    m = nv.build_block_meta(t + 1, L, D_, L_SEL, N_TOP, W)
                    O, r = nv.selection_decode_step(c["Q"][sl, s:s + 1], c["Kc"][sl, :, :ncmp(t)], c["K"][sl, :, :t + 1], c["V"][sl, :, :t + 1], m, N_TOP, t)
                    Os.append(O)
                    rs.append(r.unsqueeze(1))
                out[b] = (torch.cat(Os, dim=1), torch.cat(rs, dim=1))
        c["refs"][tag] = out
    return c["refs"][tag]


def assert_rows_equal(c, O, rg, ref, exact=True):
    worst = 0.0
    for b, (O1, r1) in ref.items():
        for s in range(c["S"]):
            assert norm(rg[b, s].cpu().numpy()) == norm(r1[0, s].cpu().numpy()), (b, s)
        if exact:
            assert torch.equal(O[b], O1[0]), b
        else:
            worst = max(worst, (O[b].float() - O1[0].float()).abs().max().item())
    return worst


def assert_inactive_zero(c, O, rg):
    for b, t0 in enumerate(c["t_pos"]):
        if not active(t0, c["S"], c["t_max"], c["K"].shape[2]):
            assert not O[b].any() and not rg[b].any(), b


_B33 = [int(v) for v in np.random.default_rng(33).integers(0, 6001, size=33)]

CASES = [
    dict(t_pos=[1055, 40, 9, 4100, -1], S=1),          # two chunks, few blocks, no compressed token, an empty slot
    dict(t_pos=[1052, 1084, 29, 62, 5000], S=3),       # n_cmp 64 -> 65, block 16 completing at 1087, n_cmp 0 -> 1 at t = 31, block 0 completing at 63
    dict(t_pos=[32796, 100], S=8),                     # form 1 launched for a batch whose short row would fit form 0
    dict(t_pos=_B33, S=4),                             # 264 rows: the 8-wave workgroups
    dict(t_pos=[1052, 40, 9000], S=4, D=128),
    dict(t_pos=[1055, 40, 9, 4100, -1], S=1, dtype=torch.float16),
    dict(t_pos=[1055, 40, 9, 4100, -1], S=1, h=1),
    dict(t_pos=[1055, 40, 9, 4100, -1], S=1, h=4),
    dict(t_pos=[1055, 40, 9, 4100, -1], S=1, h=16),
]
IDS = ["S1_mixed", "S3_boundaries", "form1", "B33_waves8", "d128", "f16", "h1", "h4", "h16"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ragged_equals_per_sequence_calls(nv, tune, case):
    """one ragged call == one call per sequence on its own truncated views: ranges equal after norm, O torch.equal; ONE launch"""
    c = make_case(nv, **case)
    p = plan(nv, c)
    assert p["launches"] == 1, p
    assert p["form"] == (1 if c["t_max"] > 32768 else 0), p
    O, rg = ragged(nv, c)
    ref = per_sequence(nv, c)
    torch.cuda.synchronize()
    assert torch.isfinite(O.float()).all()
    assert_inactive_zero(c, O, rg)
    if c["D"] == 64 and c["B"] * c["S"] * G > 256:
        # 8 waves per row here, 16 in the per-sequence calls: same chunks, another grouping of the partial records (module docstring)
        err = assert_rows_equal(c, O, rg, ref, exact=False)
        print(f"ragged (8 waves) vs per-sequence calls (16 waves): max|dO| = {err:.3e}")
        assert err <= 1e-2
        tune("DECODE_WAVES", 8)
        ref = per_sequence(nv, c, "waves8")
        torch.cuda.synchronize()
    assert_rows_equal(c, O, rg, ref)


@pytest.mark.parametrize("shape", [dict(t0=1052, S=8, B=3), dict(t0=1052, S=8, B=3, D=128)], ids=["d64", "d128"])
def test_equal_positions_are_the_rows_call(nv, shape):
    """t_pos = [t0] * B: ranges and O torch.equal with selection_decode_rows(t0) on the same buffers"""
    t0, B = shape["t0"], shape["B"]
    c = make_case(nv, [t0] * B, shape["S"], D=shape.get("D", 64))
    assert plan(nv, c)["launches"] == 1
    O, rg = ragged(nv, c)
    O1, r1 = nv.selection_decode_rows(c["Q"], c["Kc"], c["K"], c["V"], c["meta"], N_TOP, t0)
    torch.cuda.synchronize()
    assert torch.equal(rg, r1) and torch.equal(O, O1)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=["S1_mixed", "S3_boundaries", "d128"])
def test_ragged_against_the_oracle(nv, orc, case):
    """per row: ranges == the oracle's sequential selector on that row's device scores at t (zeros where the row has no compressed token);
    O within the bf16 bound (1e-2) of the oracle's masked attention on the bf16-rounded inputs truncated to t + 1"""
    c = make_case(nv, **case)
    O, rg = ragged(nv, c)
    torch.cuda.synchronize()
    f = lambda a: a.float().cpu().numpy()  # noqa: E731
    worst = 0.0
    for b, t0 in enumerate(c["t_pos"]):
        if not active(t0, c["S"], c["t_max"], c["K"].shape[2]):
            continue
        sl = slice(b, b + 1)
        for s in range(c["S"]):
            t = t0 + s
            m = nv.build_block_meta(t + 1, L, D_, L_SEL, N_TOP, W)
            mo = orc.build_block_meta(t + 1, L, D_, L_SEL, N_TOP, W)
            if ncmp(t) >= 1:
                pg = nv.selection_scores(c["Q"][sl, s:s + 1], c["Kc"][sl, :, :ncmp(t)], m)[:, 0].cpu().numpy()
            else:
                pg = np.zeros((1, G, m.S_sel), dtype=np.float32)
            r_ref = orc.select_topn_ranges(pg, mo, N_TOP, t)
            got = rg[sl, s].cpu().numpy()
            assert norm(got) == norm(r_ref), (b, s)
            O_ref = orc.sel_attention_masked(f(c["Q"][sl, s:s + 1]), f(c["K"][sl, :, :t + 1]), f(c["V"][sl, :, :t + 1]), got[:, None])
            worst = max(worst, float(np.abs(f(O[sl, s:s + 1]) - O_ref).max()))
    print(f"decode ragged {case['t_pos']} D={c['D']}: max|dO| vs oracle = {worst:.3e}")
    assert worst <= 1e-2


@pytest.mark.parametrize("S", [1, 2])
def test_inactive_and_out_of_range_slots(nv, S):
    """positions -1, S_kv - S + 1 and t_max + 1 give all-zero O and ranges; the other rows are unchanged bit for bit.  The buffers are
    physically larger than every position used and the smaller S_kv / t_max is passed: even an unguarded kernel stays inside them"""
    base = make_case(nv, [1055, 40, 1190, 9], S)  # (the third sequence only sizes the buffers: 1190 + S + 37 rows)
    m = base["meta"]
    ref = per_sequence(nv, base)
    for S_kv, t_max, bad in ((1080, 1100, 1080 - S + 1), (base["K"].shape[2], 1060, 1061)):
        pos = [1055, -1, bad, 40, 9]
        sel = [0, 0, 2, 1, 3]  # the inputs of slot b are those of sequence sel[b] of the base case
        Q, Kc = base["Q"][sel].contiguous(), base["Kc"][sel].contiguous()
        K, V = base["K"][sel].contiguous()[:, :, :S_kv], base["V"][sel].contiguous()[:, :, :S_kv]
        O = torch.ones((5, S, G, base["h"], base["D"]), dtype=base["dtype"], device="cuda")
        rg = torch.ones((5, S, G, N_TOP, 2), dtype=torch.int32, device="cuda")
        nv.selection_decode_ragged(Q, Kc, K, V, m, N_TOP, torch.tensor(pos, dtype=torch.int32, device="cuda"), t_max=t_max, out=O, ranges_out=rg)
        torch.cuda.synchronize()
        for b in (1, 2):
            assert not O[b].any() and not rg[b].any(), (S_kv, t_max, b)
        for b in (0, 3, 4):
            O1, r1 = ref[sel[b]]
            assert torch.equal(O[b], O1[0]), (S_kv, t_max, b)
            for s in range(S):
                assert norm(rg[b, s].cpu().numpy()) == norm(r1[0, s].cpu().numpy()), (S_kv, t_max, b, s)


def test_declined_plan_and_the_wrapper(nv):
    """t_max past the forms (D = 128: more than 16 chunks): the plan reports a decline, host positions still return the per-sequence
    results (zeros for the empty slot), device positions raise with the library's message"""
    c = make_case(nv, [20000, 100, -1], 2, D=128)
    p = plan(nv, c)
    assert p == {"launches": 0, "form": -1}, p
    O, rg = nv.selection_decode_ragged(c["Q"], c["Kc"], c["K"], c["V"], c["meta"], N_TOP, c["t_pos"])
    ref = per_sequence(nv, c)
    torch.cuda.synchronize()
    assert_inactive_zero(c, O, rg)
    err = assert_rows_equal(c, O, rg, ref, exact=False)
    assert err <= 1e-2
    with pytest.raises(RuntimeError, match="beyond the unsplit form at D = 128"):
        ragged(nv, c)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3], CASES[4]], ids=["S1_mixed", "form1", "B33_waves8", "d128"])
def test_ragged_run_to_run(nv, case):
    c = make_case(nv, **case)
    O, rg = ragged(nv, c)
    O2, rg2 = ragged(nv, c)
    torch.cuda.synchronize()
    assert torch.equal(O, O2) and torch.equal(rg, rg2)


def test_host_positions_are_the_device_positions(nv):
    """host integers (a list, a CPU tensor): copied without a t_max, same bits as the device array"""
    c = make_case(nv, **CASES[0])
    O, rg = ragged(nv, c)
    for host in (c["t_pos"], torch.tensor(c["t_pos"], dtype=torch.int64)):
        O2, rg2 = nv.selection_decode_ragged(c["Q"], c["Kc"], c["K"], c["V"], c["meta"], N_TOP, host)
        torch.cuda.synchronize()
        assert torch.equal(O, O2) and torch.equal(rg, rg2)


def test_existing_entry_points_keep_their_bits(nv):
    """SHAPES[0] of tests/test_hip_decode_rows.py (t0 = 1052, S = 8, B = 3), rebuilt here: selection_decode_rows and S calls of
    selection_decode_step are still bit-equal to each other"""
    t0, S, B, D, h = 1052, 8, 3, 64, 6
    rng = np.random.default_rng([t0, S, B, D, h])
    n_tok = t0 + S
    m = nv.build_block_meta(n_tok, L, D_, L_SEL, N_TOP, W)
    Q = dev(rng.standard_normal((B, S, G, h, D), dtype=np.float32), torch.bfloat16)
    Kc = dev(rng.standard_normal((B, G, m.S_cmp, D), dtype=np.float32), torch.bfloat16)
    K = dev(rng.standard_normal((B, G, n_tok + 37, D), dtype=np.float32), torch.bfloat16)[:, :, :n_tok]
    V = dev(rng.standard_normal((B, G, n_tok + 37, D), dtype=np.float32), torch.bfloat16)[:, :, :n_tok]
    assert nv.selection_decode_rows_plan(B, S, G, h, D, D, m.S_cmp, m.S_sel, n_tok, N_TOP)["launches"] == 1
    O, rg = nv.selection_decode_rows(Q, Kc, K, V, m, N_TOP, t0)
    for s in range(S):
        t = t0 + s
        m1 = nv.build_block_meta(t + 1, L, D_, L_SEL, N_TOP, W)
        O1, r1 = nv.selection_decode_step(Q[:, s:s + 1], Kc[:, :, :ncmp(t)], K[:, :, :t + 1], V[:, :, :t + 1], m1, N_TOP, t)
        torch.cuda.synchronize()
        assert norm(rg[:, s].cpu().numpy()) == norm(r1.cpu().numpy()), s
        assert torch.equal(O[:, s:s + 1], O1), s
