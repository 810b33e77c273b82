"""GPU parity: the long-row form of the ragged decode step (switch DECODE_LONG = 1, plan form 3: one workgroup per row, the chunks beyond a
wave's first two swept twice, no workspace) on rows beyond the unsplit forms, up to 128 chunks (t = 131,071).

The reference of every live sequence is S selection_decode_step calls on its own B = 1 views truncated to the token -- existing code, never
the call under test -- with DECODE_WIDE = 0, so that no reference call takes the one-pass form (whose scores are not exact).  Ranges are
equal after norm; O is torch.equal wherever the reference call was the one-launch step (selection_decode_step_plan: launches 1; both sides
then run the same waves per row), and within the project's 1e-2 where it took the two-launch route.  Every case is one launch in form 3.

Inputs, helpers and method are those of tests/test_hip_decode_ragged.py: caches poisoned (+-3e4) beyond every sequence's own rows."""
import numpy as np
import pytest
import torch

from test_hip_decode_ragged import G, N_TOP, L, D_, L_SEL, W, active, assert_inactive_zero, assert_rows_equal, make_case, ncmp, plan, ragged
from test_hip_selection import norm, nv  # noqa: F401

pytestmark = pytest.mark.gpu

LIMIT = "beyond the long-row form: at most 131,072 tokens"

CASES = {
    # 16 chunks (the last row of form 0, inside a long launch) | S_cmp = 1025: one row in chunk 16, tail masks | few blocks | no compressed
    # token | an empty slot | 20 chunks
    "d128_S1": dict(t_pos=[16414, 16415, 40, 9, -1, 20000], S=1, D=128),
    "d128_S4_16_to_17_chunks": dict(t_pos=[16412], S=4, D=128),
    "d128_128_chunks": dict(t_pos=[131070, 100], S=2, D=128),          # sixteen chunks per wave, cand = 32, page 127
    # 64 chunks | S_cmp = 4097 | 97 chunks: wave 0 alone has a seventh | the limit | no compressed token
    "d64_S1": dict(t_pos=[65566, 65567, 98400, 131069, 29], S=1),
    "d64_S3": dict(t_pos=[65566, 65567, 98400, 131069, 29], S=3),
    "d64_waves8": dict(t_pos=[32798, 32799, 50000], S=1),             # 32 / 33 chunks (S_cmp = 2049) on 8 waves
    "f16": dict(t_pos=[65566, 65567, 98400, 131069, 29], S=1, dtype=torch.float16),
    "d64_h1": dict(t_pos=[65567, 40], S=1, h=1),
    "d64_h16": dict(t_pos=[65567, 40], S=1, h=16),
    "d128_h1": dict(t_pos=[16415, 40], S=1, D=128, h=1),
    "d128_h16": dict(t_pos=[16415, 40], S=1, D=128, h=16),
}


def step_reference(nv, c, tag):
    """per live sequence S single steps on its own truncated views, computed once per case and tag (the tuning switches in force) ->
    ({b: (O [1,S,G,h,D], ranges [1,S,G,n,2])}, {b: every call was the one-launch step})"""
    if tag not in c["refs"]:
        out, one = {}, {}
        S = c["S"]
        for b, t0 in enumerate(c["t_pos"]):
            if not active(t0, S, c["t_max"], c["K"].shape[2]):
                continue
            sl = slice(b, b + 1)
            Os, rs, one[b] = [], [], True
            for s in range(S):
                t = t0 + s
                m = nv.build_block_meta(t + 1, L, D_, L_SEL, N_TOP, W)
                if ncmp(t) >= 1:
                    p = nv.selection_decode_step_plan(1, G, c["h"], c["D"], c["D"], ncmp(t), m.S_sel, t + 1, N_TOP, c["dtype"])
                    assert p["form"] != 2, p  # (DECODE_WIDE = 0: never the one-pass form)
                    one[b] = one[b] and p["launches"] == 1
                O, r = nv.selection_decode_step(c["Q"][sl, s:s + 1], c["Kc"][sl, :, :ncmp(t)], c["K"][sl, :, :t + 1], c["V"][sl, :, :t + 1], m, N_TOP, t)
                Os.append(O)
                rs.append(r.unsqueeze(1))
            out[b] = (torch.cat(Os, dim=1), torch.cat(rs, dim=1))
        c["refs"][tag] = (out, one)
    return c["refs"][tag]


def check_against_steps(nv, tune, c, waves=None):
    tune("DECODE_LONG", 1)
    tune("DECODE_WIDE", 0)
    if waves:
        tune("DECODE_WAVES", waves)
    p = plan(nv, c)
    assert p == {"launches": 1, "form": 3}, p
    O, rg = ragged(nv, c)
    ref, one = step_reference(nv, c, f"steps_waves{waves}")
    torch.cuda.synchronize()
    assert torch.isfinite(O.float()).all()
    assert_inactive_zero(c, O, rg)
    exact = {b: v for b, v in ref.items() if one[b]}
    bound = {b: v for b, v in ref.items() if not one[b]}
    # the claim under test is bit equality on the rows that only the long form holds (more than two chunks per wave): their references must
    # be one-launch steps, or the claim would go untested without notice
    nw = 8 if c["D"] == 128 or waves == 8 else 16
    long_rows = [b for b in ref if (ncmp(c["t_pos"][b] + c["S"] - 1) + 63) // 64 > 2 * nw]
    assert long_rows and all(b in exact for b in long_rows), (long_rows, sorted(exact))
    assert_rows_equal(c, O, rg, exact)
    err = assert_rows_equal(c, O, rg, bound, exact=False)
    print(f"decode long {c['t_pos']} S={c['S']} D={c['D']} h={c['h']}: {len(exact)} sequences bit-equal to single steps, {len(bound)} against the "
          f"two-launch route: max|dO| = {err:.3e}")
    assert err <= 1e-2
    return O, rg


@pytest.mark.parametrize("name", [k for k in CASES if k != "d64_waves8"])
def test_long_equals_single_steps(nv, tune, name):
    check_against_steps(nv, tune, make_case(nv, **CASES[name]))


def test_long_on_eight_waves(nv, tune):
    """D = 64 on 8 waves per row, forced for the call and for the reference"""
    check_against_steps(nv, tune, make_case(nv, **CASES["d64_waves8"]), waves=8)


def test_inactive_and_out_of_range_slots(nv, tune):
    """a slot beyond t_max and a slot beyond the capacity beside an active long one: zero O and ranges rows, the others unchanged.  The
    buffers are physically larger than every position used and the smaller S_kv / t_max is passed"""
    tune("DECODE_LONG", 1)
    tune("DECODE_WIDE", 0)
    base = make_case(nv, [65567, 40, 65700], 1)  # (the third sequence only sizes the buffers)
    m = base["meta"]
    ref, _ = step_reference(nv, base, "steps_wavesNone")
    for S_kv, t_max, bad in ((65600, 65650, 65600), (base["K"].shape[2], 65580, 65581)):
        pos = [65567, bad, 40, -1]
        sel = [0, 2, 1, 1]
        Q, Kc = base["Q"][sel].contiguous(), base["Kc"][sel].contiguous()
        K, V = base["K"][sel].contiguous()[:, :, :S_kv], base["V"][sel].contiguous()[:, :, :S_kv]
        assert nv.selection_decode_ragged_plan(4, 1, G, 6, 64, 64, m.S_cmp, m.S_sel, S_kv, N_TOP, t_max)["form"] == 3
        O = torch.ones((4, 1, G, base["h"], base["D"]), dtype=base["dtype"], device="cuda")
        rg = torch.ones((4, 1, G, N_TOP, 2), dtype=torch.int32, device="cuda")
        nv.selection_decode_ragged(Q, Kc, K, V, m, N_TOP, torch.tensor(pos, dtype=torch.int32, device="cuda"), t_max=t_max, out=O, ranges_out=rg)
        torch.cuda.synchronize()
        for b in (1, 3):
            assert not O[b].any() and not rg[b].any(), (S_kv, t_max, b)
        for b in (0, 2):
            O1, r1 = ref[sel[b]]
            assert torch.equal(O[b], O1[0]), (S_kv, t_max, b)
            assert norm(rg[b, 0].cpu().numpy()) == norm(r1[0, 0].cpu().numpy()), (S_kv, t_max, b)


@pytest.mark.parametrize("name", ["d128_S1", "d64_S1"])
def test_long_against_the_oracle(nv, orc, tune, name):
    """the two comparisons of tests/test_hip_decode_ragged.py::test_ragged_against_the_oracle, in its method: ranges == the oracle's
    sequential selector on the existing scorer's device scores; O within 1e-2 of the oracle's masked attention"""
    tune("DECODE_LONG", 1)
    c = make_case(nv, **CASES[name])
    assert plan(nv, c)["form"] == 3
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
    print(f"decode long {c['t_pos']} D={c['D']}: max|dO| vs oracle = {worst:.3e}")
    assert worst <= 1e-2


@pytest.mark.parametrize("name", ["d128_128_chunks", "d64_S1"])
def test_long_run_to_run(nv, tune, name):
    tune("DECODE_LONG", 1)
    c = make_case(nv, **CASES[name])
    O, rg = ragged(nv, c)
    O2, rg2 = ragged(nv, c)
    torch.cuda.synchronize()
    assert torch.equal(O, O2) and torch.equal(rg, rg2)


def test_limits_and_the_switch(nv, tune):
    """t_max = 131,072 with the switch on: declined with the message that names the limit; the switch off: the old decline"""
    tune("DECODE_LONG", 1)
    c = make_case(nv, **CASES["d128_128_chunks"])
    m = c["meta"]
    assert nv.selection_decode_ragged_plan(c["B"], c["S"], G, c["h"], 128, 128, m.S_cmp, m.S_sel, c["K"].shape[2], N_TOP, 131072) == {"launches": 0, "form": -1}
    with pytest.raises(RuntimeError, match=LIMIT):
        nv.selection_decode_ragged(c["Q"], c["Kc"], c["K"], c["V"], m, N_TOP, c["pos"], t_max=131072)
    tune("DECODE_LONG", 0)
    c = make_case(nv, **CASES["d128_S1"])
    assert plan(nv, c) == {"launches": 0, "form": -1}
    with pytest.raises(RuntimeError, match="beyond the unsplit form at D = 128"):
        ragged(nv, c)
