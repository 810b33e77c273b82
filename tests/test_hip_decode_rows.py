"""GPU parity: the decode step of the selected branch for S consecutive tokens per sequence in one launch (nsa_sel_decode_rows, the rows
form of decode_step_kernel in sel_decode_fused.hip).  Row (b, s, g) of one call must be what selection_decode_step returns at t = t0 + s
on the cache truncated to t + 1 tokens: ranges equal, O bit for bit (both run exact forms of the same row functions), against the oracle's
selector and masked attention, causal (a row never reads what later tokens appended), and the same through the separate launches where the
one-launch form declines.

One deviation from bit equality is structural and handled explicitly: the decode attention merges the partial records of a row's waves,
and a launch of more than 256 rows at D = 64 runs 8 waves per row where S launches of B G <= 256 rows run 16 (dec_att_waves), which
groups the same chunks differently.  For such a call (B = 17, S = 8: 272 rows) O is compared bit for bit with single steps that run the
same 8 waves (switch DECODE_WAVES), and with the default single steps to the project's bf16 bound; ranges are equal to both."""
import numpy as np
import pytest
import torch

from test_hip_selection import dev, norm, nv  # noqa: F401  (nv: the module fixture of the D = 64 tests)

pytestmark = pytest.mark.gpu

G, N_TOP = 2, 16
L, D_, L_SEL, W = 32, 16, 64, 512


def ncmp(t):
    return 0 if t + 1 < L else (t + 1 - L) // D_ + 1


_CASES = {}


def make_case(nv, t0, S, B, D=64, h=6, dtype=torch.bfloat16):
    """inputs of one call (cached per shape and never modified: tests that overwrite work on clones): the cache after the S tokens"""
    key = (t0, S, B, D, h, dtype)
    if key not in _CASES:
        rng = np.random.default_rng([t0, S, B, D, h])
        n_tok = t0 + S
        m = nv.build_block_meta(n_tok, L, D_, L_SEL, N_TOP, W)
        Q = rng.standard_normal((B, S, G, h, D), dtype=np.float32)
        Kc = rng.standard_normal((B, G, m.S_cmp, D), dtype=np.float32)
        K = rng.standard_normal((B, G, n_tok + 37, D), dtype=np.float32)  # a preallocated cache longer than the context
        V = rng.standard_normal((B, G, n_tok + 37, D), dtype=np.float32)
        c = dict(t0=t0, S=S, B=B, D=D, h=h, dtype=dtype, meta=m, Q=dev(Q, dtype), Kc=dev(Kc, dtype), K=dev(K, dtype)[:, :, :n_tok],
                 V=dev(V, dtype)[:, :, :n_tok], singles={})
        assert m.S_cmp == ncmp(n_tok - 1)
        _CASES[key] = c
    return _CASES[key]


def plan(nv, c):
    m = c["meta"]
    return nv.selection_decode_rows_plan(c["B"], c["S"], G, c["h"], c["D"], c["D"], m.S_cmp, m.S_sel, c["t0"] + c["S"], N_TOP, c["dtype"])


def rows(nv, c, Kc=None, K=None, V=None):
    return nv.selection_decode_rows(c["Q"], c["Kc"] if Kc is None else Kc, c["K"] if K is None else K, c["V"] if V is None else V, c["meta"],
                                    N_TOP, c["t0"])


def single_steps(nv, c, tag="default"):
    """S calls of selection_decode_step on the truncated views (computed once per case and tag) -> (O [B,S,G,h,D], ranges [B,S,G,n,2])"""
    if tag not in c["singles"]:
        Os, rs = [], []
        for s in range(c["S"]):
            t = c["t0"] + s
            m = nv.build_block_meta(t + 1, L, D_, L_SEL, N_TOP, W)
            O, r = nv.selection_decode_step(c["Q"][:, s:s + 1], c["Kc"][:, :, :ncmp(t)], c["K"][:, :, :t + 1], c["V"][:, :, :t + 1], m, N_TOP, t)
            Os.append(O)
            rs.append(r.unsqueeze(1))
        c["singles"][tag] = (torch.cat(Os, dim=1), torch.cat(rs, dim=1))
    return c["singles"][tag]


def assert_ranges_equal(rg, r1, S):
    for s in range(S):
        assert norm(rg[:, s].cpu().numpy()) == norm(r1[:, s].cpu().numpy()), s


SHAPES = [
    dict(t0=1052, S=8, B=3),            # n_cmp 64 -> 65 at t = 1055: rows of one call have one and two chunks
    dict(t0=1084, S=8, B=2),            # selection block 16 completes at t = 1087
    dict(t0=40, S=5, B=2),              # n_cmp 1 -> 2, fewer blocks than n_top, overlapping forced blocks
    dict(t0=32796, S=8, B=1),           # n_cmp 2048 -> 2049 at t = 32799: form 1, while the first rows would fit form 0
    dict(t0=5000, S=8, B=17),           # 272 rows: the 8-wave workgroups
    dict(t0=9000, S=1, B=3),            # S = 1: the decode step itself
    dict(t0=1052, S=8, B=3, D=128),
    dict(t0=1052, S=8, B=3, dtype=torch.float16),
    dict(t0=1052, S=8, B=3, h=1, dtype=torch.float16),
    dict(t0=1052, S=8, B=3, h=4),
    dict(t0=1052, S=8, B=3, h=16),
    dict(t0=1052, S=8, B=3, h=16, dtype=torch.float16),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()).replace("torch.", ""))
def test_rows_equal_single_steps(nv, tune, shape):
    """one rows call == S single decode steps on the truncated views: ranges equal after norm, O torch.equal; the call is ONE launch"""
    c = make_case(nv, **shape)
    p = plan(nv, c)
    assert p["launches"] == 1, p
    assert p["form"] == (1 if c["t0"] == 32796 else 0), p
    O, rg = rows(nv, c)
    O1, r1 = single_steps(nv, c)
    torch.cuda.synchronize()
    assert_ranges_equal(rg, r1, c["S"])
    if c["D"] == 64 and c["B"] * c["S"] * G > 256 >= c["B"] * G:
        # 8 waves per row here, 16 in the single steps: same chunks, another grouping of the partial records (module docstring)
        err = (O.float() - O1.float()).abs().max().item()
        print(f"rows (8 waves) vs single steps (16 waves): max|dO| = {err:.3e}")
        assert err <= 1e-2
        tune("DECODE_WAVES", 8)
        O1, r8 = single_steps(nv, c, "waves8")
        torch.cuda.synchronize()
        assert_ranges_equal(rg, r8, c["S"])
    assert torch.equal(O, O1)
    if c["S"] == 1:
        assert torch.equal(rg[:, 0], r1[:, 0])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[6]], ids=["t1052", "t32796", "d128"])
def test_rows_against_the_oracle(nv, orc, shape):
    """per row: ranges == the oracle's sequential selector on that row's device scores at t; O within the bf16 bound (1e-2) of the oracle's
    masked attention on the bf16-rounded inputs truncated to t + 1"""
    c = make_case(nv, **shape)
    assert plan(nv, c)["launches"] == 1
    O, rg = rows(nv, c)
    torch.cuda.synchronize()
    f = lambda a: a.float().cpu().numpy()  # noqa: E731
    worst = 0.0
    for s in range(c["S"]):
        t = c["t0"] + s
        m = nv.build_block_meta(t + 1, L, D_, L_SEL, N_TOP, W)
        mo = orc.build_block_meta(t + 1, L, D_, L_SEL, N_TOP, W)
        pg = nv.selection_scores(c["Q"][:, s:s + 1], c["Kc"][:, :, :ncmp(t)], m)
        r_ref = orc.select_topn_ranges(pg[:, 0].cpu().numpy(), mo, N_TOP, t)
        got = rg[:, s].cpu().numpy()
        assert norm(got) == norm(r_ref), s
        O_ref = orc.sel_attention_masked(f(c["Q"][:, s:s + 1]), f(c["K"][:, :, :t + 1]), f(c["V"][:, :, :t + 1]), got[:, None])
        worst = max(worst, float(np.abs(f(O[:, s:s + 1]) - O_ref).max()))
    print(f"decode rows t0={c['t0']} D={c['D']}: max|dO| vs oracle = {worst:.3e}")
    assert worst <= 1e-2


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[6]], ids=["d64", "d128"])
def test_rows_are_causal(nv, shape):
    """what row s = 0 must not see -- K/V beyond t0 and compressed rows beyond n_cmp(t0) -- overwritten with large finite values: row 0 is
    bit-identical, the last row is not"""
    c = make_case(nv, **shape)
    assert plan(nv, c)["launches"] == 1
    O, rg = rows(nv, c)
    Kc, K, V = c["Kc"].clone(), c["K"].clone(), c["V"].clone()
    K[:, :, c["t0"] + 1:] = 3.0e4
    V[:, :, c["t0"] + 1:] = -3.0e4
    Kc[:, :, ncmp(c["t0"]):] = 3.0e4
    O2, rg2 = rows(nv, c, Kc, K, V)
    torch.cuda.synchronize()
    assert torch.isfinite(O2[:, 0].float()).all()
    assert torch.equal(rg[:, 0], rg2[:, 0]) and torch.equal(O[:, 0], O2[:, 0])
    assert not torch.equal(O[:, -1], O2[:, -1])


@pytest.mark.parametrize("why", ["unfused", "S17", "t10", "d128_long"])
def test_declined_shapes_take_the_separate_launches(nv, tune, why):
    """where the one-launch form declines the plan says more than one launch, the call still returns and agrees with the S single steps
    (ranges equal, O within 1e-2)"""
    if why == "unfused":
        c = make_case(nv, t0=1052, S=8, B=3)
        tune("DECODE_UNFUSED", 1)
    elif why == "S17":
        c = make_case(nv, t0=1052, S=17, B=2)
    elif why == "t10":
        c = make_case(nv, t0=10, S=8, B=2)  # n_cmp(t0) = 0
    else:
        c = make_case(nv, t0=20000, S=8, B=1, D=128)  # more than 16 chunks at D = 128
    p = plan(nv, c)
    assert p["launches"] > 1 and p["form"] == -1, p
    O, rg = rows(nv, c)
    O1, r1 = single_steps(nv, c, why)
    torch.cuda.synchronize()
    assert_ranges_equal(rg, r1, c["S"])
    err = (O.float() - O1.float()).abs().max().item()
    print(f"separate launches ({why}) vs single steps: max|dO| = {err:.3e}")
    assert err <= 1e-2


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[4], SHAPES[6]], ids=["t1052", "form1", "waves8", "d128"])
def test_rows_run_to_run(nv, shape):
    c = make_case(nv, **shape)
    assert plan(nv, c)["launches"] == 1
    O, rg = rows(nv, c)
    O2, rg2 = rows(nv, c)
    torch.cuda.synchronize()
    assert torch.equal(O, O2) and torch.equal(rg, rg2)
