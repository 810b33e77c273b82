"""GPU parity: the sliding and the compressed branch with per-sequence positions (nsa_band_attn_fwd_ragged; the keyword arguments t_pos /
t_max of sliding_window_attention, batched_causal_attention_compressed and band_attention_hip).  Query row (b, s) sits at t_pos[b] + s.
Per sequence against the oracle's band attention at that sequence's position -- fp32 through the generic kernel to 1e-3, bf16 through the
MFMA kernel to 1e-2 at D = 64 and 128, the bars of DESIGN.md section 2 --, equal positions bit-equal to the scalar-t0 call, and slots
without a sequence or beyond the bounds zero with lse = -inf.

Every K/V row beyond a sequence's own tokens, and every compressed row beyond its n_cmp, holds +-3e4: a row that reads past its bound
cannot pass."""
import numpy as np
import pytest
import torch

from test_hip_selection import dev, nv  # noqa: F401

pytestmark = pytest.mark.gpu

G, H = 2, 6
L, D_, W = 32, 16, 512
BIG = 3.0e4
SETS = {"S1_mixed": ([1055, 40, 9, 4100, -1], 1), "S3_boundaries": ([1052, 1084, 29, 62, 5000], 3)}


def ncmp(t):
    return 0 if t + 1 < L else (t + 1 - L) // D_ + 1


_CASES = {}


def make_case(t_pos, S, D, dtype):
    """Q and, per branch, K/V of capacity t_max + 1 tokens (sliding) / n_cmp(t_max) compressed tokens, poisoned beyond each sequence's own"""
    key = (tuple(t_pos), S, D, dtype)
    if key not in _CASES:
        B = len(t_pos)
        t_max = max(t_pos) + S - 1
        rng = np.random.default_rng([abs(t) for t in t_pos] + [S, D])
        Q = rng.standard_normal((B, S, G, H, D), dtype=np.float32)
        kv = {}
        for branch, rows in (("sliding", t_max + 1), ("compressed", ncmp(t_max))):
            K = rng.standard_normal((B, G, rows, D), dtype=np.float32)
            V = rng.standard_normal((B, G, rows, D), dtype=np.float32)
            for b, t0 in enumerate(t_pos):
                own = 0 if t0 < 0 else (t0 + S if branch == "sliding" else ncmp(t0 + S - 1))
                K[b, :, own:] = BIG
                V[b, :, own:] = -BIG
            kv[branch] = (dev(K, dtype), dev(V, dtype))
        _CASES[key] = dict(t_pos=list(t_pos), S=S, B=B, D=D, t_max=t_max, Q=dev(Q, dtype), kv=kv,
                           pos=torch.tensor(t_pos, dtype=torch.int32, device="cuda"))
    return _CASES[key]


def run(nv, c, branch, variant=0, pos=None, t_max=None, t0=None, lse=False):
    K, V = c["kv"][branch]
    band = dict(a=0, dd=1, c=0, w=W) if branch == "sliding" else dict(a=L, dd=D_, c=1)
    if t0 is not None:
        return nv.band_attention_hip(c["Q"], K, V, t0=t0, variant=variant, return_lse=lse, **band)
    return nv.band_attention_hip(c["Q"], K, V, variant=variant, return_lse=lse, t_pos=c["pos"] if pos is None else pos,
                                 t_max=c["t_max"] if t_max is None else t_max, **band)


def check_against_oracle(nv, orc, c, branch, variant, tol):
    O, lse = run(nv, c, branch, variant, lse=True)
    torch.cuda.synchronize()
    assert torch.isfinite(O.float()).all()
    f = lambda a: a.float().cpu().numpy()  # noqa: E731
    K, V = c["kv"][branch]
    worst = 0.0
    for b, t0 in enumerate(c["t_pos"]):
        if t0 < 0:
            assert not O[b].any() and bool((lse[b] == -float("inf")).all()), b
            continue
        own = max(t0 + c["S"] if branch == "sliding" else ncmp(t0 + c["S"] - 1), 1)  # (an empty interval needs no key: one row keeps the shapes)
        q, k, v = f(c["Q"][b:b + 1]), f(K[b:b + 1, :, :own]), f(V[b:b + 1, :, :own])
        if branch == "sliding":
            O_ref = orc.sliding_window_attention(q, k, v, W, t0=t0)
        else:
            O_ref = orc.batched_causal_attention_compressed(q, k, v, L, D_, t0=t0)
            if ncmp(t0 + c["S"] - 1) == 0:
                assert not O[b].any() and bool((lse[b] == -float("inf")).all()), b
        worst = max(worst, float(np.abs(f(O[b:b + 1]) - O_ref).max()))
    print(f"band ragged {branch} {c['t_pos']} D={c['D']} variant={variant}: max|dO| vs oracle = {worst:.3e}")
    assert worst <= tol


@pytest.mark.parametrize("branch", ["sliding", "compressed"])
@pytest.mark.parametrize("name", list(SETS))
def test_fp32_generic_against_the_oracle(nv, orc, name, branch):
    t_pos, S = SETS[name]
    check_against_oracle(nv, orc, make_case(t_pos, S, 64, torch.float32), branch, 0, 1e-3)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("branch", ["sliding", "compressed"])
@pytest.mark.parametrize("name", list(SETS))
def test_bf16_mfma_against_the_oracle(nv, orc, name, branch, D):
    t_pos, S = SETS[name]
    check_against_oracle(nv, orc, make_case(t_pos, S, D, torch.bfloat16), branch, 2, 1e-2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("branch", ["sliding", "compressed"])
@pytest.mark.parametrize("S", [1, 3])
def test_equal_positions_are_the_scalar_call(nv, S, branch, dtype):
    t0 = 1052
    c = make_case([t0] * 3, S, 64, dtype)
    O, lse = run(nv, c, branch, lse=True)
    O1, lse1 = run(nv, c, branch, t0=t0, lse=True)
    torch.cuda.synchronize()
    assert torch.equal(O, O1) and torch.equal(lse, lse1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("branch", ["sliding", "compressed"])
def test_inactive_slots_are_zero(nv, branch, dtype):
    """a negative position, one past t_max, and one whose last row would need keys beyond S_kv: zero rows, lse = -inf; the live rows keep
    their bits"""
    S = 2
    c = make_case([1055, 40, 1190, 9], S, 64, dtype)
    O0, lse0 = run(nv, c, branch, lse=True)
    past_kv = c["t_max"] + 1 if branch == "sliding" else 16 * ncmp(c["t_max"]) + L  # the first position whose hi passes the S_kv rows given
    for bad, t_max in ((-1, c["t_max"]), (1150, 1100), (past_kv, past_kv + S)):
        pos = torch.tensor([1055, 40, bad, 9], dtype=torch.int32, device="cuda")
        # (t_max must still bound the live positions: the first two cases keep the case's, the middle one lowers it below the slot alone)
        live = [0, 1, 3]
        O, lse = run(nv, c, branch, pos=pos, t_max=t_max, lse=True)
        torch.cuda.synchronize()
        assert not O[2].any() and bool((lse[2] == -float("inf")).all()), (bad, t_max)
        for b in live:
            assert torch.equal(O[b], O0[b]) and torch.equal(lse[b], lse0[b]), (bad, t_max, b)
