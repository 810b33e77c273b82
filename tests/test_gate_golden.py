"""CPU: the eager gate MLP + three-branch mix of the package (nsa_vibe_amd.nsa_attention: GateMLP.forward, _gate_probs_fn,
NSAAttention._combine) against the REFERENCE module's outputs and autograd gradients (g21, oracle/make_gate_goldens.py).  This pins the
eager side that the native-vs-eager GPU tests compare with, so those become reference parity rather than self-consistency."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from conftest import load_golden

CASES = list(gi.G21_CASES)


def _gate(x, dtype=torch.float32):
    from nsa_vibe_amd.nsa_attention import GateMLP

    m = GateMLP(x["Dk"], x["Hd"])
    with torch.no_grad():
        for p, k in ((m.fc1.weight, "w1"), (m.fc1.bias, "b1"), (m.fc2.weight, "w2"), (m.fc2.bias, "b2")):
            p.copy_(torch.from_numpy(x[k]))
    return m.to(dtype)


def _layer(x, dtype=torch.float32):
    """NSAAttention of the case's head geometry whose output projection is the identity, so _combine returns the mix itself"""
    from nsa_vibe_amd.nsa_attention import NSAAttention

    G, h, Dk, Dv = gi.G21_G, x["h"], x["Dk"], x["Dv"]
    m = NSAAttention(G * h * Dv, G * h, G, Dk, Dv, gate_hidden=x["Hd"], gate_temp=x["tau"])
    m.gate = _gate(x)
    with torch.no_grad():
        m.out.weight.copy_(torch.eye(G * h * Dv))
    return m.to(dtype)


def _check_gates(got, g, case, tol=1e-6):
    ref = g[case + "_gates"]
    got = got.detach().float().reshape(-1, 3).numpy()
    assert np.abs(got - ref).max() <= tol
    # one-hot rows exactly where the reference's top-2 logit gap exceeds 50 (two exact zeros; a softmax row of fp32 has at most one)
    assert np.array_equal((got == 0.0).sum(1) == 2, g[case + "_gap"] > 50.0)


@pytest.mark.parametrize("case", CASES)
def test_gate_mlp_forward_matches_reference(case):
    from nsa_vibe_amd.nsa_attention import _gate_probs_fn

    g, x = load_golden("g21_gate"), gi.g21_inputs(case)
    m = _gate(x)
    q = torch.from_numpy(x["Q"]).mean(dim=3)
    with torch.no_grad():
        _check_gates(m(q, tau=x["tau"]), g, case)
        _check_gates(_gate_probs_fn(q, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, x["tau"]), g, case)


@pytest.mark.parametrize("case", CASES)
def test_combine_matches_reference_mix_and_gradients(case):
    """NSAAttention._combine (the eager mix every native-vs-eager test compares with): gates, O and the autograd gradients of dQ, the three
    branch outputs and the gate MLP's parameters against the reference's, including the zero MLP gradient of one-hot rows"""
    g, x = load_golden("g21_gate"), gi.g21_inputs(case)
    RD, G, h, Dk, Dv = gi.G21_RD, gi.G21_G, x["h"], x["Dk"], x["Dv"]
    m = _layer(x)
    Q, Oc, Os, Ow = (torch.from_numpy(x[k]) for k in ("Q", "O_cmp", "O_sel", "O_win"))
    with torch.no_grad():
        O = m._combine(Q, Oc, Os, Ow)
    _check_gates(m._last_gates, g, case)
    ref = g[case + "_O"]
    assert np.abs(O.reshape(-1, h, Dv)[:RD].numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    # gradients of the dense rows (the first RD / G tokens), for the fixture's dO
    n = RD // G
    ins = [t[:, :n].clone().requires_grad_(True) for t in (Q, Oc, Os, Ow)]
    (m._combine(*ins) * torch.from_numpy(x["dO"])[:, :n].reshape(1, n, -1)).sum().backward()
    got = dict(dQ=ins[0].grad.reshape(RD, h, Dk), dO_cmp=ins[1].grad.reshape(RD, h, Dv), dO_sel=ins[2].grad.reshape(RD, h, Dv),
               dO_win=ins[3].grad.reshape(RD, h, Dv), dW1=m.gate.fc1.weight.grad, db1=m.gate.fc1.bias.grad, dW2=m.gate.fc2.weight.grad,
               db2=m.gate.fc2.bias.grad)
    for k, v in got.items():
        r = g[case + "_" + k]
        err = float(np.abs(v.numpy() - r).max())
        assert err <= 1e-5 * max(1.0, float(np.abs(r).max())), (k, err)
    peaked = g[case + "_gap"][:RD] > 50.0
    if peaked.any():
        assert (got["dQ"][torch.from_numpy(peaked)] == 0).all()
    if not peaked.all():
        assert (got["dQ"][torch.from_numpy(~peaked)].abs().amax(dim=(1, 2)) > 0).all()


def test_combine_bf16_follows_the_reference_rounding_chain():
    """m7c in bf16 on CPU: the eager GateMLP + mix give the reference module's bf16 gates and outputs bit for bit (the rounding points the
    kernels mirror with rnd<T>)"""
    g, x = load_golden("g21_gate"), gi.g21_inputs("m7c")
    RD, h, Dv = gi.G21_RD, x["h"], x["Dv"]
    m = _layer(x, torch.bfloat16)
    with torch.no_grad():
        O = m._combine(*(torch.from_numpy(x[k]).bfloat16() for k in ("Q", "O_cmp", "O_sel", "O_win")))
    assert np.array_equal(m._last_gates.float().reshape(-1, 3).numpy(), g["m7c_gates_bf16"])
    assert np.array_equal(O.float().reshape(-1, h, Dv)[:RD].numpy(), g["m7c_O_bf16"])


def test_g21_fixture_is_non_uniform():
    """the fixture exercises the gate: non-peaked cases span the gates and every branch wins rows; the peaked case straddles the threshold"""
    g = load_golden("g21_gate")
    for case in CASES:
        gates, gap = g[case + "_gates"], g[case + "_gap"]
        if case == "peaked":
            assert 0.2 < (gap > 50).mean() < 0.8 and (np.abs(gap - 50.0) > 1e-3).all()
        elif case == "clamp":
            assert (gap > 50).all()
        else:
            assert gates.max(1).max() >= 0.7 and gates.min(1).min() <= 0.1 and (np.bincount(gates.argmax(1), minlength=3) > 0).all()
