"""CPU: the package's eager RoPE and pooling (nsa_vibe_amd.nsa_attention.apply_rope, avg_pool_phi) against the REFERENCE's apply_rope and
avg_pool_phi_rope_kv, outputs and autograd gradients (g22, oracle/make_rope_pool_goldens.py), in fp32, bf16 and fp16.  On the CPU both run
the same torch operations, so RoPE matches bit for bit.  The pooling is avg_pool1d here and avg_pool2d in the reference: in bf16 / fp16 they
give the same bits; in fp32 their window sums may be ordered differently, so fp32 pooling is held to the oracle's bound
(nsa_oracle.cmp_pool_bound) instead.  This pins the eager side that native-vs-eager GPU tests compare with."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
from conftest import load_golden

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.mark.parametrize("dt", gi.G22_DTYPES)
@pytest.mark.parametrize("case", list(gi.G22_ROPE_CASES))
def test_eager_apply_rope_matches_reference(case, dt):
    from nsa_vibe_amd.nsa_attention import apply_rope

    g = load_golden("g22_rope_pool")
    D, scale, _, grad = gi.G22_ROPE_CASES[case]
    x = gi.g22_inputs(case)
    xt = torch.from_numpy(x["x"]).to(TDT[dt]).requires_grad_(grad)
    y = apply_rope(xt, torch.from_numpy(x["pos"]), scale=scale)
    assert y.dtype == TDT[dt]
    assert np.array_equal(y.detach().float().numpy(), gi.g22_unpack(g[f"rope_{case}_{dt}_y"]))
    if grad:
        y.backward(torch.from_numpy(x["dy"]).to(TDT[dt]))
        assert np.array_equal(xt.grad.float().numpy(), gi.g22_unpack(g[f"rope_{case}_{dt}_dx"]))


@pytest.mark.parametrize("dt", gi.G22_DTYPES)
@pytest.mark.parametrize("case", list(gi.G22_POOL_CASES))
def test_eager_avg_pool_phi_matches_reference(orc, case, dt):
    """the module's eager pooling chain: avg_pool_phi(apply_rope(K_raw, pos), V_raw) -- the position scale is NOT passed (compress_pool.py:20)"""
    from nsa_vibe_amd.nsa_attention import apply_rope, avg_pool_phi

    g = load_golden("g22_rope_pool")
    l, d, D, S, _, _, grad = gi.G22_POOL_CASES[case]
    x = gi.g22_inputs(case)
    win = gi.g22_pool_windows(case)
    K = torch.from_numpy(x["K"]).to(TDT[dt]).requires_grad_(grad)
    V = torch.from_numpy(x["V"]).to(TDT[dt]).requires_grad_(grad)
    Kc, Vc = avg_pool_phi(apply_rope(K, torch.from_numpy(x["pos"])), V, l, d)
    n = 0 if S < l else (S - l) // d + 1
    assert Kc.shape == (1, 1, n, D) and Vc.shape == (1, 1, n, D)
    rK, rV = gi.g22_unpack(g[f"pool_{case}_{dt}_Kc"]), gi.g22_unpack(g[f"pool_{case}_{dt}_Vc"])
    gK, gV = Kc.detach().float().numpy()[:, :, win], Vc.detach().float().numpy()[:, :, win]
    if dt == "fp32":
        bK, bV = orc.cmp_pool_bound(x["K"], x["V"], l, d, x["pos"], dt)
        assert (np.abs(gK - rK) <= bK[:, :, win]).all() and (np.abs(gV - rV) <= bV[:, :, win]).all()
    else:
        assert np.array_equal(gK, rK) and np.array_equal(gV, rV)
    if grad:
        torch.autograd.backward([Kc, Vc], [torch.from_numpy(x["dKc"]).to(TDT[dt]), torch.from_numpy(x["dVc"]).to(TDT[dt])])
        rK, rV = gi.g22_unpack(g[f"pool_{case}_{dt}_dK"]), gi.g22_unpack(g[f"pool_{case}_{dt}_dV"])
        if dt == "fp32":
            bK, bV = orc.cmp_pool_bwd_bound(x["dKc"], x["dVc"], S, l, d, x["pos"], dt)
            assert (np.abs(K.grad.numpy() - rK) <= bK).all() and (np.abs(V.grad.numpy() - rV) <= bV).all()
        else:
            assert np.array_equal(K.grad.float().numpy(), rK) and np.array_equal(V.grad.float().numpy(), rV)
