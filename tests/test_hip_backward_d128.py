"""GPU: the MFMA attention backward at head dimension 128 (selection kernels, band dQ kernel, the layer's training step) against the
oracle, the generic kernel and itself (no atomics: bitwise run-to-run reproducibility)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128


@pytest.fixture(scope="module")
def nv():
    import nsa_vibe_amd

    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return nsa_vibe_amd


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def rounded(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def _rand_ranges(rng, B, S, G, n, S_kv, aligned):
    if aligned:
        st = rng.integers(0, max(1, S_kv // 64), size=(B, S, G, n)) * 64
        en = np.minimum(st + 64, S_kv)
    else:
        st = rng.integers(0, S_kv, size=(B, S, G, n))
        en = np.minimum(st + rng.integers(0, 90, size=st.shape), S_kv)
    return np.stack([st, en], axis=-1).astype(np.int32)


def _grads(nv, Q, K, V, rg, dO, dtype, bwd_variant, variant=0):
    q, k, v = (dev(x, dtype).requires_grad_(True) for x in (Q, K, V))
    nv.selection_attention_hip(q, k, v, dev(rg), variant=variant, bwd_variant=bwd_variant).backward(dev(dO, dtype))
    return q.grad, k.grad, v.grad


def _close(got, ref, tol=3e-2):
    got = got.float().cpu().numpy() if torch.is_tensor(got) else got
    ref = ref.float().cpu().numpy() if torch.is_tensor(ref) else ref
    assert np.isfinite(got).all()
    err = np.abs(got - ref).max()
    assert err <= tol * max(1.0, np.abs(ref).max()), f"err {err:.3e} (ref max {np.abs(ref).max():.2f})"


@pytest.mark.parametrize("B,S,G,h,S_kv,n,aligned", [(1, 6, 2, 6, 512, 5, True), (2, 300, 2, 6, 300, 6, False), (1, 700, 1, 16, 700, 4, True),
                                                   (2, 40, 2, 1, 130, 3, False), (1, 520, 2, 4, 520, 16, True)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sel_backward_d128_vs_oracle(nv, orc, B, S, G, h, S_kv, n, aligned, dtype):
    """MFMA backward at D = 128 (h = 16: the one-row dQ kernel) vs the oracle's backward and the generic kernel; bitwise reproducible"""
    rng = np.random.default_rng([B, S, h, n, D])
    Q = rng.standard_normal((B, S, G, h, D), dtype=np.float32)
    K = rng.standard_normal((B, G, S_kv, D), dtype=np.float32)
    V = rng.standard_normal((B, G, S_kv, D), dtype=np.float32)
    dO = rng.standard_normal((B, S, G, h, D), dtype=np.float32)
    rg = _rand_ranges(rng, B, S, G, n, S_kv, aligned)
    rg[0, 0, 0] = 0  # empty row
    rg[0, 1, 0, 0] = (0, S_kv)  # every key, overlapping the other ranges of the row
    g1 = _grads(nv, Q, K, V, rg, dO, dtype, 2)
    g2 = _grads(nv, Q, K, V, rg, dO, dtype, 2)
    for a, b_ in zip(g1, g2):
        assert torch.equal(a, b_)  # no atomics: bitwise reproducible
    assert not g1[0][0, 0, 0].any()  # empty row: zero dQ
    ref = orc.sel_attention_masked_bwd(rounded(Q, dtype), rounded(K, dtype), rounded(V, dtype), rg, rounded(dO, dtype))
    for got, r in zip(g1, ref):
        _close(got, r)
    for got, gen in zip(g1, _grads(nv, Q, K, V, rg, dO, dtype, 1)):
        _close(got, gen)


def test_sel_backward_d128_auto_routes_to_mfma(nv):
    """bwd_variant=None (auto) takes the MFMA route at D = 128: bitwise the gradients of bwd_variant=2"""
    rng = np.random.default_rng(128)
    B, S, G, h, S_kv, n = 2, 200, 2, 6, 400, 6
    Q, dO = (rng.standard_normal((B, S, G, h, D), dtype=np.float32) for _ in range(2))
    K, V = (rng.standard_normal((B, G, S_kv, D), dtype=np.float32) for _ in range(2))
    rg = _rand_ranges(rng, B, S, G, n, S_kv, False)
    for a, b_ in zip(_grads(nv, Q, K, V, rg, dO, torch.bfloat16, None), _grads(nv, Q, K, V, rg, dO, torch.bfloat16, 2)):
        assert torch.equal(a, b_)


def test_sel_backward_mfma_refused_where_unsupported(nv):
    """bwd_variant=2 raises for shapes the MFMA backward does not take (here Dk != Dv); auto falls back to the generic kernel"""
    B, S, G, h, S_kv = 1, 8, 1, 2, 64
    q = torch.randn(B, S, G, h, 128, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, G, S_kv, 128, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, G, S_kv, 64, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    rg = torch.tensor([[0, 64]], dtype=torch.int32, device="cuda").expand(B, S, G, 1, 2).contiguous()
    with pytest.raises(RuntimeError, match="MFMA variant requested"):
        nv.selection_attention_hip(q, k, v, rg, variant=1, bwd_variant=2).sum().backward()
    nv.selection_attention_hip(q, k, v, rg, variant=1).sum().backward()
    assert torch.isfinite(q.grad).all()


def test_sel_backward_d128_long_context_kernel_switch(nv, tune):
    """D = 128 dQ of the query-tile kernel == the one-row kernel: more than 65536 keys, ranges across key 65536 and the partial last tile"""
    rng = np.random.default_rng(2128)
    B, S, G, h, n, S_kv = 1, 21, 2, 6, 8, 70000
    Q = dev(rng.standard_normal((B, S, G, h, D), dtype=np.float32), torch.bfloat16)
    K = dev(rng.standard_normal((B, G, S_kv, D), dtype=np.float32), torch.bfloat16)
    V = dev(rng.standard_normal((B, G, S_kv, D), dtype=np.float32), torch.bfloat16)
    dO = dev(rng.standard_normal((B, S, G, h, D), dtype=np.float32), torch.bfloat16)
    st = rng.integers(0, S_kv - 200, size=(B, S, G, n))
    rg = np.stack([st, st + rng.integers(0, 150, size=st.shape)], axis=-1).astype(np.int32)
    rg[0, :, :, 0] = (0, 64)
    rg[0, :, :, 1] = (65500, 65610)
    rg[0, 2, 0] = 0  # empty row
    rg[0, 5, 1, 2] = (69990, 70000)
    res = {}
    for mode in ("0", "1"):
        tune("SEL_ROWS", mode)
        q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
        nv.selection_attention_hip(q, k, v, dev(rg), variant=2, bwd_variant=2).backward(dO)
        res[mode] = (q.grad, k.grad, v.grad)
    for a, b_ in zip(res["0"], res["1"]):
        assert torch.isfinite(a).all() and (a.float() - b_.float()).abs().max().item() <= 2e-2 * max(1.0, a.float().abs().max().item())
    assert not res["1"][0][0, 2, 0].any()


def test_sel_backward_d128_sixteen_row_splits(nv):
    """S = 16384: the dK / dV rows go to 16 splits whose partial slabs are summed in a fixed order -- bitwise reproducible, and equal
    to the generic kernel within bf16 tolerance"""
    torch.manual_seed(16)
    B, S, G, h, n = 1, 16384, 1, 6, 16
    Q = torch.randn(B, S, G, h, D, device="cuda", dtype=torch.bfloat16)
    K = torch.randn(B, G, S, D, device="cuda", dtype=torch.bfloat16)
    V = torch.randn(B, G, S, D, device="cuda", dtype=torch.bfloat16)
    dO = torch.randn(B, S, G, h, D, device="cuda", dtype=torch.bfloat16)
    meta = nv.build_block_meta(S, 32, 16, 64, n, 512)
    rg = nv.select_topn_ranges_batched(torch.rand(B, S, G, S // 64, device="cuda"), meta, n, S)
    res = []
    for bv in (2, 2, 1):
        q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
        nv.selection_attention_hip(q, k, v, rg, bwd_variant=bv).backward(dO)
        res.append((q.grad, k.grad, v.grad))
    for a, b_ in zip(res[0], res[1]):
        assert torch.equal(a, b_)
    for a, gen in zip(res[0], res[2]):
        _close(a, gen)


def test_sel_backward_d128_strided_kv(nv, orc):
    """K / V as views [:, :, :t] of larger [B, G, S_max, 128] buffers (the layout of NSA_KV)"""
    rng = np.random.default_rng(77)
    B, S, G, h, n, S_max = 2, 150, 2, 6, 5, 400
    Q = rng.standard_normal((B, S, G, h, D), dtype=np.float32)
    Kf = rng.standard_normal((B, G, S_max, D), dtype=np.float32)
    Vf = rng.standard_normal((B, G, S_max, D), dtype=np.float32)
    dO = rng.standard_normal((B, S, G, h, D), dtype=np.float32)
    rg = _rand_ranges(rng, B, S, G, n, S, False)
    dt = torch.bfloat16
    q = dev(Q, dt).requires_grad_(True)
    kf = dev(Kf, dt).requires_grad_(True)
    vf = dev(Vf, dt).requires_grad_(True)
    k, v = kf[:, :, :S], vf[:, :, :S]
    assert not k.is_contiguous()
    nv.selection_attention_hip(q, k, v, dev(rg), bwd_variant=2).backward(dev(dO, dt))
    rq, rk, rv = orc.sel_attention_masked_bwd(rounded(Q, dt), rounded(Kf[:, :, :S], dt), rounded(Vf[:, :, :S], dt), rg, rounded(dO, dt))
    _close(q.grad, rq)
    _close(kf.grad[:, :, :S], rk)
    _close(vf.grad[:, :, :S], rv)
    assert not kf.grad[:, :, S:].any() and not vf.grad[:, :, S:].any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("band,B,S,G", [(dict(w=77), 2, 300, 2), (dict(w=512), 1, 700, 2), (dict(a=32, dd=16, c=1), 1, 900, 2),
                                        (dict(w=512), 2, 2100, 4), (dict(a=32, dd=16, c=1), 2, 2100, 4)])
def test_band_backward_d128_vs_oracle(nv, orc, dtype, band, B, S, G):
    """band backward at D = 128: dQ kernel (few and >= 2048 token groups), dK / dV through the selection kernels; reproducible"""
    from nsa_vibe_amd.band_attention import band_attention_hip

    h = 6
    S_kv = S if "w" in band else (S - 32) // 16 + 1
    rng = np.random.default_rng(3000 + S)
    Q = rng.standard_normal((B, S, G, h, D), dtype=np.float32)
    K = rng.standard_normal((B, G, S_kv, D), dtype=np.float32)
    V = rng.standard_normal((B, G, S_kv, D), dtype=np.float32)
    dO = rng.standard_normal((B, S, G, h, D), dtype=np.float32)
    runs = []
    for _ in range(2):
        q, k, v = (dev(x, dtype).requires_grad_(True) for x in (Q, K, V))
        band_attention_hip(q, k, v, variant=2, bwd_variant=2, **band).backward(dev(dO, dtype))
        runs.append((q.grad, k.grad, v.grad))
    for a, b_ in zip(runs[0], runs[1]):
        assert torch.equal(a, b_)
    ref = orc.band_attention_bwd(rounded(Q, dtype), rounded(K, dtype), rounded(V, dtype), rounded(dO, dtype), **band)
    for got, r in zip(runs[0], ref):
        _close(got, r, 2e-2)


def test_layer_training_step_d128(nv):
    """NSAAttention with d_k = d_v = 128 in bf16, all three branches live: gradients of x and of every parameter against fp32 autograd of
    the same layer on the same ranges, and two identical steps give bitwise-equal gradients"""
    from test_hip_module import _torch_reference_layer

    from nsa_vibe_amd.nsa_attention import NSAAttention

    torch.manual_seed(5)
    m = NSAAttention(256, 4, 2, 128, 128, l=16, d=8, l_sel=32, n_sel=4, w=48, selector="batched").cuda().bfloat16().train()
    B, S = 2, 200
    x0 = torch.randn(B, S, 256, device="cuda")
    w_out = torch.randn(B, S, 256, device="cuda")
    steps = []
    for _ in range(2):
        m.zero_grad()
        x = x0.bfloat16().requires_grad_(True)
        out, _ = m(x, m.new_kv(B, S, "cuda", torch.bfloat16), prefill=True)
        (out.float() * w_out).sum().backward()
        steps.append((x.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()}, m._last_ranges.clone()))
    assert torch.equal(steps[0][2], steps[1][2])
    assert torch.equal(steps[0][0], steps[1][0])
    for n in steps[0][1]:
        assert torch.equal(steps[0][1][n], steps[1][1][n]), n
    m32 = NSAAttention(256, 4, 2, 128, 128, l=16, d=8, l_sel=32, n_sel=4, w=48, selector="batched").cuda().float().train()
    m32.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
    xr = x0.bfloat16().float().requires_grad_(True)
    ref = _torch_reference_layer(m32, xr, steps[0][2])
    (ref * w_out).sum().backward()
    _close(steps[0][0], xr.grad, 5e-2)
    for n, p in m32.named_parameters():
        _close(steps[0][1][n], p.grad, 5e-2)
