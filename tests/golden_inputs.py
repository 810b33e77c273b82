"""Seeded input recipes shared by oracle/make_goldens.py (fixture generation, build container)
and the parity tests (CPU + GPU box).  numpy PCG64 streams only -- numpy guarantees
`default_rng(seed)` bit-streams are stable across versions/platforms, so inputs too big to
commit (64k K/V) are regenerated instead of stored; fixtures hold the expected outputs.
"""
import numpy as np


def _rng(*key):
    return np.random.default_rng(list(key))


def randn(rng, *shape):
    return rng.standard_normal(shape, dtype=np.float32)


# g5: test_selection_varlen_semantic.py:46-58 shape (B2 S6 G1 h2 D32 S_kv16, span 3)
def g5_inputs():
    r = _rng(5)
    B, S, G, h, Dk, Dv, S_kv = 2, 6, 1, 2, 32, 32, 16
    Q, K, V = randn(r, B, S, G, h, Dk), randn(r, B, G, S_kv, Dk), randn(r, B, G, S_kv, Dv)
    rg = np.zeros((B, S, G, 2, 2), np.int32)
    for t in range(S):
        rg[:, t, :, 0, 0] = max(0, t - 3)
        rg[:, t, :, 0, 1] = min(S_kv, t + 1)
    return Q, K, V, rg


# g6: test_selection_masked_empty_rows.py:6-20
def g6_inputs():
    r = _rng(6)
    Q, K, V = randn(r, 1, 2, 1, 2, 8), randn(r, 1, 1, 4, 8), randn(r, 1, 1, 4, 8)
    return Q, K, V, np.zeros((1, 2, 1, 1, 2), np.int32)


# g7: test_triton_sel_edge_cases.py:23-39 (clamping of out-of-bounds ranges)
def g7_inputs():
    r = _rng(7)
    B, S, G, h, D, S_kv = 1, 1, 1, 2, 16, 16
    Q, K, V = randn(r, B, S, G, h, D), randn(r, B, G, S_kv, D), randn(r, B, G, S_kv, D)
    rg = np.array([[-5, -1], [10, 100]], np.int32).reshape(1, 1, 1, 2, 2)
    return Q, K, V, rg


# g8: test_triton_sel_parity_gpu.py:21-37 multi-span
def g8_inputs():
    r = _rng(8)
    B, S, G, h, D, S_kv = 4, 1, 1, 2, 64, 192
    Q, K, V = randn(r, B, S, G, h, D), randn(r, B, G, S_kv, D), randn(r, B, G, S_kv, D)
    rg = np.zeros((B, S, G, 3, 2), np.int32)
    rg[..., 0, :] = (16, 40)
    rg[..., 1, :] = (64, 96)
    rg[..., 2, :] = (120, 160)
    return Q, K, V, rg


# g8b: overlapping, unsorted, duplicated, empty and inverted ranges -> union semantics
def g8b_inputs():
    r = _rng(88)
    B, S, G, h, D, S_kv = 2, 3, 2, 3, 32, 100
    Q, K, V = randn(r, B, S, G, h, D), randn(r, B, G, S_kv, D), randn(r, B, G, S_kv, D)
    rg = np.zeros((B, S, G, 6, 2), np.int32)
    rg[:, 0, :] = [[50, 70], [10, 30], [20, 40], [10, 30], [0, 0], [90, 100]]
    rg[:, 1, :] = [[0, 100], [5, 6], [99, 100], [0, 0], [0, 0], [0, 0]]
    rg[:, 2, :] = [[30, 31], [31, 32], [95, 250], [60, 60], [-9, 2], [0, 0]]
    return Q, K, V, rg


def g9_scores(S):
    return _rng(9, S).random((1, S, 2, (S + 63) // 64), dtype=np.float32)


def g9_scores_small(S, S_sel):
    return _rng(90, S).random((2, S, 2, S_sel), dtype=np.float32)


# g10: m7c shape (G2 h6 D64, l32 d16 l'64 n16); sampled rows: first 130, every 997th, last 64
def g10_rows(S):
    ts = sorted(set(list(range(0, min(130, S))) + list(range(0, S, 997)) + list(range(max(0, S - 64), S))))
    return np.array(ts, np.int32)


def g10_q_kcmp(S, ts, G=2, h=6, D=64):
    S_cmp = (S - 32) // 16 + 1
    Kc = randn(_rng(10, S, 1), 1, G, S_cmp, D)
    Qr = randn(_rng(10, S, 2), 1, len(ts), G, h, D)
    return Qr, Kc


def g10_kv(S, G=2, D=64):
    r = _rng(10, S, 3)
    return randn(r, 1, G, S, D), randn(r, 1, G, S, D)


def g11_inputs(ci, S, G, h, D, S_cmp):
    r = _rng(11, ci)
    B = 2 if S <= 512 else 1
    return (randn(r, B, S, G, h, D), randn(r, B, G, S_cmp, D), randn(r, B, G, S, D), randn(r, B, G, S, D))


# g19: the reference NSAAttention module at the m7c_125m head geometry (oracle/make_m7c_module_goldens.py).  Weights and inputs are
# regenerated from PCG64 streams on both sides (a 768-wide state dict is 7 MB: too big to commit) and are bf16-representable, so the
# fp32 reference and a bf16 module see identical parameters and activations at the layer input.
G19_CFG = dict(dim=768, n_heads=12, n_kv_groups=2, d_k=64, d_v=64, l=32, d=16, l_sel=64, n_sel=16, w=512)
G19_S_PRE, G19_N_DEC, G19_B = 4096, 2200, 1


def _bf16_round(a):
    """fp32 array rounded to the nearest bf16 value (ties to even), still stored as fp32"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def g19_state(names_shapes):
    """names_shapes: [(state-dict key, shape)] in the reference module's own order -> {key: fp32 array (bf16-representable)}"""
    out = {}
    for i, (name, shape) in enumerate(names_shapes):
        shape = tuple(int(x) for x in shape)
        r = _rng(19, i)
        if len(shape) == 2:
            w = randn(r, *shape) / np.float32(np.sqrt(shape[1]))
        else:
            w = randn(r, *shape) * np.float32(0.02)
        out[name] = _bf16_round(w)
    return out


def g19_inputs():
    r = _rng(19, 1000)
    x_pre = _bf16_round(randn(r, G19_B, G19_S_PRE, G19_CFG["dim"]))
    x_dec = _bf16_round(randn(r, G19_N_DEC, G19_B, 1, G19_CFG["dim"]))
    return x_pre, x_dec


def g19_rows():
    """prefill rows / decode steps whose outputs the fixture keeps"""
    pre = np.unique(np.concatenate([np.arange(0, 200, 7), np.arange(200, G19_S_PRE - 96, 29), np.arange(G19_S_PRE - 96, G19_S_PRE)]))
    dec = np.unique(np.concatenate([np.arange(0, 100, 9), np.arange(100, G19_N_DEC - 40, 37), np.arange(G19_N_DEC - 40, G19_N_DEC)]))
    return pre.astype(np.int64), dec.astype(np.int64)


# g20: the reference NSAAttention module at BASELINE configs[0]'s exact shape = the CLI defaults of bench/bench_decode.py:63-72 (dim 256, 8 heads,
# G 2 -> h 4, d_k = d_v 32, l 32, d 16, l' 64, n 16, w 512), context 512 + 32 decode steps (oracle/make_m7c_module_goldens.py, second case).
# Weights / inputs by the g19 recipe (bf16-representable PCG64 streams, regenerated on both sides).
G20_CFG = dict(dim=256, n_heads=8, n_kv_groups=2, d_k=32, d_v=32, l=32, d=16, l_sel=64, n_sel=16, w=512)
G20_S_PRE, G20_N_DEC, G20_B = 512, 512 + 32, 1


def g20_state(names_shapes):
    out = {}
    for i, (name, shape) in enumerate(names_shapes):
        shape = tuple(int(x) for x in shape)
        r = _rng(20, i)
        w = randn(r, *shape) / np.float32(np.sqrt(shape[1])) if len(shape) == 2 else randn(r, *shape) * np.float32(0.02)
        out[name] = _bf16_round(w)
    return out


def g20_inputs():
    r = _rng(20, 1000)
    x_pre = _bf16_round(randn(r, G20_B, G20_S_PRE, G20_CFG["dim"]))
    x_dec = _bf16_round(randn(r, G20_N_DEC, G20_B, 1, G20_CFG["dim"]))
    return x_pre, x_dec


def topn_gap(p_row, t, n_top=16, l_sel=64):
    """gap between the last picked and the first rejected ranking key of one score row at token t (fp32 keys p - idx * 1e-8 as
    nsa/core/selection_scorer.py:182-184 forms them; candidates = complete blocks minus the forced ones 0, t // l', t // l' - 1);
    inf when nothing is rejected"""
    S_sel = p_row.shape[-1]
    nvalid = min(S_sel, (t + 1) // l_sel)
    key = (np.asarray(p_row, np.float32) - np.arange(S_sel, dtype=np.float32) * np.float32(1e-8)).astype(np.float32)
    ok = np.zeros(S_sel, bool)
    ok[:nvalid] = True
    cb = t // l_sel
    for f in (0, cb, max(cb - 1, 0)):
        if f < S_sel:
            ok[f] = False
    k = np.sort(key[ok])[::-1]
    kk = n_top - 3
    return float(k[kk - 1] - k[kk]) if kk >= 1 and k.size > kk else float("inf")


# g21: the gate MLP + three-branch mix of the reference module (oracle/make_gate_goldens.py).  Per case: Q [1,S,G,h,Dk] (post-RoPE query
# rows of S tokens, G = 2 groups), the three branch outputs O_cmp / O_sel / O_win [1,S,G,h,Dv], the gate weights fc1 [Hd,Dk] + bias,
# fc2 [3,Hd] + bias and a seeded upstream gradient dO; every value bf16-representable.  fc2 is scaled so the gates of a row span roughly
# 0.05-0.9 (non-saturated, clearly non-uniform, each branch winning some rows); its bias shifts the three logits apart.  The first
# G21_RD rows carry the dense outputs (O and the autograd gradients) in the fixture; every row carries its gates.
G21_CASES = {  # name: (Dk, h, hidden, Dv, tau, fc2 gain, fc2 bias[, shift of the sel row of fc2 (peaked: half the rows beyond the gap 50)])
    "m7c": (64, 6, 32, 64, 1.0, 1.0, (0.0, 0.4, -0.3)),
    "boundary": (64, 8, 32, 64, 0.7, 0.8, (0.3, -0.2, 0.0)),
    "wide_hidden": (64, 6, 64, 64, 2.0, 2.0, (-0.3, 0.0, 0.5)),
    "many_heads": (64, 12, 32, 64, 1.0, 1.0, (0.0, 0.2, -0.2)),
    "d128": (128, 6, 64, 128, 1.0, 1.0, (0.2, 0.0, -0.2)),
    "tiny": (16, 4, 8, 16, 1.0, 1.0, (0.0, 0.3, -0.3)),
    "odd_split": (40, 3, 20, 32, 1.0, 1.0, (-0.2, 0.3, 0.0)),
    "peaked": (64, 6, 32, 64, 1.0, 2.0, (0.0, 50.0, 0.0), 7.0),
    "clamp": (64, 6, 32, 64, 0.0, 1.0, (0.0, 0.0, 0.0)),
}
G21_S, G21_G, G21_RD = 48, 2, 6


def g21_inputs(case):
    """-> dict of fp32 arrays (bf16-representable) + scalars for one g21 case"""
    Dk, h, Hd, Dv, tau, gain, bias = G21_CASES[case][:7]
    shift = G21_CASES[case][7] if len(G21_CASES[case]) > 7 else 0.0
    r = _rng(21, list(G21_CASES).index(case))
    S, G = G21_S, G21_G
    q = _bf16_round(randn(r, 1, S, G, h, Dk))
    oc, os_, ow = (_bf16_round(randn(r, 1, S, G, h, Dv)) for _ in range(3))
    w1 = _bf16_round(randn(r, Hd, Dk) * np.float32(2.0 / np.sqrt(Dk) * np.sqrt(h)))
    b1 = _bf16_round(randn(r, Hd) * np.float32(0.1))
    w2 = randn(r, 3, Hd) * np.float32(gain * 1.2 / np.sqrt(Hd))
    w2[1] += np.float32(shift / Hd)
    w2 = _bf16_round(w2)
    b2 = _bf16_round(np.asarray(bias, np.float32))
    dO = _bf16_round(randn(r, 1, S, G, h, Dv))
    return dict(Q=q, O_cmp=oc, O_sel=os_, O_win=ow, w1=w1, b1=b1, w2=w2, b2=b2, dO=dO, tau=float(tau), h=h, Dk=Dk, Dv=Dv, Hd=Hd)


# g22: RoPE and the compressed-token pooling of the reference (oracle/make_rope_pool_goldens.py).  Every value is a multiple of 1/32 below 8
# in magnitude (8 significant bits), so it is exact in bf16 AND fp16 and each case runs in fp32, bf16 and fp16 on the same numbers.
G22_POS_LONG = (2047, 2048, 4095, 32767, 65535, 65536, 131071, 262143)
G22_DTYPES = ("fp32", "bf16", "fp16")
# RoPE cases: name -> (D, scale, positions, with gradient).  384 / 768 / 1536 are flattened Q widths (n_heads d_k); "dense" = 0 .. 299.
G22_ROPE_CASES = {
    "d16_dense_s1": (16, 1.0, "dense", False),
    "d16_dense_s3": (16, 3.0, "dense", True),
    "d16_dense_s4": (16, 4.0, "dense", False),
    **{f"d{D}_long_s{s}": (D, float(s), G22_POS_LONG, D in (64, 384)) for D in (16, 32, 64, 128) for s in (1, 4, 3)},
    **{f"d384_long_s{s}": (384, float(s), G22_POS_LONG, s == 3) for s in (1, 3)},
    **{f"d768_long_s{s}": (768, float(s), G22_POS_LONG[3::2] + (65536,), False) for s in (1, 3)},
    **{f"d1536_long_s{s}": (1536, float(s), (65536, 262143), False) for s in (1, 3)},
}
# pooling cases: name -> (l, d, D = Dk = Dv, S, first position, windows stored (None = all), with gradient).  Position offset p0 > 0 with
# S = l is a decode emission (pos = arange(S_raw - l, S_raw), reference nsa_attention.py:586-604).
G22_POOL_CASES = {}
for _l, _d in ((32, 16), (16, 8), (32, 32), (64, 16), (24, 8)):
    for _D in (32, 64, 128):
        for _S in (_l - 1, _l, _l + _d - 1):
            G22_POOL_CASES[f"l{_l}d{_d}_D{_D}_S{_S}"] = (_l, _d, _D, _S, 0, None, False)
        G22_POOL_CASES[f"l{_l}d{_d}_D{_D}_S4101"] = (_l, _d, _D, 4101, 0, "ends", False)
        G22_POOL_CASES[f"l{_l}d{_d}_D{_D}_dec65568"] = (_l, _d, _D, _l, 65568, None, False)
    G22_POOL_CASES[f"l{_l}d{_d}_D64_dec262112"] = (_l, _d, 64, _l, 262112, None, False)
    G22_POOL_CASES[f"l{_l}d{_d}_D32_grad"] = (_l, _d, 32, _l + _d + 5, 0, None, True)  # two windows, then 5 rows after the last
G22_POOL_CASES["l32d16_D32_grad_off"] = (32, 16, 32, 32 + 16 + 5, 65568, None, True)


def g22_pool_windows(case):
    """indices of the compressed tokens stored for a pooling case ("ends": the first 2 and the last 2 of a long run)"""
    l, d, _, S, _, rows, _ = G22_POOL_CASES[case]
    n = 0 if S < l else (S - l) // d + 1
    return np.arange(n) if rows is None else np.array([0, 1, n - 2, n - 1])


def _g22_vals(r, *shape):
    return (np.clip(np.rint(randn(r, *shape) * np.float32(32.0)), -255, 255) / np.float32(32.0)).astype(np.float32)


def g22_inputs(case):
    """-> dict: RoPE case: x [R,D], pos [R] int64, dy [R,D] (upstream gradient); pooling case: K [1,1,S,D], V [1,1,S,D], pos [S],
    dKc / dVc [1,1,n_cmp,D]"""
    if case in G22_ROPE_CASES:
        D, _, pos, _ = G22_ROPE_CASES[case]
        r = _rng(22, 0, list(G22_ROPE_CASES).index(case))
        p = np.arange(300, dtype=np.int64) if pos == "dense" else np.asarray(pos, np.int64)
        return dict(x=_g22_vals(r, p.size, D), pos=p, dy=_g22_vals(r, p.size, D))
    l, d, D, S, p0, _, _ = G22_POOL_CASES[case]
    r = _rng(22, 1, list(G22_POOL_CASES).index(case))
    n = 0 if S < l else (S - l) // d + 1
    return dict(K=_g22_vals(r, 1, 1, S, D), V=_g22_vals(r, 1, 1, S, D), pos=np.arange(p0, p0 + S, dtype=np.int64),
                dKc=_g22_vals(r, 1, 1, n, D), dVc=_g22_vals(r, 1, 1, n, D))


def g22_unpack(a):
    """a stored g22 output -> float32 (bf16 is stored as its uint16 bit pattern)"""
    if a.dtype == np.uint16:
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)
