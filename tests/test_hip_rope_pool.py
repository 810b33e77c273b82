"""GPU: RoPE + cache append and the compressed-token pooling, forward and backward, in every kernel that carries them, against the oracle
(nsa_oracle_rope / _bwd, nsa_oracle_cmp_pool / _bwd), which tests/test_oracle_golden.py pins to the REFERENCE (g22,
oracle/make_rope_pool_goldens.py):
  * nsa_rope_cache_append (rope_cache_append_kernel): t0 up to 262000, S > 2048 (the grid's position loop), B up to 70 (batch slices);
  * nsa_cmp_pool_append: cmp_pool_wide_kernel and cmp_pool_kernel (l <= 32 unrolled, l > 32 loop, Dv = 128), windows beyond 65536, j0 > 0,
    a position scale that must not reach the pooled keys;
  * nsa_rope_cache_append_bwd (null cache gradients, S B > 2048 rows) and nsa_cmp_pool_bwd (n_cmp = 0, rows after the last window, l = 24);
  * the layer: prefill, extend, decode in every projection form (qkv_rope_append_fast_kernel for B <= 2, linear_mfma_kernel<ROPE> for
    B >= 3 and B > 64, qkv_rope_append_kernel for fp32), a step at t = 65535, NSA_ROPE_SCALE = 3, and the training ops _RopeAppendFn /
    _CmpPoolFn.

Every comparison uses the per-element float64 bound of nsa_oracle.rope_bound (derivation in oracle/nsa_oracle.py): |x| angle_err + c ulp_T(|x|)
for the rotated pair (x0, x1), angle_err = a 2^-22 + 2 ulp32(a) + 2^-22 at the fp32 angle a = (p / s) f_i, c = 6 (bf16, fp16) or 8 (fp32).
A wrong frequency, position, scale or rotation width errs by ~|x| f_i p: order |x| on the high-frequency pairs, far above the bound.
Copies (V, raw K) must be exact; rows the call does not own must be untouched.  The worst error / bound ratio seen on the MI355X is
recorded in each test's docstring (printed under -s).  Each of six hand-made kernel mutations (Q rotated per head, a position scale in
the pooling, a dropped window in the pooling backward, the backward rotation's sign, decode position t0 + 1, the unrolled pooling's last
row) made a test here fail by a factor of 30 to 200 over its bound."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENT = -3.5  # sentinel of the rows a call must not write (exact in every dtype)


def _vals(rng, *shape):
    """multiples of 1/32 below 8: exact in bf16 and fp16"""
    return (np.clip(np.rint(rng.standard_normal(shape) * 32.0), -255, 255) / 32.0).astype(np.float32)


def _ratio(got, ref, bound):
    e = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    assert np.isfinite(e).all()
    assert (e[bound == 0] == 0).all(), "an element that must be exact is not"
    return float((e / np.where(bound > 0, bound, 1.0)).max()) if e.size else 0.0


def _np(t):
    return t.detach().float().cpu().numpy()


def _desc(dt, G, h, Dk, Dv, l=32, d=16, scale=1.0):
    from nsa_vibe_amd import _lib

    ds = _lib.NsaLayerDesc()
    ds.dim, ds.G, ds.h, ds.Dk, ds.Dv = G * h * Dv, G, h, Dk, Dv
    ds.l, ds.d, ds.l_sel, ds.n_sel, ds.w = l, d, 64, 16, 512
    ds.gate_hidden, ds.dtype, ds.gate_tau = 8, _lib.NSA_DT_F32 if dt == "fp32" else (_lib.NSA_DT_BF16 if dt == "bf16" else _lib.NSA_DT_F16), 1.0
    ds.rope_base, ds.rope_scale = 10000.0, float(scale)
    return ds


class _Cache:
    """the eight cache buffers [B,G,S_max,D] / [B,G,n_cmp_max,D] filled with the sentinel, and their nsa_kv_desc"""

    def __init__(self, dt, B, G, Dk, Dv, S_max, n_cmp_max):
        from nsa_vibe_amd import _lib

        mk = lambda n, D: torch.full((B, G, n, D), SENT, dtype=DT[dt], device="cuda")  # noqa: E731
        self.t = {k: mk(S_max, Dk if k[0] == "K" else Dv) for k in ("K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw")}
        self.t["K_cmp"], self.t["V_cmp"] = mk(n_cmp_max, Dk), mk(n_cmp_max, Dv)
        self.kd = _lib.NsaKvDesc()
        for k, v in self.t.items():
            setattr(self.kd, k, v.data_ptr())
        self.kd.B, self.kd.S_max, self.kd.n_cmp_max = B, S_max, n_cmp_max


def _check_untouched(buf, lo, hi):
    """rows outside [lo, hi) of a [B,G,N,D] buffer still hold the sentinel (checked on the device)"""
    assert bool((buf[:, :, :lo] == SENT).all()) and bool((buf[:, :, hi:] == SENT).all())


# ---- nsa_rope_cache_append -------------------------------------------------------------------------------------------------------------
# (G, h, Dk, Dv): m7c, the D = 128 layer (12 heads), D = 32
GEOM = {"m7c": (2, 6, 64, 64), "d128": (2, 6, 128, 128), "d32": (2, 4, 32, 32)}
APPEND = [  # geometry, t0, S, B, scale, dtype
    ("m7c", 0, 300, 1, 1.0, "bf16"), ("m7c", 5, 2049, 1, 3.0, "fp16"), ("m7c", 65530, 300, 1, 1.0, "fp32"),
    ("m7c", 262000, 300, 1, 3.0, "bf16"), ("m7c", 5, 1, 70, 1.0, "bf16"), ("m7c", 0, 300, 3, 3.0, "fp32"),
    ("d128", 65530, 300, 1, 1.0, "bf16"), ("d128", 0, 2049, 1, 3.0, "fp32"), ("d128", 262000, 1, 1, 3.0, "fp16"),
    ("d32", 262000, 1, 1, 1.0, "fp16"), ("d32", 5, 300, 3, 1.0, "bf16"), ("d32", 0, 1, 70, 3.0, "fp32"),
]


def _expect_append(orc, proj, G, h, Dk, Dv, pos, dt, scale):
    """the seven outputs of RoPE + append from the oracle: Q [B,S,NQ] rotated over the flattened NQ width, K_sel / K_win [B,G,S,Dk]
    rotated per group, the rest copied -- with their bounds (0 for the copies)"""
    B, S, _ = proj.shape
    NQ, GK, GV = G * h * Dk, G * Dk, G * Dv
    cut = np.cumsum([0, NQ, GK, GV, GK, GV, GK, GV])
    parts = [proj[..., cut[i]: cut[i + 1]] for i in range(7)]
    out = {"Q": (orc.rope(parts[0], pos, dt, scale), orc.rope_bound(parts[0], pos, dt, scale))}
    for i, k in enumerate(("K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw"), start=1):
        D = Dk if k[0] == "K" else Dv
        p = np.ascontiguousarray(parts[i].reshape(B, S, G, D).transpose(0, 2, 1, 3))
        out[k] = (orc.rope(p, pos, dt, scale), orc.rope_bound(p, pos, dt, scale)) if k in ("K_sel", "K_win") else (p, np.zeros_like(p))
    return out


@pytest.mark.parametrize("geom,t0,S,B,scale,dt", APPEND, ids=[f"{g}-t{t}-S{s}-B{b}-s{int(c)}-{d}" for g, t, s, b, c, d in APPEND])
def test_rope_cache_append_matches_oracle(orc, geom, t0, S, B, scale, dt):
    """Q and all six cache slices against the oracle; V and raw K copied unrotated; rows outside [t0, t0 + S) untouched.
    Worst error / bound seen on the MI355X: 0.70 (D 128, S 2049, fp32), 0.33 (bf16 at t0 = 262000), 0.33 (fp16)."""
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _stream

    G, h, Dk, Dv = GEOM[geom]
    NT = G * h * Dk + 3 * G * Dk + 3 * G * Dv
    rng = np.random.default_rng([22, t0, S, B, Dk])
    proj = _vals(rng, B, S, NT)
    c = _Cache(dt, B, G, Dk, Dv, t0 + S + 8, 1)
    P = torch.from_numpy(proj).to(DT[dt]).cuda()
    Q = torch.full((B, S, G, h, Dk), SENT, dtype=DT[dt], device="cuda")
    ds = _desc(dt, G, h, Dk, Dv, scale=scale)
    _lib.check(_lib.lib().nsa_rope_cache_append(ctypes.byref(ds), ctypes.byref(c.kd), P.data_ptr(), Q.data_ptr(), S, t0, _stream(P.device)),
               "nsa_rope_cache_append")
    torch.cuda.synchronize()
    pos = np.arange(t0, t0 + S)
    exp = _expect_append(orc, proj, G, h, Dk, Dv, pos, dt, scale)
    worst = _ratio(_np(Q).reshape(B, S, -1), *exp["Q"])
    for k in ("K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw"):
        worst = max(worst, _ratio(_np(c.t[k][:, :, t0: t0 + S]), *exp[k]))
        _check_untouched(c.t[k], t0, t0 + S)
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


# ---- nsa_cmp_pool_append ---------------------------------------------------------------------------------------------------------------
POOL = [  # l, d, D (= Dk = Dv), B, j0, j1, scale in the descriptor, dtype; the leg in the id
    (32, 16, 64, 1, 0, 255, 1.0, "bf16", "wide"),
    (32, 16, 64, 1, 0, 600, 3.0, "fp16", "narrow-unrolled"),
    (64, 16, 64, 1, 0, 600, 1.0, "bf16", "narrow-loop"),
    (64, 16, 128, 1, 3, 10, 3.0, "fp32", "narrow-loop-Dv128"),
    (32, 16, 128, 1, 2, 9, 1.0, "bf16", "wide-Dv128"),
    (24, 8, 32, 1, 8194, 8200, 1.0, "fp16", "wide-l24-past65536"),
    (24, 8, 32, 1, 8194, 8794, 3.0, "bf16", "narrow-l24-past65536"),
    (32, 32, 64, 2, 2049, 2051, 3.0, "fp32", "wide-past65536"),
    (16, 8, 64, 3, 5, 700, 3.0, "bf16", "narrow-B3"),
]


@pytest.mark.parametrize("l,d,D,B,j0,j1,scale,dt,leg", POOL, ids=[p[-1] + "-" + p[-2] for p in POOL])
def test_cmp_pool_append_matches_oracle(orc, l, d, D, B, j0, j1, scale, dt, leg):
    """compressed tokens [j0, j1) against the oracle pooling of the raw cache at its absolute positions (no position scale: a descriptor
    with rope_scale = 3 must give the same keys); compressed rows outside [j0, j1) untouched.  Worst error / bound seen on the MI355X: 0.091 (fp32, windows past 65536)."""
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _stream

    G = 2
    S_max = (j1 - 1) * d + l + 5
    c = _Cache(dt, B, G, D, D, S_max, j1 + 4)
    rng = np.random.default_rng([22, 7, l, d, D, j0])
    r0, r1 = j0 * d, (j1 - 1) * d + l
    K, V = _vals(rng, B, G, r1 - r0, D), _vals(rng, B, G, r1 - r0, D)
    c.t["K_raw"][:, :, r0: r1] = torch.from_numpy(K).to(DT[dt]).cuda()
    c.t["V_raw"][:, :, r0: r1] = torch.from_numpy(V).to(DT[dt]).cuda()
    ds = _desc(dt, G, 2, D, D, l=l, d=d, scale=scale)
    _lib.check(_lib.lib().nsa_cmp_pool_append(ctypes.byref(ds), ctypes.byref(c.kd), j0, j1, _stream(c.t["K_raw"].device)), "nsa_cmp_pool_append")
    torch.cuda.synchronize()
    pos = np.arange(r0, r1)
    oK, oV = orc.cmp_pool(K, V, l, d, pos, dt)
    bK, bV = orc.cmp_pool_bound(K, V, l, d, pos, dt)
    assert oK.shape[-2] == j1 - j0
    worst = max(_ratio(_np(c.t["K_cmp"][:, :, j0: j1]), oK, bK), _ratio(_np(c.t["V_cmp"][:, :, j0: j1]), oV, bV))
    _check_untouched(c.t["K_cmp"], j0, j1)
    _check_untouched(c.t["V_cmp"], j0, j1)
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


# ---- backward kernels ------------------------------------------------------------------------------------------------------------------
APPEND_BWD = [  # geometry, t0, S, B, scale, dtype, gradients left null
    ("m7c", 0, 300, 1, 1.0, "bf16", ("V_sel", "V_win", "V_raw")),
    ("d128", 65530, 2049, 1, 3.0, "fp32", ()),
    ("d32", 5, 700, 3, 1.0, "fp16", ("V_sel", "K_raw")),
    ("m7c", 262000, 64, 2, 3.0, "bf16", ("V_win",)),
]


@pytest.mark.parametrize("geom,t0,S,B,scale,dt,null", APPEND_BWD, ids=[f"{a[0]}-t{a[1]}-S{a[2]}-B{a[3]}-{a[5]}" for a in APPEND_BWD])
def test_rope_cache_append_bwd_matches_oracle(orc, geom, t0, S, B, scale, dt, null):
    """dproj against the oracle's rotation backward (Q over NQ, K_sel / K_win per group) and copies; a null cache gradient gives exactly 0.
    Worst error / bound seen on the MI355X: 0.63 (D 128, t0 65530, fp32), 0.33 (fp16), 0.30 (bf16)."""
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _stream

    G, h, Dk, Dv = GEOM[geom]
    NQ, GK, GV = G * h * Dk, G * Dk, G * Dv
    rng = np.random.default_rng([22, 9, t0, S, B])
    dQ = _vals(rng, B, S, G, h, Dk)
    names = ("K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw")
    grads = {k: None if k in null else _vals(rng, B, G, S, Dk if k[0] == "K" else Dv) for k in names}
    dev = {k: None if v is None else torch.from_numpy(v).to(DT[dt]).cuda() for k, v in grads.items()}
    tQ = torch.from_numpy(dQ).to(DT[dt]).cuda()
    dproj = torch.full((B, S, NQ + 3 * GK + 3 * GV), SENT, dtype=DT[dt], device="cuda")
    ds = _desc(dt, G, h, Dk, Dv, scale=scale)
    _lib.check(_lib.lib().nsa_rope_cache_append_bwd(ctypes.byref(ds), B, S, t0, tQ.data_ptr(), *(None if dev[k] is None else dev[k].data_ptr()
                                                                                                   for k in names), dproj.data_ptr(),
                                                    _stream(tQ.device)), "nsa_rope_cache_append_bwd")
    torch.cuda.synchronize()
    got = _np(dproj)
    pos = np.arange(t0, t0 + S)
    worst = _ratio(got[..., :NQ], orc.rope_bwd(dQ.reshape(B, S, NQ), pos, dt, scale), orc.rope_bound(dQ.reshape(B, S, NQ), pos, dt, scale))
    col = NQ
    for k in names:
        D = Dk if k[0] == "K" else Dv
        g = got[..., col: col + G * D].reshape(B, S, G, D).transpose(0, 2, 1, 3)
        col += G * D
        if grads[k] is None:
            assert (g == 0).all(), k
        elif k in ("K_sel", "K_win"):
            worst = max(worst, _ratio(g, orc.rope_bwd(grads[k], pos, dt, scale), orc.rope_bound(grads[k], pos, dt, scale)))
        else:
            assert np.array_equal(g, grads[k]), k
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


POOL_BWD = [  # l, d, D, B, S, n_cmp, dtype
    (32, 16, 64, 1, 101, 5, "bf16"), (32, 16, 64, 2, 101, 3, "fp32"), (24, 8, 32, 1, 77, 6, "fp16"), (24, 8, 64, 2, 77, 6, "bf16"),
    (64, 16, 128, 1, 150, 6, "fp32"), (32, 32, 32, 1, 100, 3, "bf16"), (32, 16, 64, 1, 50, 0, "bf16"), (16, 8, 32, 1, 20, 0, "fp16"),
]


@pytest.mark.parametrize("l,d,D,B,S,n_cmp,dt", POOL_BWD, ids=[f"l{a[0]}d{a[1]}-D{a[2]}-B{a[3]}-S{a[4]}-n{a[5]}-{a[6]}" for a in POOL_BWD])
def test_cmp_pool_bwd_matches_oracle(orc, l, d, D, B, S, n_cmp, dt):
    """dK_raw / dV_raw against the oracle pooling backward; rows after the last window and every row of n_cmp = 0 get exactly 0.
    Worst error / bound seen on the MI355X: 0.35 (l 64, fp32), 0.25 (l 24)."""
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _stream

    G = 2
    rng = np.random.default_rng([22, 11, l, d, S, n_cmp])
    dKc, dVc = _vals(rng, B, G, n_cmp, D), _vals(rng, B, G, n_cmp, D)
    tK, tV = (torch.from_numpy(a).to(DT[dt]).cuda() for a in (dKc, dVc))
    dKr = torch.full((B, G, S, D), SENT, dtype=DT[dt], device="cuda")
    dVr = torch.full((B, G, S, D), SENT, dtype=DT[dt], device="cuda")
    ds = _desc(dt, G, 2, D, D, l=l, d=d, scale=3.0)  # (no position scale inside the pooling: the descriptor's must not matter)
    _lib.check(_lib.lib().nsa_cmp_pool_bwd(ctypes.byref(ds), B, S, n_cmp, tK.data_ptr() if n_cmp else None, tV.data_ptr() if n_cmp else None,
                                           dKr.data_ptr(), dVr.data_ptr(), _stream(tK.device)), "nsa_cmp_pool_bwd")
    torch.cuda.synchronize()
    oK, oV = orc.cmp_pool_bwd(dKc, dVc, S, l, d, None, dt)
    bK, bV = orc.cmp_pool_bwd_bound(dKc, dVc, S, l, d, None, dt)
    gK, gV = _np(dKr), _np(dVr)
    last = (n_cmp - 1) * d + l if n_cmp else 0
    assert last < S and (gK[:, :, last:] == 0).all() and (gV[:, :, last:] == 0).all()
    worst = max(_ratio(gK, oK, bK), _ratio(gV, oV, bV))
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


# ---- the layer -------------------------------------------------------------------------------------------------------------------------
def _layer(dt, H=12, dk=64, monkeypatch=None, scale=None, prefill_tile=0):
    from nsa_vibe_amd.nsa_attention import NSAAttention

    if scale is not None:
        monkeypatch.setenv("NSA_ROPE_SCALE", str(scale))
    torch.manual_seed(22)
    m = NSAAttention(768, H, 2, dk, dk, l=32, d=16, l_sel=64, n_sel=16, w=512, prefill_tile=prefill_tile)
    return m.cuda().to(DT[dt]).eval()


def _proj64(m, x):
    """the fused projection in float64 from the layer's own (dtype) x and weights, rounded to the dtype, and a bound on the kernel's
    projection error: 1 ulp of the dtype (the GEMM's rounding) + dim 2^-23 sum |x w| (its fp32 accumulation)"""
    W = torch.cat([getattr(m, n).weight.detach() for n in m._QKV], 0).double()
    xd = x.detach().double()
    p = xd @ W.t()
    acc = xd.abs() @ W.abs().t() * (x.shape[-1] * 2.0 ** -23)
    dt = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[x.dtype]
    from oracle import nsa_oracle as orc

    pr = p.to(x.dtype).float().cpu().numpy()
    return pr, orc.ulp(pr, dt) + acc.cpu().numpy()


def _check_layer_rows(orc, m, kv, x, t0, dt, scale=1.0):
    """the six cache slices of rows [t0, t0 + S) against the oracle on the float64 projection of x [B,S,dim]; a pair's bound grows by the
    projection error of its two inputs (rotated: |e0| + |e1| on each output)"""
    B, S, _ = x.shape
    G, h, Dk, Dv = m.n_kv_groups, m.h_per_group, m.d_k, m.d_v
    proj, pe = _proj64(m, x)
    pos = np.arange(t0, t0 + S)
    exp = _expect_append(orc, proj, G, h, Dk, Dv, pos, dt, scale)
    NQ, GK, GV = G * h * Dk, G * Dk, G * Dv
    cut = np.cumsum([0, NQ, GK, GV, GK, GV, GK, GV])
    worst = 0.0
    for i, k in enumerate(("K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw"), start=1):
        D = Dk if k[0] == "K" else Dv
        e = np.ascontiguousarray(pe[..., cut[i]: cut[i + 1]].reshape(B, S, G, D).transpose(0, 2, 1, 3))
        if k in ("K_sel", "K_win"):
            e = np.repeat(e[..., 0::2] + e[..., 1::2], 2, axis=-1)
        ref, b = exp[k]
        worst = max(worst, _ratio(_np(getattr(kv, "_" + k)[:, :, t0: t0 + S]), ref, b + e))
    return worst


def _check_cmp(orc, m, kv, j0, j1, dt):
    """compressed rows [j0, j1) against the oracle pooling of the layer's own raw cache (no position scale)"""
    l, d = m.l, m.d
    r0, r1 = j0 * d, (j1 - 1) * d + l
    K, V = _np(kv._K_raw[:, :, r0: r1]), _np(kv._V_raw[:, :, r0: r1])
    pos = np.arange(r0, r1)
    oK, oV = orc.cmp_pool(K, V, l, d, pos, dt)
    bK, bV = orc.cmp_pool_bound(K, V, l, d, pos, dt)
    return max(_ratio(_np(kv._K_cmp[:, :, j0: j1]), oK, bK), _ratio(_np(kv._V_cmp[:, :, j0: j1]), oV, bV))


def _kv(m, B, S_max, dt):
    from nsa_vibe_amd.kv_cache import NSA_KV

    return NSA_KV(B, m.n_kv_groups, m.d_k, m.d_v, S_max, m.l, m.d, m.l_sel, m.n_sel, m.w, "cuda", DT[dt])


def _x(B, S, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, 768, generator=g).to(DT[dt]).cuda()


def _n(S, l=32, d=16):
    return 0 if S < l else (S - l) // d + 1


@pytest.mark.parametrize("S,dt,scale", [(31, "bf16", None), (4101, "bf16", None), (4101, "fp16", 3.0)])
def test_layer_prefill_caches(orc, monkeypatch, S, dt, scale):
    """the one-call prefill (nsa_layer_prefill: rope_cache_append + cmp_pool) leaves caches that match the oracle on the float64
    projection; NSA_ROPE_SCALE = 3 scales K_sel / K_win but not the pooled keys.  Worst error / bound seen on the MI355X: 0.89 (S 4101, bf16: the
    projection's ulp dominates), 0.52 (NSA_ROPE_SCALE = 3, fp16)."""
    m = _layer(dt, monkeypatch=monkeypatch, scale=scale)
    x = _x(1, S, dt, S)
    kv = _kv(m, 1, S, dt)
    with torch.no_grad():
        m(x, kv, prefill=True)
    torch.cuda.synchronize()
    assert kv.t == S and kv.n_cmp == _n(S)
    worst = _check_layer_rows(orc, m, kv, x, 0, dt, scale or 1.0)
    if kv.n_cmp:
        worst = max(worst, _check_cmp(orc, m, kv, 0, kv.n_cmp, dt))
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


def test_layer_extend_caches(orc):
    """extend onto a filled cache in tiles of 100 rows (d = 16: windows straddle the chunk boundaries).  Worst error / bound seen on the MI355X:
    0.67."""
    dt = "bf16"
    m = _layer(dt, prefill_tile=100)
    x = _x(1, 340, dt, 3)
    kv = _kv(m, 1, 340, dt)
    with torch.no_grad():
        m.prefill_tile = 0
        m(x[:, :40], kv, prefill=True)
        m.prefill_tile = 100
        m(x[:, 40:], kv, prefill=True)
    torch.cuda.synchronize()
    assert kv.t == 340 and kv.n_cmp == _n(340)
    worst = max(_check_layer_rows(orc, m, kv, x[:, 40:], 40, dt), _check_cmp(orc, m, kv, _n(40), _n(340), dt))
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


DECODE = [(1, "bf16", None), (2, "fp16", None), (3, "bf16", None), (70, "bf16", None), (1, "fp32", None), (3, "fp32", 3.0), (2, "bf16", 3.0)]


@pytest.mark.parametrize("B,dt,scale", DECODE, ids=[f"B{b}-{d}" + (f"-s{int(s)}" if s else "") for b, d, s in DECODE])
def test_layer_decode_caches(orc, monkeypatch, B, dt, scale):
    """decode steps 40 .. 79 (emissions at 48, 64, 80 raw tokens) in each projection form: qkv_rope_append_fast_kernel (bf16 / fp16, B <= 2),
    linear_mfma_kernel<ROPE> (B >= 3; B = 70 > 64 takes a second row tile), qkv_rope_append_kernel (fp32).  Worst error / bound seen on the
    MI355X: 0.80 (B 70), 0.67 (B 3), 0.33 (B 1-2), 0.07 (fp32)."""
    m = _layer(dt, monkeypatch=monkeypatch, scale=scale)
    x = _x(B, 80, dt, B)
    kv = _kv(m, B, 80, dt)
    with torch.no_grad():
        m(x[:, :40], kv, prefill=True)
        for t in range(40, 80):
            m(x[:, t: t + 1], kv, prefill=False)
    torch.cuda.synchronize()
    assert kv.t == 80 and kv.n_cmp == _n(80)
    worst = max(_check_layer_rows(orc, m, kv, x[:, 40:], 40, dt, scale or 1.0), _check_cmp(orc, m, kv, _n(40), _n(80), dt))
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


def test_layer_decode_step_at_65535(orc):
    """one decode step at t = 65535 after the cache rows before it were written directly: the new row is rotated at position 65535 and
    the emission (S_raw = 65536) pools raw rows 65504 .. 65535 at their absolute positions.  Worst error / bound seen on the MI355X: 0.055."""
    dt, t = "bf16", 65535
    m = _layer(dt)
    kv = _kv(m, 1, t + 1, dt)
    g = torch.Generator().manual_seed(5)
    for k in ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw"):
        getattr(kv, k)[:, :, :t] = torch.randn(1, 2, t, 64, generator=g).to(DT[dt]).cuda()
    n_prev = _n(t)
    for k in ("_K_cmp", "_V_cmp"):
        getattr(kv, k)[:, :, :n_prev] = torch.randn(1, 2, n_prev, 64, generator=g).to(DT[dt]).cuda()
    kv.t, kv.n_cmp = t, n_prev
    kv.ensure_meta(t)
    x = _x(1, 1, dt, 65535)
    with torch.no_grad():
        m(x, kv, prefill=False)
    torch.cuda.synchronize()
    assert kv.t == t + 1 and kv.n_cmp == _n(t + 1) == n_prev + 1
    worst = max(_check_layer_rows(orc, m, kv, x, t, dt), _check_cmp(orc, m, kv, n_prev, n_prev + 1, dt))
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("geom,dt", [("m7c", "bf16"), ("d128", "fp32")])
def test_training_rope_and_pool_gradients(orc, geom, dt):
    """_RopeAppendFn + _CmpPoolFn at the layer shapes (m7c; D = 128): the gradient of the fused projection against the oracle backward of
    the rotation (Q, K_sel, K_win), the pooling (K_raw, V_raw through K_cmp / V_cmp) and the copies; V_sel is unused (gradient 0).
    Worst error / bound seen on the MI355X: 0.41 (D 128, fp32), 0.17 (m7c, bf16)."""
    from nsa_vibe_amd.nsa_attention import _CmpPoolFn, _RopeAppendFn

    G, h, Dk, Dv = GEOM[geom]
    S, B = 101, 2
    m = _layer(dt, H=G * h, dk=Dk).train()
    kv = _kv(m, B, S, dt)
    NQ, GK, GV = G * h * Dk, G * Dk, G * Dv
    NT = NQ + 3 * GK + 3 * GV
    rng = np.random.default_rng([22, 13, Dk])
    proj = torch.from_numpy(_vals(rng, B, S, NT)).to(DT[dt]).cuda().requires_grad_(True)
    Q, Ks, Vs, Kw, Vw, Kr, Vr = _RopeAppendFn.apply(proj, m, kv, S)
    kv.t = S
    Kc, Vc = _CmpPoolFn.apply(Kr, Vr, m, kv, S)
    n = _n(S)
    up = {k: _vals(rng, *shape) for k, shape in (("Q", (B, S, G, h, Dk)), ("Ks", (B, G, S, Dk)), ("Kw", (B, G, S, Dk)), ("Vw", (B, G, S, Dv)),
                                                  ("Kc", (B, G, n, Dk)), ("Vc", (B, G, n, Dv)))}
    torch.autograd.backward([Q, Ks, Kw, Vw, Kc, Vc], [torch.from_numpy(up[k]).to(DT[dt]).cuda() for k in ("Q", "Ks", "Kw", "Vw", "Kc", "Vc")])
    got = _np(proj.grad)
    pos = np.arange(S)
    q = up["Q"].reshape(B, S, NQ)
    worst = _ratio(got[..., :NQ], orc.rope_bwd(q, pos, dt), orc.rope_bound(q, pos, dt))
    dKr, dVr = orc.cmp_pool_bwd(up["Kc"], up["Vc"], S, m.l, m.d, None, dt)
    bKr, bVr = orc.cmp_pool_bwd_bound(up["Kc"], up["Vc"], S, m.l, m.d, None, dt)
    col = NQ
    for k, D in (("Ks", Dk), ("Vs", Dv), ("Kw", Dk), ("Vw", Dv), ("Kr", Dk), ("Vr", Dv)):
        g = got[..., col: col + G * D].reshape(B, S, G, D).transpose(0, 2, 1, 3)
        col += G * D
        if k == "Vs":
            assert (g == 0).all()
        elif k in ("Ks", "Kw"):
            worst = max(worst, _ratio(g, orc.rope_bwd(up[k], pos, dt), orc.rope_bound(up[k], pos, dt)))
        elif k == "Vw":
            assert np.array_equal(g, up[k])
        else:
            worst = max(worst, _ratio(g, dKr, bKr) if k == "Kr" else _ratio(g, dVr, bVr))
    print(f"worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst
