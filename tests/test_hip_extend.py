"""Extend route: prefill onto a filled cache / tiled prefill with decode-step semantics (nsa_layer_extend, nsa_sel_scores_rows).

Row t of an extend normalises its compressed scores over the n_cmp(t) compressed tokens a decode step at t sees and selects sequentially,
so S decode steps and one extend of S tokens give the same caches, ranges and outputs (up to the rounding of the different kernel forms),
and the result does not depend on how the tokens are split into chunks.  The reference's decode route is frozen in the g20 (fp32) and g19
(bf16, m7c geometry) goldens: a tiled prefill has to reproduce both.
"""
import copy
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

gpu = pytest.mark.gpu


def _n_cmp(S_raw, l=32, d=16):
    return 0 if S_raw < l else (S_raw - l) // d + 1


def _clone_kv(kv):
    c = copy.copy(kv)
    for name in ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp"):
        setattr(c, name, getattr(kv, name).clone())
    for name in ("reads_pred", "reads_act_total", "reads_act_sel", "reads_act_cmp", "reads_act_win"):
        setattr(c, name, list(getattr(kv, name)))
    for attr in ("_desc", "_dec_ctx", "_blk_ctx"):
        c.__dict__.pop(attr, None)
    return c


# ---- 1. reference-pinned, fp32 (g20: the reference's decode route from an empty cache, every row) --------------------------------------
def _g20_module(prefill_tile):
    import golden_inputs as gi
    from nsa_vibe_amd.nsa_attention import NSAAttention

    g = load_golden("g20_tiny_bench_module")
    dim, H, G, dk, dv, l, d, ls, n, w = (int(x) for x in g["cfg"])
    m = NSAAttention(dim, H, G, dk, dv, l=l, d=d, l_sel=ls, n_sel=n, w=w, selector="sequential", prefill_tile=prefill_tile)
    names_shapes = [(str(nm), tuple(int(x) for x in sh if x > 0)) for nm, sh in zip(g["names"], g["shapes"])]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gi.g20_state(names_shapes).items()})
    with torch.no_grad():
        m.gate.fc2.bias.copy_(torch.tensor([-1000.0, 1000.0, -1000.0]))
    _, x_dec = gi.g20_inputs()
    x = torch.from_numpy(np.ascontiguousarray(x_dec[:, :, 0].transpose(1, 0, 2))).cuda()  # [1, 544, 256]
    return g, m.cuda().eval(), x


def _g20_check(g, m, out, ranges):
    from test_hip_module import _live

    assert np.abs(out.cpu().numpy()[0] - g["out_dec"][:, 0, 0]).max() <= 1e-3
    got = ranges[0].cpu().numpy()
    assert all(_live(got[t, gg]) == _live(g["ranges_dec"][t, gg]) for t in range(got.shape[0]) for gg in range(got.shape[1]))
    assert m.get_fallback_counters()["total_fallbacks"] == 0


@gpu
@pytest.mark.parametrize("tile", [544, 100, 64, 1])
def test_g20_tiled_prefill_matches_reference_decode(tile):
    g, m, x = _g20_module(tile)
    with torch.no_grad():
        kv = m.new_kv(1, x.shape[1], "cuda", torch.float32)
        out, kv = m(x, kv, prefill=True)
    torch.cuda.synchronize()
    assert kv.t == x.shape[1] and kv.n_cmp == _n_cmp(x.shape[1]) and len(kv.reads_pred) == x.shape[1]
    _g20_check(g, m, out, m._last_ranges)


@gpu
def test_g20_prefill_onto_filled_cache_matches_reference_decode():
    g, m, x = _g20_module(300)
    with torch.no_grad():
        kv = m.new_kv(1, x.shape[1], "cuda", torch.float32)
        o1, kv = m(x[:, :300], kv, prefill=True)
        r1 = m._last_ranges
        m.prefill_tile = 0
        o2, kv = m(x[:, 300:], kv, prefill=True)  # a plain prefill on the filled cache
        r2 = m._last_ranges
    torch.cuda.synchronize()
    assert kv.t == x.shape[1]
    _g20_check(g, m, torch.cat([o1, o2], dim=1), torch.cat([r1, r2], dim=1))


# ---- 2. reference-pinned, bf16, m7c geometry (g19) ------------------------------------------------------------------------------------
def _g19_extend(splits, tile):
    import golden_inputs as gi
    from test_hip_module import _g19_module

    g, m = _g19_module("sequential", torch.bfloat16)
    m.prefill_tile = tile
    _, x_dec = gi.g19_inputs()
    x = torch.from_numpy(np.ascontiguousarray(x_dec[:, :, 0].transpose(1, 0, 2))).cuda().bfloat16()  # [1, 2200, 768]
    outs, rgs = [], []
    with torch.no_grad():
        kv = m.new_kv(x.shape[0], x.shape[1], "cuda", torch.bfloat16)
        for a, b in splits:
            o, kv = m(x[:, a:b], kv, prefill=True)
            outs.append(o)
            rgs.append(m._last_ranges)
    torch.cuda.synchronize()
    return g, m, kv, torch.cat(outs, dim=1), torch.cat(rgs, dim=1)


@gpu
@pytest.mark.parametrize("splits,tile", [([(0, 2200)], 2200), ([(0, 2200)], 512), ([(0, 1100), (1100, 2200)], 0)])
def test_g19_tiled_prefill_matches_reference_decode(splits, tile):
    from test_hip_module import _g19_check, _row_err

    g, m, kv, out, ranges = _g19_extend(splits, tile)
    rows = g["rows_dec"]
    got = out.float().cpu().numpy()[0, rows]
    assert np.isfinite(got).all() and kv.t == 2200
    err, scale = _row_err(got, g["out_dec"][:, 0, 0])
    _g19_check(f"extend {splits} tile {tile}", err, scale, ranges[0, torch.from_numpy(rows).cuda()].cpu().numpy(), g["ranges_dec"],
               g["gap_dec"], 0.5)
    assert m.get_fallback_counters()["total_fallbacks"] == 0


# ---- 3. every scorer form against the oracle chain on K_cmp[:n_cmp(t)] --------------------------------------------------------------
def _oracle_rows(orc, Q, Kc, ts, om, scale):
    """per row: compute_pcmp_all over the row's own n_cmp(t) compressed tokens -> Eq.9/10 -> sequential top-n at t"""
    B, S, G = Q.shape[:3]
    S_sel = om.sel_starts.size
    pg = np.zeros((B, S, G, S_sel), np.float32)
    for s, t in enumerate(ts):
        nc = min(_n_cmp(t + 1), Kc.shape[2])
        if nc == 0:
            continue
        p = orc.compute_pcmp_all(Q[:, s: s + 1], Kc[:, :, :nc], scale)
        _, g = orc.map_pcmp_to_pslc_and_pgrp(p, om)
        pg[:, s] = g[:, 0]
    tt = np.repeat(np.asarray(ts, np.int32), G)
    r = np.stack([orc.select_topn_ranges_rows(pg[b].reshape(S * G, S_sel), tt, om, 16) for b in range(B)])
    return pg, r.reshape(B, S, G, 16, 2)


@gpu
@pytest.mark.parametrize("ctx", ["short", "long"])
@pytest.mark.parametrize("form", ["generic", "mfma16", "mfma16flat", "mfma32", "decode"])
def test_decode_normalised_scorer_matches_oracle_chain(orc, tune, ctx, form):
    import nsa_vibe_amd as nv
    from nsa_vibe_amd.selection_scorer import select_topn_ranges_rows, selection_scores, selection_scores_select
    from test_hip_selection import _topn_gap

    S = 96 if form == "decode" else 192
    T = 3264 if ctx == "short" else 49280  # n_cmp(T - 1) = 203 / 3079 compressed tokens
    q0 = T - S
    B, G = (2, 2)
    g = torch.Generator(device="cuda")
    g.manual_seed(T + S)
    meta = nv.build_block_meta(T, 32, 16, 64, 16, 512)
    om = orc.build_block_meta(T, 32, 16, 64, 16, 512)
    Q = torch.randn(B, S, G, 6, 64, device="cuda", generator=g).bfloat16()
    Kc = torch.randn(B, G, _n_cmp(T), 64, device="cuda", generator=g).bfloat16()
    Kc[:, :, ::7] *= 3.0
    variant = {"generic": 1, "mfma16": 2, "mfma16flat": 2, "mfma32": 2, "decode": 3}[form]
    if form.startswith("mfma"):
        tune("SCORES_FORM", {"mfma16": 0, "mfma16flat": 1, "mfma32": 2}[form])
    pg = selection_scores(Q, Kc, meta, 0.125, variant=variant, q0=q0, normalize="causal")
    rg = select_topn_ranges_rows(pg, meta, 16, t0=q0)
    if form == "mfma32":  # the scorer with the top-n selection in its epilogue (the extend's call) must give the same ranges
        tune("SCORES_SELECT", 1)
        _, rg2 = selection_scores_select(Q, Kc, meta, 16, mode="sequential", t0=q0, scale=0.125, normalize="causal")
        assert torch.equal(rg2, rg)
    pg2 = selection_scores(Q, Kc, meta, 0.125, variant=variant, q0=q0, normalize="causal")
    torch.cuda.synchronize()
    assert torch.equal(pg, pg2)  # reproducible bit for bit
    ts = np.arange(q0, T)
    ref_pg, ref_r = _oracle_rows(orc, Q.float().cpu().numpy(), Kc.float().cpu().numpy(), ts, om, 0.125)
    got = pg.cpu().numpy()
    readable = (np.arange(om.sel_starts.size)[None, :] + 1) * 64 <= (ts[:, None] + 1)  # [S, S_sel]
    err = np.abs(got - ref_pg) * readable[None, :, None, :]
    print(f"{form} {ctx}: max |p_grp - oracle| {err.max():.3e}, max |oracle| {np.abs(ref_pg).max():.3e}")
    # fp32 exp2 / log2 forms against the oracle's expf: ~1e-6 of the row maximum at 200 compressed tokens, ~1.2e-5 at 3k (the same for the
    # unnormalised prefill scorers at this context); ranges must agree wherever the 13th / 14th key gap exceeds twice that
    tol = (4e-6 if ctx == "short" else 2e-5) * max(1.0, float(np.abs(ref_pg).max()))
    assert err.max() <= tol, err.max()
    gaps = _topn_gap(ref_pg.reshape(-1, om.sel_starts.size), np.tile(ts, B).astype(np.int32))
    same = (rg.cpu().numpy() == ref_r).all(axis=(-1, -2)).reshape(-1)
    gated = gaps > 2 * tol
    assert gated.mean() > 0.5 and same[gated].all()


@gpu
def test_decode_normalised_scorer_fp32_generic(orc):
    import nsa_vibe_amd as nv
    from nsa_vibe_amd.selection_scorer import selection_scores

    B, G, S, T = 1, 2, 150, 1000
    q0 = T - S
    meta = nv.build_block_meta(T, 32, 16, 64, 16, 512)
    om = orc.build_block_meta(T, 32, 16, 64, 16, 512)
    Q = torch.randn(B, S, G, 4, 32, device="cuda")
    Kc = torch.randn(B, G, _n_cmp(T), 32, device="cuda")
    pg = selection_scores(Q, Kc, meta, 32 ** -0.5, variant=1, q0=q0, normalize="causal")
    ref, _ = _oracle_rows(orc, Q.cpu().numpy(), Kc.cpu().numpy(), np.arange(q0, T), om, 32 ** -0.5)
    assert np.abs(pg.cpu().numpy() - ref).max() < 2e-6


# ---- 4. against decode steps at a long context ----------------------------------------------------------------------------------------
def _m7c_layer(B=2):
    from nsa_vibe_amd.nsa_attention import NSAAttention

    torch.manual_seed(11)
    m = NSAAttention(768, 12, 2, 64, 64, l=32, d=16, l_sel=64, n_sel=16, w=512, selector="sequential")
    return m.cuda().bfloat16().eval()


@gpu
def test_extend_equals_decode_steps_long_context():
    from test_hip_module import _live

    m = _m7c_layer()
    B, T = 2, 60000
    Smax = max((1, 7, 256))
    x = torch.randn(B, T + Smax, 768, device="cuda").bfloat16()
    with torch.no_grad():
        kv = m.new_kv(B, T + Smax, "cuda", torch.bfloat16)
        m(x[:, :T], kv, prefill=True)
        for S in (1, 7, 256):
            ka, kb = _clone_kv(kv), _clone_kv(kv)
            oa, _ = m(x[:, T: T + S], ka, prefill=True)
            ra = m._last_ranges.clone()
            ob, rb = [], []
            for i in range(S):
                o, _ = m(x[:, T + i: T + i + 1], kb, prefill=False)
                ob.append(o)
                rb.append(m._last_ranges.clone())
            ob, rb = torch.cat(ob, dim=1), torch.stack(rb, dim=1)  # [B,S,dim], [B,S,G,n,2]
            torch.cuda.synchronize()
            # the decode step projects with its own fused GEMV, the extend with the prefill GEMM: the cached rows agree up to the bf16
            # rounding of the projection (and of the pooled tokens built from them); everything before the extend is untouched
            for name in ("K_sel", "V_sel", "K_cmp", "V_cmp", "K_cmp_raw_seq"):
                a, b = getattr(ka, name).float(), getattr(kb, name).float()
                assert a.shape == b.shape, name
                n_old = T if name != "K_cmp" and name != "V_cmp" else _n_cmp(T)
                assert torch.equal(a[:, :, :n_old], b[:, :, :n_old]), name
                dmax = (a - b).abs().max().item()
                print(f"S={S} {name}: max |extend - decode| {dmax:.3e}")
                assert dmax <= 2e-2 * max(1.0, b.abs().max().item()), (name, dmax)
            assert (ka.t, ka.n_cmp, len(ka.reads_pred)) == (kb.t, kb.n_cmp, len(kb.reads_pred))
            assert ka.reads_act_cmp == kb.reads_act_cmp and ka.reads_act_win == kb.reads_act_win
            # rows whose decode-side 13th / 14th gap is wide: same ranges, outputs within the layer tests' bf16 tolerance
            same = np.array([[_live(ra[b, s, g].cpu().numpy()) == _live(rb[b, s, g].cpu().numpy()) for g in range(2)]
                             for b in range(B) for s in range(S)])
            assert same.mean() >= 0.9, same.mean()
            rows = same.all(axis=1).reshape(B, S)
            err = (oa.float() - ob.float()).abs().amax(dim=-1).cpu().numpy()
            assert err[rows].max() <= 1e-2 * max(1.0, float(ob.float().abs().max())), err[rows].max()
    assert m.get_fallback_counters()["total_fallbacks"] == 0


# ---- 5. chunking invariance and route equality ----------------------------------------------------------------------------------------
def _run_tiles(m, x, tile, one_call=True):
    m.prefill_tile = tile
    with torch.no_grad():
        kv = m.new_kv(x.shape[0], x.shape[1], "cuda", x.dtype)
        if one_call:
            out, kv = m(x, kv, prefill=True)
        else:
            out, kv = m._extend(x, kv, one_call=False)
    torch.cuda.synchronize()
    return out, m._last_ranges.clone(), kv


@gpu
def test_extend_chunking_invariance_and_routes():
    from test_hip_module import _live

    m = _m7c_layer(1)
    x = torch.randn(1, 2048, 768, device="cuda").bfloat16()
    base_o, base_r, base_kv = _run_tiles(m, x, 2048)
    for tile in (64, 512):
        # chunk boundaries on the scorer's 64-row tile: the ranges are bit-identical; the outputs agree up to the bf16 rounding of the
        # projection GEMM and the attention forms, which are chosen by the chunk's row count
        o, r, kv = _run_tiles(m, x, tile)
        assert torch.equal(r, base_r), tile
        d = (o.float() - base_o.float()).abs().max().item()
        print(f"tile {tile}: max |out - out(2048)| {d:.3e}")
        assert d <= 1e-2, (tile, d)
        assert (kv.K_cmp.float() - base_kv.K_cmp.float()).abs().max().item() <= 2e-2
    o, r, _ = _run_tiles(m, x, 100)  # boundaries off the 64-row tile: ranges gap-gated, outputs within bf16 noise
    same = np.array([_live(a) == _live(b) for a, b in zip(r.reshape(-1, 16, 2).cpu().numpy(), base_r.reshape(-1, 16, 2).cpu().numpy())])
    assert same.mean() >= 0.97
    rows = torch.from_numpy(same.reshape(2048, 2).all(axis=1)).cuda()
    assert (o[0, rows].float() - base_o[0, rows].float()).abs().max().item() <= 2e-2
    o1, r1, _ = _run_tiles(m, x, 512, one_call=True)
    o2, r2, _ = _run_tiles(m, x, 512, one_call=False)  # the per-stage composition
    assert torch.equal(r1, r2) and torch.equal(o1, o2)
    o3, r3, _ = _run_tiles(m, x, 512)  # run to run
    assert torch.equal(o3, o1) and torch.equal(r3, r1)


# ---- 6. model level: a second turn on filled caches ---------------------------------------------------------------------------------
@gpu
def test_tiny_lm_multi_turn_prefill_matches_token_by_token():
    from nsa_vibe_amd.llama_block_nsa import TinyLM

    torch.manual_seed(2)
    lm = TinyLM(97, 64, 3, 4, 2, 16, 16, 8, 4, 8, 4, 16, selector="sequential").cuda().float().eval()
    B, P, S, n = 2, 60, 37, 8
    tok = torch.randint(0, 97, (B, P + S + n), device="cuda")
    with torch.no_grad():
        caches = lm.new_caches(B, P + S + n, "cuda", torch.float32)
        lm.prefill(tok[:, :P], caches)
        second = lm.prefill(tok[:, P: P + S], caches, last_only=False)
        got = [second] + [lm.decode(tok[:, t: t + 1], caches) for t in range(P + S, P + S + n)]
        ref_c = lm.new_caches(B, P + S + n, "cuda", torch.float32)
        lm.prefill(tok[:, :P], ref_c)
        ref = [lm.decode(tok[:, t: t + 1], ref_c) for t in range(P, P + S + n)]
    got, ref = torch.cat(got, dim=1), torch.cat(ref, dim=1)
    assert got.shape == ref.shape == (B, S + n, 97)
    assert (got - ref).abs().max().item() <= 2e-4


# ---- 7. CPU: switches, errors, routing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("val,want", [(None, 0), ("0", 0), ("-3", 0), ("abc", 0), ("256", 256)])
def test_prefill_tile_env_parsing(monkeypatch, val, want):
    from nsa_vibe_amd.nsa_attention import NSAAttention

    if val is None:
        monkeypatch.delenv("NSA_PREFILL_TILE", raising=False)
    else:
        monkeypatch.setenv("NSA_PREFILL_TILE", val)
    assert NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=8, n_sel=4, w=16).prefill_tile == want
    assert NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=8, n_sel=4, w=16, prefill_tile=48).prefill_tile == 48
    assert NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=8, n_sel=4, w=16, prefill_tile=-5).prefill_tile == 0


def test_extend_under_autograd_on_filled_cache_raises():
    from nsa_vibe_amd.nsa_attention import NSAAttention

    m = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=8, n_sel=4, w=16)
    kv = m.new_kv(1, 32, "cpu", torch.float32)
    kv.t = 10
    with pytest.raises(RuntimeError, match="filled cache"):
        m(torch.randn(1, 4, 64, requires_grad=True), kv, prefill=True)
    assert m.get_fallback_counters()["total_fallbacks"] == 0


def test_prefill_tile_not_applied_under_autograd(monkeypatch):
    from nsa_vibe_amd.nsa_attention import NSAAttention

    m = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=8, n_sel=4, w=16, prefill_tile=2)
    seen = []
    monkeypatch.setattr(NSAAttention, "_prefill", lambda self, x, kv, one_call=True: seen.append("prefill") or (x, kv))
    monkeypatch.setattr(NSAAttention, "_extend", lambda self, x, kv, one_call=True: seen.append("extend") or (x, kv))
    kv = m.new_kv(1, 32, "cpu", torch.float32)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m(torch.randn(1, 4, 64, requires_grad=True), kv, prefill=True)
        m(torch.randn(1, 4, 64, requires_grad=True), m.new_kv(1, 32, "cpu", torch.float32), prefill=True)
    assert seen == ["prefill", "prefill"]
    assert sum(issubclass(x.category, RuntimeWarning) and "prefill_tile" in str(x.message) for x in w) == 1


def test_parity_mode_on_filled_cache_raises(monkeypatch):
    from nsa_vibe_amd.nsa_attention import NSAAttention

    monkeypatch.setenv("NSA_FORCE_PARITY", "1")
    m = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=8, n_sel=4, w=16)
    kv = m.new_kv(1, 32, "cpu", torch.float32)
    kv.t = 8
    with torch.no_grad(), pytest.raises(RuntimeError, match="NSA_FORCE_PARITY"):
        m(torch.randn(1, 4, 64), kv, prefill=True)


def test_route_selection(monkeypatch):
    """prefill_tile = 0 on an empty cache keeps the existing prefill route; a filled cache or a tile takes the extend route"""
    from nsa_vibe_amd.nsa_attention import NSAAttention

    monkeypatch.delenv("NSA_PREFILL_TILE", raising=False)
    seen = []
    monkeypatch.setattr(NSAAttention, "_prefill", lambda self, x, kv, one_call=True: seen.append("prefill") or (x, kv))
    monkeypatch.setattr(NSAAttention, "_extend", lambda self, x, kv, one_call=True: seen.append("extend") or (x, kv))
    m = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=8, n_sel=4, w=16)
    with torch.no_grad():
        m(torch.randn(1, 4, 64), m.new_kv(1, 32, "cpu", torch.float32), prefill=True)
        kv = m.new_kv(1, 32, "cpu", torch.float32)
        kv.t = 5
        m(torch.randn(1, 4, 64), kv, prefill=True)
        m.prefill_tile = 2
        m(torch.randn(1, 4, 64), m.new_kv(1, 32, "cpu", torch.float32), prefill=True)
    assert seen == ["prefill", "extend", "extend"]


def test_block_native_prefill_shortcut_respects_tile(monkeypatch):
    from nsa_vibe_amd.llama_block_nsa import LlamaBlockNSA
    from nsa_vibe_amd.nsa_attention import NSAAttention

    blk = LlamaBlockNSA(64, 4, 2, 16, 16, l=8, d=4, l_sel=8, n_sel=4, w=16, prefill_tile=3)
    seen = []
    monkeypatch.setattr(NSAAttention, "_native_ok", lambda self, x: True)
    monkeypatch.setattr(LlamaBlockNSA, "_prefill_native", lambda self, x, kv: seen.append("block_native") or x)
    monkeypatch.setattr(NSAAttention, "_extend", lambda self, x, kv, one_call=True: seen.append("extend") or (x, kv))
    with torch.no_grad():
        blk(torch.randn(1, 4, 64), blk.attn.new_kv(1, 32, "cpu", torch.float32), prefill=True)
    assert seen == ["extend"]
