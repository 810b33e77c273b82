"""GPU parity: the one-launch decode step of the selected branch (sel_decode_fused.hip) and the decode attention as its own launch
(sel_attn_decode.hip) at head dimension 128.  Mirrors the D = 64 tests of test_hip_selection.py: ranges bit-exact against the oracle's
selector on the device scores, O within the project's bf16 bar (1e-2) of the oracle's attention, and the fused route bit-identical to
the separate launches (both run the row functions of sel_attn_decode.hpp).  The four-chunks-per-wave and one-pass forms are not built
for D = 128: shapes that would need them take the separate launches, which the plan query must report."""
import numpy as np
import pytest
import torch

from test_hip_selection import dev, norm, nv  # noqa: F401  (nv: the module fixture of the D = 64 tests)

pytestmark = pytest.mark.gpu

D128 = 128


def _shape(nv, S_ctx, n=16):
    m = nv.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    return m, m.S_cmp, m.S_sel


@pytest.mark.parametrize("S_ctx,B", [(4096, 8), (16384, 5), (65536, 1), (65536, 32)])
def test_plan_reports_one_launch_at_d128(nv, S_ctx, B):
    """nsa_sel_decode_step_plan: the shapes of the issue run as ONE launch at D = 128 (form 0: logits in registers; 64k rows as a team of
    four workgroups of eight waves, two chunks per wave)"""
    m, S_cmp, S_sel = _shape(nv, S_ctx)
    p = nv.selection_decode_step_plan(B, 2, 6, D128, D128, S_cmp, S_sel, S_ctx, 16, torch.bfloat16)
    assert p["launches"] == 1 and p["form"] == 0, p
    assert p["nsplit"] == (1 if S_ctx <= 16384 else 8 if B == 1 else 4), p
    p16 = nv.selection_decode_step_plan(B, 2, 6, D128, D128, S_cmp, S_sel, S_ctx, 16, torch.float16)
    assert p16 == p


def test_plan_at_d64_is_the_plan_of_the_existing_forms(nv, tune):
    """at D = 64 the query reports what decode_step_plan has always chosen (README round 3 / 4: unsplit to 16k, teams of 8 chunks at 64k with
    few rows, the one-pass form where B*G teams do not fit the chip), and follows the tuning switches"""
    G, h, n = 2, 6, 16
    q = lambda S, B: nv.selection_decode_step_plan(B, G, h, 64, 64, _shape(nv, S)[1], _shape(nv, S)[2], S, n)  # noqa: E731
    assert q(4096, 8) == {"launches": 1, "form": 0, "nsplit": 1}
    assert q(16384, 64) == {"launches": 1, "form": 0, "nsplit": 1}
    assert q(16384, 256) == {"launches": 1, "form": 0, "nsplit": 1}
    assert q(65536, 1) == {"launches": 1, "form": 0, "nsplit": 8}
    assert q(65536, 128) == {"launches": 1, "form": 2, "nsplit": 1}
    tune("DECODE_WIDE", 0)
    p = q(65536, 128)
    assert p["launches"] == 2 and p["form"] == -1 and p["nsplit"] == 0
    tune("DECODE_WIDE", -1), tune("DECODE_UNFUSED", 1)
    assert q(4096, 8)["launches"] > 1


@pytest.mark.parametrize("S_ctx,B", [(65536, 1), (65536, 4), (16384, 5), (200, 3), (70, 2)])
def test_fused_decode_step_d128(nv, orc, S_ctx, B):
    """test_fused_decode_step at D = 128: nsa_sel_decode_step == the three separate calls, and == the oracle's decode chain (bf16)"""
    rng = np.random.default_rng([S_ctx, B, D128])
    G, h, D, n = 2, 6, D128, 16
    m = nv.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    mo = orc.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    dt = torch.bfloat16
    Q = rng.standard_normal((B, 1, G, h, D), dtype=np.float32)
    Kc = rng.standard_normal((B, G, m.S_cmp, D), dtype=np.float32)
    K = rng.standard_normal((B, G, S_ctx + 37, D), dtype=np.float32)  # preallocated cache longer than the context
    V = rng.standard_normal((B, G, S_ctx + 37, D), dtype=np.float32)
    t = S_ctx - 1
    Kd, Vd = dev(K, dt), dev(V, dt)
    assert nv.selection_decode_step_plan(B, G, h, D, D, m.S_cmp, m.S_sel, S_ctx, n, dt)["launches"] == 1
    O, rg = nv.selection_decode_step(dev(Q, dt), dev(Kc, dt), Kd[:, :, :S_ctx], Vd[:, :, :S_ctx], m, n, t)
    p = nv.selection_scores(dev(Q, dt), dev(Kc, dt), m)
    r2 = nv.select_topn_ranges(p[:, 0], m, n, t)
    O2 = nv.selection_attention_hip(dev(Q, dt), Kd[:, :, :S_ctx], Vd[:, :, :S_ctx], r2.unsqueeze(1))
    assert torch.equal(rg, r2) and torch.equal(O, O2)
    rd = lambda a: torch.from_numpy(a).to(dt).float().numpy()  # noqa: E731
    r_ref = orc.select_topn_ranges(p[:, 0].cpu().numpy(), mo, n, t)
    assert norm(rg.cpu().numpy()) == norm(r_ref)
    O_ref = orc.sel_attention_masked(rd(Q), rd(K[:, :, :S_ctx]), rd(V[:, :, :S_ctx]), rg.cpu().numpy()[:, None])
    err = np.abs(O.float().cpu().numpy() - O_ref).max()
    print(f"D=128 decode step S_ctx={S_ctx} B={B}: max|dO| = {err:.3e}")
    assert err <= 1e-2


@pytest.mark.parametrize("h", [1, 3, 4, 6, 8, 16])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_equals_unfused_d128(nv, tune, h, dtype):
    """the one-launch step at D = 128 (HC = 6 and the generic head sum; unsplit and as a team of four workgroups) against the separate
    launches (DECODE_UNFUSED = 1, with the closed-form stencil and with the CSC taps): ranges and O bit-identical, run to run too"""
    g = torch.Generator(device="cuda")
    g.manual_seed(150 + h)
    B, G, D, n, S_ctx = 3, 2, D128, 16, 9000
    meta = nv.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    mk = lambda *sh: torch.randn(*sh, device="cuda", generator=g).to(dtype)  # noqa: E731
    Q, Kc, K, V = mk(B, 1, G, h, D), mk(B, G, meta.S_cmp, D), mk(B, G, S_ctx, D), mk(B, G, S_ctx, D)
    t = S_ctx - 1
    for stencil in (0, 1):
        tune("DECODE_STENCIL", stencil)
        tune("DECODE_UNFUSED", 1)
        O0, r0 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)
        tune("DECODE_UNFUSED", -1)
        for ns in (1, 4):
            tune("DECODE_SPLIT", ns)
            plan = nv.selection_decode_step_plan(B, G, h, D, D, meta.S_cmp, meta.S_sel, S_ctx, n, dtype)
            assert plan == {"launches": 1, "form": 0, "nsplit": ns}
            O1, r1 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)
            O2, r2 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)  # tickets left clean
            torch.cuda.synchronize()
            assert torch.equal(r0, r1) and torch.equal(O0, O1), (h, ns, stencil)
            assert torch.equal(r1, r2) and torch.equal(O1, O2), (h, ns, stencil)
        tune("DECODE_SPLIT", -1)


@pytest.mark.parametrize("S_ctx,B,n", [(65536, 32, 16), (65536, 2, 40), (40000, 3, 3), (100001, 1, 64), (131072, 2, 16), (4096, 200, 16)])
def test_fused_equals_unfused_d128_long_rows_and_many_rows(nv, tune, S_ctx, B, n):
    """teams of workgroups at long contexts (64k with 64 rows: the four workgroups of every row exactly fill the chip), 3 <= n_top <= 64,
    and more rows than CUs: the automatic plan is one launch, bit-identical to the separate launches; a team with a poll budget of zero
    (every workgroup finishes the row's records alone) gives the same bits"""
    g = torch.Generator(device="cuda")
    g.manual_seed(S_ctx + B + n)
    G, h, D = 2, 6, D128
    meta = nv.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    mk = lambda *sh: torch.randn(*sh, device="cuda", generator=g, dtype=torch.bfloat16)  # noqa: E731
    Q, Kc, K, V = mk(B, 1, G, h, D), mk(B, G, meta.S_cmp, D), mk(B, G, S_ctx, D), mk(B, G, S_ctx, D)
    t = S_ctx - 1
    assert nv.selection_decode_step_plan(B, G, h, D, D, meta.S_cmp, meta.S_sel, S_ctx, n)["launches"] == 1
    tune("DECODE_UNFUSED", 1)
    O0, r0 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)
    tune("DECODE_UNFUSED", -1)
    O1, r1 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)
    tune("DECODE_TEAM_SPIN", 0)
    O2, r2 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)
    torch.cuda.synchronize()
    assert torch.equal(r0, r1) and torch.equal(O0, O1)
    assert torch.equal(r0, r2) and torch.equal(O0, O2)


@pytest.mark.parametrize("S_ctx", [3000, 16384, 65536])
def test_decode_step_on_tie_heavy_scores_d128(nv, orc, tune, S_ctx):
    """the construction of test_decode_step_on_tie_heavy_scores at D = 128 (all ties, plateaus, a peaked softmax, an ordinary row, NaN
    logits): ranges bit-equal to the separate launches and to the oracle's selector (key desc, index asc)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(S_ctx)
    B, G, h, D, n = 5, 2, 6, D128, 16
    meta = nv.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    mo = orc.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    mk = lambda *sh: torch.randn(*sh, device="cuda", generator=g).bfloat16()  # noqa: E731
    Q, K, V = mk(B, 1, G, h, D), mk(B, G, S_ctx, D), mk(B, G, S_ctx, D)
    Kc = torch.zeros(B, G, meta.S_cmp, D, device="cuda", dtype=torch.bfloat16)  # b = 0: all ties
    three = mk(3, D)
    Kc[1] = three[torch.randint(0, 3, (G, meta.S_cmp), device="cuda", generator=g)]  # plateaus
    Kc[2] = mk(G, meta.S_cmp, D)
    Kc[2, :, 777 % meta.S_cmp] = Q[2, 0, :, 0] * 40  # one column takes all the mass: the other blocks' scores underflow to exact zeros
    Kc[3] = mk(G, meta.S_cmp, D)  # ordinary
    Kc[4] = mk(G, meta.S_cmp, D)
    Kc[4, 0, 5] = float("nan")  # one NaN logit poisons the row's normaliser: every score NaN, no candidate
    t = S_ctx - 1
    tune("DECODE_UNFUSED", 1)
    O0, r0 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)
    tune("DECODE_UNFUSED", -1)
    for ns in (-1, 1, 4):
        tune("DECODE_SPLIT", ns)
        assert nv.selection_decode_step_plan(B, G, h, D, D, meta.S_cmp, meta.S_sel, S_ctx, n)["launches"] == 1
        O1, r1 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)
        torch.cuda.synchronize()
        assert torch.equal(r0, r1), ns
    tune("DECODE_SPLIT", -1)
    O1, r1 = nv.selection_decode_step(Q, Kc, K, V, meta, n, t)
    fin = torch.isfinite(O0.float()).all(dim=-1).all(dim=-1)
    assert torch.equal(O0[fin], O1[fin])
    p = nv.selection_scores(Q, Kc, meta)[:, 0].cpu().numpy()
    ok = np.isfinite(p).all(axis=-1)
    want = orc.select_topn_ranges(np.where(ok[..., None], p, 0.0).astype(np.float32), mo, n, t)
    got = r1.cpu().numpy()
    for b in range(B):
        for gg in range(G):
            if ok[b, gg]:
                assert norm(got[b, gg][None]) == norm(want[b, gg][None]), (b, gg)
    assert got[0, 0].tolist()[:3] == [[0, 64 * 14], [64 * (t // 64 - 1), t + 1], [0, 0]]  # all ties: blocks 1..13 win


def test_declined_shapes_take_the_separate_launches_d128(nv, orc, tune):
    """shapes the D = 128 plan declines still give the result of the separate launches, and the plan query says so: a context beyond the
    128 chunks of a row (140000 tokens), a long context with more rows than teams fit (B = 64 at 64k: 128 rows x 4 workgroups > CUs; the
    forms D = 64 uses there are not built), the wide forms forced by switch, and a block geometry other than l = 2d, l' = 4d = 64"""
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    G, h, D, n = 2, 6, D128, 16
    mk = lambda *sh: torch.randn(*sh, device="cuda", generator=g, dtype=torch.bfloat16)  # noqa: E731
    f = lambda a: a.float().cpu().numpy()  # noqa: E731
    # (a) beyond 128 chunks
    S_ctx, B = 140000, 1
    meta = nv.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    mo = orc.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    Q, Kc, K, V = mk(B, 1, G, h, D), mk(B, G, meta.S_cmp, D), mk(B, G, S_ctx, D), mk(B, G, S_ctx, D)
    p = nv.selection_decode_step_plan(B, G, h, D, D, meta.S_cmp, meta.S_sel, S_ctx, n)
    assert p["launches"] > 1 and p["form"] == -1 and p["nsplit"] == 0, p
    O1, r1 = nv.selection_decode_step(Q, Kc, K, V, meta, n, S_ctx - 1)
    tune("DECODE_UNFUSED", 1)
    O0, r0 = nv.selection_decode_step(Q, Kc, K, V, meta, n, S_ctx - 1)
    tune("DECODE_UNFUSED", -1)
    assert torch.equal(r0, r1) and torch.equal(O0, O1)
    pg = nv.selection_scores(Q, Kc, meta)
    assert norm(r1.cpu().numpy()) == norm(orc.select_topn_ranges(pg[:, 0].cpu().numpy(), mo, n, S_ctx - 1))
    assert np.abs(f(O1) - orc.sel_attention_masked(f(Q), f(K), f(V), r1.cpu().numpy()[:, None])).max() <= 1e-2
    # (b) more rows at 64k than teams fit the chip; (c) the wide forms by switch: D = 128 stays on form 0 (exact) where it fits
    S_ctx = 65536
    meta = nv.build_block_meta(S_ctx, 32, 16, 64, n, 512)
    p = nv.selection_decode_step_plan(64, G, h, D, D, meta.S_cmp, meta.S_sel, S_ctx, n)
    assert p["launches"] == 2 and p["form"] == -1, p
    for wide in (1, 2):
        tune("DECODE_WIDE", wide)
        assert nv.selection_decode_step_plan(2, G, h, D, D, meta.S_cmp, meta.S_sel, S_ctx, n)["form"] == 0
        assert nv.selection_decode_step_plan(64, G, h, D, D, meta.S_cmp, meta.S_sel, S_ctx, n)["launches"] == 2
    tune("DECODE_WIDE", -1)
    B = 64
    Q, Kc, K, V = mk(B, 1, G, h, D), mk(B, G, meta.S_cmp, D), mk(B, G, S_ctx, D), mk(B, G, S_ctx, D)
    O1, r1 = nv.selection_decode_step(Q, Kc, K, V, meta, n, S_ctx - 1)
    tune("DECODE_UNFUSED", 1)
    O0, r0 = nv.selection_decode_step(Q, Kc, K, V, meta, n, S_ctx - 1)
    tune("DECODE_UNFUSED", -1)
    assert torch.equal(r0, r1) and torch.equal(O0, O1)
    del K, V
    # (d) another block geometry.  NOT covered by the plan assertion: nsa_sel_decode_step_plan has no l / d / l' arguments and speaks about the
    # default geometry only, so here only the result (== separate launches, == oracle) is checked; the plan's "more than one launch" is
    # asserted for (a) and (b) above
    S_ctx, B = 3000, 2
    meta = nv.build_block_meta(S_ctx, 16, 8, 32, n, 512)
    mo = orc.build_block_meta(S_ctx, 16, 8, 32, n, 512)
    Q, Kc, K, V = mk(B, 1, G, h, D), mk(B, G, meta.S_cmp, D), mk(B, G, S_ctx, D), mk(B, G, S_ctx, D)
    O1, r1 = nv.selection_decode_step(Q, Kc, K, V, meta, n, S_ctx - 1)
    tune("DECODE_UNFUSED", 1)
    O0, r0 = nv.selection_decode_step(Q, Kc, K, V, meta, n, S_ctx - 1)
    assert torch.equal(r0, r1) and torch.equal(O0, O1)
    pg = nv.selection_scores(Q, Kc, meta)
    assert norm(r1.cpu().numpy()) == norm(orc.select_topn_ranges(pg[:, 0].cpu().numpy(), mo, n, S_ctx - 1))
    assert np.abs(f(O1) - orc.sel_attention_masked(f(Q), f(K), f(V), r1.cpu().numpy()[:, None])).max() <= 1e-2


def test_decode_attention_launch_d128_arbitrary_ranges(nv, orc):
    """sel_attn_decode.hip at D = 128 on ranges no selector produces (overlapping, empty, unclamped, not multiples of 64, a row without
    keys), K rows strided (a view of a wider cache), bf16 and f16: against the oracle's masked attention"""
    rng = np.random.default_rng(128)
    B, G, h, D, S_kv, n = 3, 2, 5, D128, 1500, 7
    Q = rng.standard_normal((B, 1, G, h, D), dtype=np.float32)
    K = rng.standard_normal((B, G, S_kv, D), dtype=np.float32)
    V = rng.standard_normal((B, G, S_kv, D), dtype=np.float32)
    r = np.zeros((B, 1, G, n, 2), dtype=np.int32)
    r[..., 0] = rng.integers(0, S_kv, size=(B, 1, G, n))
    r[..., 1] = r[..., 0] + rng.integers(-20, 300, size=(B, 1, G, n))  # some empty (end <= start), some past S_kv
    r[0, 0, 0] = 0  # a row without keys -> zeros
    r[1, 0, 1, 0] = (0, S_kv + 100)  # everything, overlapping the others
    for dt in (torch.bfloat16, torch.float16):
        rd = lambda a: torch.from_numpy(a).to(dt).float().numpy()  # noqa: E731
        Kw = torch.zeros(B, G, S_kv, D + 64, device="cuda", dtype=dt)
        Kw[..., :D] = dev(K, dt)
        O = nv.selection_attention_hip(dev(Q, dt), Kw[..., :D], dev(V, dt), dev(r))
        O_ref = orc.sel_attention_masked(rd(Q), rd(K), rd(V), np.minimum(r, S_kv))
        assert np.abs(O.float().cpu().numpy() - O_ref).max() <= 1e-2
        assert float(O[0, 0, 0].float().abs().max()) == 0.0


def test_module_decode_d128_fused_equals_unfused_and_eager(tune, monkeypatch):
    """NSAAttention with 128-wide heads: prefill 300 tokens, 40 decode steps through nsa_layer_decode_step (strict: a failing native call
    raises).  Every step's output with the one-launch selected branch equals the output with DECODE_UNFUSED = 1 bit for bit, and the eager
    composition within the tolerance test_native_vs_eager_over_odd_configurations uses for its dk = 128 configuration."""
    from nsa_vibe_amd.nsa_attention import NSAAttention

    monkeypatch.setenv("NSA_HIP_STRICT", "1")
    torch.manual_seed(128)
    dtype = torch.bfloat16
    m = NSAAttention(768, 6, 2, 128, 128).cuda().to(dtype).eval()
    B, S, n_dec = 2, 300, 40
    x = torch.randn(B, S + n_dec, 768, device="cuda", dtype=dtype)
    outs = {}
    for mode in ("fused", "unfused", "eager"):
        if mode == "eager":
            monkeypatch.setenv("NSA_HIP_EAGER_TRAIN", "1")
        tune("DECODE_UNFUSED", 1 if mode == "unfused" else -1)
        kv = m.new_kv(B, S + n_dec, "cuda", dtype)
        with torch.set_grad_enabled(mode == "eager"):
            o, kv = m(x[:, :S], kv, prefill=True)
            dec = []
            for t in range(S, S + n_dec):
                y, kv = m(x[:, t: t + 1], kv, prefill=False)
                dec.append(y.detach())
        outs[mode] = torch.cat(dec, dim=1)
    assert torch.isfinite(outs["fused"]).all()
    assert torch.equal(outs["fused"], outs["unfused"])
    err = (outs["fused"].float() - outs["eager"].float()).abs().amax(dim=-1)
    print(f"D=128 module decode vs eager: median {err.median().item():.3e}, max {err.max().item():.3e}")
    assert err.median().item() <= 6e-2 and (err <= 6e-2).float().mean().item() >= 0.85
