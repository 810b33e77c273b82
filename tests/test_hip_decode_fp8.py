"""FP8 (OCP e4m3) K/V caches of the ragged and the paged selected-branch decode step (nsa_sel_decode_ragged_fp8 / _paged_fp8) and the
quantiser that makes them (nsa_kv_quantize_fp8).  The cases, their inputs and the page scatter are those of tests/test_hip_decode_ragged.py
and tests/test_hip_decode_paged.py; K / V are quantised with torch on the CPU (amax / 448) and poisoned in FP8 terms: rows behind a
sequence's own tokens and unused pool pages hold +-448 with scale 64."""
import pytest
import torch

from test_hip_decode_paged import PAGE, paged, scatter
from test_hip_decode_ragged import CASES, G, IDS, N_TOP, active, make_case, ragged
from test_hip_selection import dev, nv  # noqa: F401  (nv: the module fixture of the D = 64 tests)

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
BF16 = torch.bfloat16
NAMES = ("S1_mixed", "S3_boundaries", "form1", "B33_waves8", "d128", "h1")
FP8_CASES = [CASES[IDS.index(i)] for i in NAMES]
EDGES = dict(t_pos=[1022, 1023, 1024, 2047, 2048], S=3)


def quant(X):
    Xf = X.float().cpu()
    amax = Xf.abs().amax(-1)
    sc = torch.where(amax == 0, torch.ones_like(amax), amax / 448)
    return (Xf / sc[..., None]).clamp(-448, 448).to(FP8), sc


def fp8_case(nv, case):
    """the case with FP8 caches, made once: K8 / V8 / ks / vs, ones for the unit-scale tests, and the dequantised bf16 caches.  ks and vs
    are the quantiser's scales times a per-row power of two p in [1/8, 8] (drawn separately for K and V), so a dropped or misindexed
    scale cannot cancel; the row's bytes are divided by the same p (rounded and saturated to e4m3 again), so K^ = K8 * ks and V^ = V8 * vs
    stay the unit-normal data the 1e-2 bound is stated for (with V's bytes left alone |V^| reaches 32, where half a bf16 ulp of O alone
    is 6e-2: measured 5.7e-2 on S1_mixed)"""
    c = make_case(nv, **case)
    if "f8" not in c:
        (K8, ks), (V8, vs) = quant(c["K"]), quant(c["V"])
        gen = torch.Generator().manual_seed(len(c["t_pos"]))
        p = torch.exp2(torch.randint(-3, 4, vs.shape, generator=gen).float())
        V8, vs = (V8.float() / p[..., None]).clamp(-448, 448).to(FP8), vs * p
        p = torch.exp2(torch.randint(-3, 4, ks.shape, generator=gen).float())
        K8, ks = (K8.float() / p[..., None]).clamp(-448, 448).to(FP8), ks * p
        for b, t0 in enumerate(c["t_pos"]):
            own = t0 + c["S"] if t0 >= 0 else 0
            K8.view(torch.uint8)[b, :, own:] = 0x7E  # +448
            V8.view(torch.uint8)[b, :, own:] = 0xFE  # -448
            ks[b, :, own:] = 64
            vs[b, :, own:] = 64
        c["f8"] = dict(K8=K8.cuda(), V8=V8.cuda(), ks=ks.cuda(), vs=vs.cuda(), one=torch.ones_like(ks).cuda(),
                       deq=dict(c, K=K8.to(BF16).cuda(), V=V8.to(BF16).cuda(), refs={}))
    return c, c["f8"]


def ragged8(nv, c, f, ks, vs, **kw):
    return nv.selection_decode_ragged(c["Q"], c["Kc"], f["K8"], f["V8"], c["meta"], N_TOP, c["pos"], t_max=c["t_max"], k_scale=ks, v_scale=vs, **kw)


def fp8_pools(c, f, ks, vs):
    """scatter() on the dequantised caches, the pools back to FP8 (exact; the bf16 poison saturates to +-448) and the scales through the same table"""
    pl = scatter(f["deq"], seed=len(c["t_pos"]) + c["S"])
    zk, zv = (torch.full((pl["n_pages"], G, PAGE), 64.0, device="cuda") for _ in range(2))
    for b, t0 in enumerate(c["t_pos"]):
        own = t0 + c["S"] if t0 >= 0 else 0
        for j in range((own + PAGE - 1) // PAGE):
            r, p = min(PAGE, own - PAGE * j), pl["table"][b][j]
            zk[p, :, :r], zv[p, :, :r] = ks[b, :, PAGE * j:PAGE * j + r], vs[b, :, PAGE * j:PAGE * j + r]
    return dict(pl, K=pl["K"].float().clamp(-448, 448).to(FP8), V=pl["V"].float().clamp(-448, 448).to(FP8)), zk, zv


@pytest.mark.parametrize("case", FP8_CASES, ids=NAMES)
def test_unit_scales_are_the_bf16_call_bit_for_bit(nv, case):
    """all scales 1.0f: O and ranges torch.equal with selection_decode_ragged on K8.to(bf16), V8.to(bf16); the plan is the bf16 plan"""
    c, f = fp8_case(nv, case)
    m = c["meta"]
    args = (c["B"], c["S"], G, c["h"], c["D"], c["D"], m.S_cmp, m.S_sel, c["K"].shape[2], N_TOP, c["t_max"])
    assert nv.selection_decode_ragged_fp8_plan(*args) == nv.selection_decode_ragged_plan(*args) and nv.selection_decode_ragged_plan(*args)["launches"] == 1
    O, rg = ragged8(nv, c, f, f["one"], f["one"])
    O1, r1 = ragged(nv, f["deq"])
    assert O.dtype == BF16 and torch.isfinite(O.float()).all()
    assert torch.equal(rg, r1) and torch.equal(O, O1)
    assert torch.equal(rg, ragged(nv, c)[1])  # the selection does not read K / V


@pytest.mark.parametrize("case", FP8_CASES + [EDGES], ids=NAMES + ("page_edges",))
def test_paged_fp8_is_the_ragged_fp8_call_bit_for_bit(nv, case):
    """pools behind a permuted table, general scales: O and ranges torch.equal with the FP8 ragged call on the contiguous caches"""
    c, f = fp8_case(nv, case)
    pl, zk, zv = fp8_pools(c, f, f["ks"], f["vs"])
    O, rg = paged(nv, c, pl, k_scale_pool=zk, v_scale_pool=zv)
    O1, r1 = ragged8(nv, c, f, f["ks"], f["vs"])
    assert torch.equal(rg, r1) and torch.equal(O, O1)


def worst_error(c, O, rg, Kd, Vd):
    """worst |O - plain float64 softmax attention over the call's own ranges on Kd, Vd| over the live rows; inactive slots must be zero rows"""
    Qd, rc, worst = c["Q"].double(), rg.cpu(), 0.0
    for b, t0 in enumerate(c["t_pos"]):
        if not active(t0, c["S"], c["t_max"], c["K"].shape[2]):
            assert not O[b].any() and not rg[b].any(), b
            continue
        for s in range(c["S"]):
            for g in range(G):
                keep = torch.zeros(Kd.shape[2], dtype=torch.bool)
                for a, e in rc[b, s, g].tolist():
                    keep[a:max(a, e)] = True
                idx = keep.nonzero().flatten().cuda()
                p = torch.softmax(Qd[b, s, g] @ Kd[b, g, idx].T * c["D"] ** -0.5, dim=-1)
                worst = max(worst, (O[b, s, g].double() - p @ Vd[b, g, idx]).abs().max().item())
    return worst


@pytest.mark.parametrize("case", FP8_CASES, ids=NAMES)
def test_general_scales_against_float64(nv, case):
    """O against a plain float64 softmax attention over the call's own ranges on K^ = K8 * k_scale, V^ = V8 * v_scale: 1e-2 absolute, the
    project's bf16 bound (tests/test_hip_decode_ragged.py) -- as in the bf16 path one rounding on P and one on O, inputs unit normal.  Ranges
    are the bf16 call's; inactive slots give zero rows; scales of rows behind a sequence's tokens set to inf change nothing."""
    c, f = fp8_case(nv, case)
    O, rg = ragged8(nv, c, f, f["ks"], f["vs"])
    assert torch.equal(rg, ragged(nv, c)[1])
    worst = worst_error(c, O, rg, f["K8"].double() * f["ks"].double()[..., None], f["V8"].double() * f["vs"].double()[..., None])
    O16, r16 = ragged(nv, c)  # beside it: the bf16 call on the case's own bf16 caches against the same reference on those
    print(f"worst |O - float64|: fp8 general scales {worst:.3e}, bf16 call {worst_error(c, O16, r16, c['K'].double(), c['V'].double()):.3e}")
    assert worst <= 1e-2
    ki, vi = f["ks"].clone(), f["vs"].clone()
    for b, t0 in enumerate(c["t_pos"]):
        ki[b, :, max(t0 + c["S"], 0):] = vi[b, :, max(t0 + c["S"], 0):] = float("inf")
    assert torch.equal(ragged8(nv, c, f, ki, vi)[0], O)


def test_nan_scale_of_a_live_row_reaches_the_rows_that_read_it(nv):
    """what the quantiser stores for a row that holds a NaN or an infinity is a NaN scale.  On a V row (sequence 0's own token, group 0; every
    row reads its own token) it makes that (sequence, group)'s output rows NaN and changes no bit of the other group or sequences.  On a K
    row the FP8 call does what the bf16 call does with a NaN in that K row (unit scales, the dequantised caches): the same rows are NaN
    and every other bit is equal -- the epilogue all decode kernels share writes a zero row when the row sum is not > 0, NaN included."""
    c, f = fp8_case(nv, FP8_CASES[0])
    t0 = c["t_pos"][0]
    O, rg = ragged8(nv, c, f, f["ks"], f["vs"])
    z = f["vs"].clone()
    z[0, 0, t0] = float("nan")
    O2, r2 = ragged8(nv, c, f, f["ks"], z)
    assert torch.isnan(O2[0, :, 0].float()).all()
    assert torch.equal(r2, rg) and torch.equal(O2[0, :, 1], O[0, :, 1]) and torch.equal(O2[1:], O[1:])
    z = f["one"].clone()
    z[0, 0, t0] = float("nan")
    O3, r3 = ragged8(nv, c, f, z, f["one"])
    Kn = f["deq"]["K"].clone()
    Kn[0, 0, t0] = float("nan")
    Ob, rb = ragged(nv, dict(f["deq"], K=Kn))
    assert torch.equal(r3, rb) and torch.equal(torch.isnan(O3), torch.isnan(Ob)) and torch.equal(O3.nan_to_num(0.0), Ob.nan_to_num(0.0))
    O1 = ragged8(nv, c, f, f["one"], f["one"])[0]
    assert not torch.equal(O3[0, :, 0], O1[0, :, 0]) and torch.equal(O3[0, :, 1], O1[0, :, 1]) and torch.equal(O3[1:], O1[1:])


def test_table_entry_outside_the_pool_makes_the_sequence_inactive(nv):
    c, f = fp8_case(nv, FP8_CASES[0])
    pl, zk, zv = fp8_pools(c, f, f["ks"], f["vs"])
    O1, r1 = paged(nv, c, pl, k_scale_pool=zk, v_scale_pool=zv)
    for bad in (pl["n_pages"], -1):
        table = [list(r) for r in pl["table"]]
        table[3][1] = bad  # t_pos[3] = 4100 needs entries 0 .. 4
        O, rg = paged(nv, c, pl, table=table, k_scale_pool=zk, v_scale_pool=zv)
        assert not O[3].any() and not rg[3].any()
        assert torch.equal(O[:3], O1[:3]) and torch.equal(rg[:3], r1[:3])


@pytest.mark.parametrize("D", [64, 128])
def test_quantiser(nv, D):
    """nsa_kv_quantize_fp8 on normal rows, an all-zero row and a row holding +-3e4, from a strided source with t0 > 0: scale == torch's fp32
    amax / 448 exactly, bytes == (x.float() / scale).clamp(-448, 448).to(float8_e4m3fn), rows outside [t0, t1) untouched; the paged variant
    through a permuted table row gives the contiguous result"""
    gen = torch.Generator().manual_seed(D)
    big = torch.randn((2, G, 2100, 2 * D), generator=gen).to(BF16)
    big[0, 0, 7] = 0
    big[1, 1, 9, D // 2 + 3], big[1, 1, 9, D // 2 + D - 1] = 3e4, -3e4
    X = big.cuda()[..., D // 2:D // 2 + D]  # row stride 2 D, 16-byte aligned columns
    t0, t1 = 5, 2089
    out = torch.full(X.shape, 0.5, device="cuda").to(FP8)
    sc = torch.full(X.shape[:3], 7.0, device="cuda")
    X8, z = nv.quantize_kv_fp8(X, t0, t1, out=out, scale_out=sc)
    q8, zr = quant(X)
    assert torch.equal(z[:, :, t0:t1].cpu(), zr[:, :, t0:t1]) and z[0, 0, 7] == 1
    assert torch.equal(X8.view(torch.uint8)[:, :, t0:t1].cpu(), q8.view(torch.uint8)[:, :, t0:t1])
    for sl in (slice(0, t0), slice(t1, None)):
        assert (z[:, :, sl] == 7).all() and (X8[:, :, sl].float() == 0.5).all()
    # one slot's tokens [t0, t1) in pages 2, 0, 1 of a pool of 4 (page 3: a spare)
    row, xp = [2, 0, 1], torch.zeros((4, G, PAGE, D), dtype=BF16, device="cuda")
    for j, p in enumerate(row):
        n = min(PAGE, 2100 - PAGE * j)
        xp[p, :, :n] = X[1, :, PAGE * j:PAGE * j + n]
    o8, oz = torch.full(xp.shape, 0.5, device="cuda").to(FP8), torch.full(xp.shape[:3], 7.0, device="cuda")
    nv.quantize_kv_fp8_paged(xp, torch.tensor(row, dtype=torch.int32, device="cuda"), t0, t1, o8, oz)
    for j, p in enumerate(row):
        lo, hi = max(t0, PAGE * j), min(t1, PAGE * j + PAGE)
        assert torch.equal(o8.view(torch.uint8)[p, :, lo - PAGE * j:hi - PAGE * j], X8.view(torch.uint8)[1, :, lo:hi])
        assert torch.equal(oz[p, :, lo - PAGE * j:hi - PAGE * j], z[1, :, lo:hi])
    assert (oz[3] == 7).all() and (oz[2, :, :t0] == 7).all() and (oz[1, :, t1 - 2 * PAGE:] == 7).all()


def test_declines_name_the_limit(nv, tune):
    """f16 queries, a missing scale, a scale with a row stride, scales beside bf16 K / V, DECODE_UNFUSED = 1 and a t_max beyond form 1 with and
    without DECODE_LONG: each raises a message naming the limit, and the plan says launches 0, form -1"""
    c, f = fp8_case(nv, FP8_CASES[0])
    m, one = c["meta"], f["one"]
    args = (c["B"], c["S"], G, c["h"], c["D"], c["D"], m.S_cmp, m.S_sel, c["K"].shape[2], N_TOP)
    declined = {"launches": 0, "form": -1}
    assert nv.selection_decode_ragged_fp8_plan(*args, c["t_max"], torch.float16) == declined
    with pytest.raises(RuntimeError, match="bf16 queries"):
        nv.selection_decode_ragged(c["Q"].half(), c["Kc"].half(), f["K8"], f["V8"], m, N_TOP, c["pos"], t_max=c["t_max"], k_scale=one, v_scale=one)
    with pytest.raises(RuntimeError, match="need both"):
        ragged8(nv, c, f, one, None)
    with pytest.raises(RuntimeError, match="unit row stride"):
        ragged8(nv, c, f, one, one.repeat_interleave(2, dim=-1)[..., ::2])
    with pytest.raises(RuntimeError, match="belong to FP8"):
        ragged(nv, c, k_scale=one, v_scale=one)
    # a t_max beyond form 1 (16 waves: 64 chunks of 64 compressed tokens), with and without the long-row switch
    far = 70000
    mf = nv.build_block_meta(far + 1, m.l, m.d, m.l_sel, N_TOP, 512)
    fargs = (1, 1, G, 6, 64, 64, mf.S_cmp, mf.S_sel, far + 1, N_TOP, far)
    K8 = torch.zeros((1, G, far + 1, 64), dtype=FP8, device="cuda")
    z = torch.ones((1, G, far + 1), device="cuda")
    Q, Kc = dev(torch.zeros((1, 1, G, 6, 64)).numpy(), BF16), dev(torch.zeros((1, G, mf.S_cmp, 64)).numpy(), BF16)
    for long_row in (0, 1):
        tune("DECODE_LONG", long_row)
        assert nv.selection_decode_ragged_fp8_plan(*fargs) == declined
        with pytest.raises(RuntimeError, match="not built for FP8"):
            nv.selection_decode_ragged(Q, Kc, K8, K8, mf, N_TOP, [far], k_scale=z, v_scale=z)
    tune("DECODE_LONG", 0)
    tune("DECODE_UNFUSED", 1)
    assert nv.selection_decode_ragged_fp8_plan(*args, c["t_max"]) == declined
    with pytest.raises(RuntimeError, match="DECODE_UNFUSED"):
        ragged8(nv, c, f, one, one)
