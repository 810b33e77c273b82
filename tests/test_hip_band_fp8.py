"""FP8 (OCP e4m3) K/V caches of the sliding and the compressed branch of a ragged decode step (nsa_band_attn_fwd_ragged_fp8 / _paged_fp8; the
keyword arguments k_scale / v_scale of band_attention_hip, sliding_window_attention and batched_causal_attention_compressed) and the paged
quantiser on pages of any size.  The cases, their inputs and the page scatter are those of tests/test_hip_band_ragged.py and
tests/test_hip_band_paged.py; K / V are quantised with torch on the CPU (amax / 448) and poisoned in FP8 terms: rows behind a sequence's own
keys and unused pool pages hold +-448 with scale 64."""
import numpy as np
import pytest
import torch

from test_hip_band_paged import BANDS, PAGE, key_rows, scatter, unsplit_case
from test_hip_band_ragged import G, SETS, make_case
from test_hip_selection import dev, nv  # noqa: F401

pytestmark = pytest.mark.gpu

FP8, BF16 = torch.float8_e4m3fn, torch.bfloat16
BRANCHES = ["sliding", "compressed"]
EDGES = ([1022, 1023, 1024, 2047, 2048], 3)


def quant(X, seed):
    """torch's amax / 448 quantisation, then each row's scale times a power of two p in [1/8, 8] and its bytes divided by p: X^ = X8 * scale
    stays the unit-normal data the 1e-2 bound is stated for, and a dropped or misindexed scale cannot cancel"""
    Xf = X.float().cpu()
    amax = Xf.abs().amax(-1)
    sc = torch.where(amax == 0, torch.ones_like(amax), amax / 448)
    p = torch.exp2(torch.randint(-3, 4, sc.shape, generator=torch.Generator().manual_seed(seed)).float())
    return (Xf / (sc * p)[..., None]).clamp(-448, 448).to(FP8), sc * p


def own_rows(c, branch, b):
    t0 = c["t_pos"][b]
    return key_rows(BANDS[branch], t0, c["S"])[1] if t0 >= 0 else 0


def fp8_case(c, branch):
    """the FP8 caches of a case and branch, made once: K8 / V8 / ks / vs (general scales), ones, and the dequantised bf16 caches"""
    key = ("f8", branch)
    if key not in c:
        K, V = c["kv"][branch]
        (K8, ks), (V8, vs) = quant(K, 2 * K.shape[2]), quant(V, 2 * K.shape[2] + 1)
        for b in range(c["B"]):
            own = own_rows(c, branch, b)
            K8.view(torch.uint8)[b, :, own:], V8.view(torch.uint8)[b, :, own:] = 0x7E, 0xFE  # +448, -448
            ks[b, :, own:] = vs[b, :, own:] = 64
        c[key] = dict(K8=K8.cuda(), V8=V8.cuda(), ks=ks.cuda(), vs=vs.cuda(), one=torch.ones_like(ks).cuda(), Kd=K8.to(BF16).cuda(), Vd=V8.to(BF16).cuda())
    return c[key]


def get_case(kind, a, D, h=6):
    c = unsplit_case(a, D) if kind == "unsplit" else make_case(*(EDGES if a == "edges" else SETS[a]), D, BF16)
    if h != 6 and ("Q", h) not in c:
        c["Q", h] = dev(np.random.default_rng(h).standard_normal((c["B"], c["S"], G, h, D), dtype=np.float32), BF16)
    return c, (c["Q"] if h == 6 else c["Q", h])


def call(nv, c, Q, K, V, branch, **kw):
    return nv.band_attention_hip(Q, K, V, return_lse=True, t_pos=c["pos"], t_max=c["t_max"], **BANDS[branch], **kw)


def assert_equal_bits(got, ref):
    torch.cuda.synchronize()
    assert torch.isfinite(got[0].float()).all()
    assert torch.equal(got[1], ref[1]) and torch.equal(got[0], ref[0])


UNIT = [("set", "S1_mixed", 64), ("set", "S1_mixed", 128), ("set", "S3_boundaries", 64), ("set", "S3_boundaries", 128), ("unsplit", 32, 64),
        ("unsplit", 32, 128), ("unsplit", 256, 64), ("unsplit", 256, 128), ("set", "S3_boundaries", 64, 16), ("set", "S3_boundaries", 64, 1)]


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("spec", UNIT, ids=lambda s: "-".join(map(str, s)))
def test_unit_scales_are_the_bf16_call_bit_for_bit(nv, spec, branch):
    """all scales 1.0f: O and lse torch.equal with the bf16 ragged call on K8.to(bf16), V8.to(bf16) -- the split form (both SETS, D = 64 and
    128, h = 6, 16 and 1) and the unsplit forms NT = 1 (S = 32) and NT = 3 / 2 (S = 256)"""
    c, Q = get_case(*spec)
    f = fp8_case(c, branch)
    got = call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=f["one"], v_scale=f["one"])
    assert got[0].dtype == BF16
    assert_equal_bits(got, call(nv, c, Q, f["Kd"], f["Vd"], branch))


def fp8_pools(c, f, branch, rows):
    """scatter() on the dequantised caches, the pools back to FP8 (exact; the bf16 poison saturates to +-448), the scales through the same table"""
    pl = scatter(f["Kd"], f["Vd"], c["t_pos"], c["S"], BANDS[branch], rows, seed=len(c["t_pos"]) + c["S"] + rows)
    zk, zv = (torch.full((pl["n_pages"], G, rows), 64.0, device="cuda") for _ in range(2))
    for b, t0 in enumerate(c["t_pos"]):
        lo, hi = key_rows(BANDS[branch], t0, c["S"]) if t0 >= 0 else (0, 0)
        for j in range(lo // rows, (hi - 1) // rows + 1) if hi > lo else ():
            r, p = min(rows, hi - rows * j), pl["table"][b][j]
            zk[p, :, :r], zv[p, :, :r] = f["ks"][b, :, rows * j:rows * j + r], f["vs"][b, :, rows * j:rows * j + r]
    to8 = lambda X: X.float().clamp(-448, 448).to(FP8)  # noqa: E731
    return dict(pl, K=to8(pl["K"]), V=to8(pl["V"]), ks=zk, vs=zv)


def paged8(nv, c, Q, pl, branch, table=None):
    tb = torch.tensor(pl["table"] if table is None else table, dtype=torch.int32, device="cuda")
    return call(nv, c, Q, pl["K"], pl["V"], branch, k_scale=pl["ks"], v_scale=pl["vs"], block_table=tb)


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("name,D,rows", [("S1_mixed", 64, None), ("S3_boundaries", 128, None), ("S3_boundaries", 64, 32), ("edges", 64, None),
                                         ("unsplit", 64, None)])
def test_paged_fp8_is_the_ragged_fp8_call_bit_for_bit(nv, name, D, rows, branch):
    """general scales behind a permuted table: pages of 1024 (sliding) / 64 (compressed) rows, pages of 32 rows where every unaligned tile
    straddles, positions at page edges, and the unsplit NT = 3 form"""
    c, Q = get_case("unsplit", 256, D) if name == "unsplit" else get_case("set", name, D)
    f = fp8_case(c, branch)
    pl = fp8_pools(c, f, branch, rows or PAGE[branch])
    assert_equal_bits(paged8(nv, c, Q, pl, branch), call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=f["ks"], v_scale=f["vs"]))


def float64_ref(c, Q, Kh, Vh, branch):
    """plain float64 softmax attention of every row over its [lo, hi) on Kh, Vh [B,G,n,D] -> O, lse (zeros / -inf for an empty interval)"""
    band, D = BANDS[branch], Q.shape[-1]
    O = torch.zeros(Q.shape, dtype=torch.float64, device="cuda")
    lse = torch.full(Q.shape[:-1], -float("inf"), dtype=torch.float64, device="cuda")
    for b, t0 in enumerate(c["t_pos"]):
        for s in range(c["S"] if t0 >= 0 else 0):
            hi = key_rows(band, t0 + s, 1)[1]
            lo = max(0, hi - band["w"])
            if hi > lo:
                x = torch.einsum("ghd,gkd->ghk", Q[b, s].double(), Kh[b, :, lo:hi]) * D ** -0.5
                lse[b, s] = torch.logsumexp(x, -1)
                O[b, s] = torch.einsum("ghk,gkd->ghd", torch.softmax(x, -1), Vh[b, :, lo:hi])
    return O, lse


def worst(got, ref):
    live = torch.isfinite(ref[1])
    assert torch.equal(torch.isfinite(got[1]), live) and not got[0][~live].any()  # inactive slots and empty rows: zero rows, lse = -inf
    return (got[0].double() - ref[0]).abs().max().item(), (got[1].double() - ref[1])[live].abs().max().item()


@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("name,D", [("S1_mixed", 64), ("S3_boundaries", 64), ("S3_boundaries", 128)])
def test_general_scales_against_float64(nv, name, D, branch):
    """O against float64 on K^ = K8 * k_scale, V^ = V8 * v_scale: 1e-2 absolute, the project's bf16 bound -- as in the bf16 kernels one
    rounding on P and one on O.  lse: the kernel's logits, exponentials and row sum are fp32 in both forms (nothing is rounded to bf16 on
    the way to lse), so its error is that of the bf16 ragged call on the dequantised caches against the same reference, plus two more fp32
    roundings per logit (c2 * k_scale and the product): 2^-23 of a logit below 64 nats, 1e-5.  Bound: twice the bf16 call's worst + 1e-5.
    Scales of rows behind each sequence's own keys set to inf change no bit."""
    c, Q = get_case("set", name, D)
    f = fp8_case(c, branch)
    got = call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=f["ks"], v_scale=f["vs"])
    Kh, Vh = f["K8"].double() * f["ks"].double()[..., None], f["V8"].double() * f["vs"].double()[..., None]
    dO, dl = worst(got, float64_ref(c, Q, Kh, Vh, branch))
    Kb, Vb = Kh.to(BF16), Vh.to(BF16)  # beside it: the bf16 call on the dequantised caches against float64 on those
    dO16, dl16 = worst(call(nv, c, Q, Kb, Vb, branch), float64_ref(c, Q, Kb.double(), Vb.double(), branch))
    print(f"band fp8 {branch} {name} D={D}: worst |dO| {dO:.3e} (bf16 call {dO16:.3e}), worst |dlse| {dl:.3e} (bf16 call {dl16:.3e})")
    assert dO <= 1e-2
    assert dl <= 2 * dl16 + 1e-5
    ki, vi = f["ks"].clone(), f["vs"].clone()
    for b in range(c["B"]):
        ki[b, :, own_rows(c, branch, b):] = vi[b, :, own_rows(c, branch, b):] = float("inf")
    assert_equal_bits(call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=ki, v_scale=vi), got)


@pytest.mark.parametrize("branch", BRANCHES)
def test_nan_scale_of_a_live_key_reaches_the_rows_that_read_it(nv, branch):
    """what the quantiser stores for a row that holds a NaN or an infinity is a NaN scale.  On a V row (sequence 0's last key row, group 1) it
    makes that (sequence, group)'s output rows NaN and changes no bit of lse, of the other group or of the other sequences.  On a K row the
    FP8 call does what the bf16 call does with a NaN in that K row (unit scales, the dequantised caches): the same elements of O and lse
    are NaN and every other bit is equal -- the epilogues the band kernels share write a zero row when the row sum is not > 0, NaN included."""
    c, Q = get_case("set", "S1_mixed", 64)
    f = fp8_case(c, branch)
    r = own_rows(c, branch, 0) - 1
    O, lse = call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=f["ks"], v_scale=f["vs"])
    z = f["vs"].clone()
    z[0, 1, r] = float("nan")
    O2, lse2 = call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=f["ks"], v_scale=z)
    assert torch.isnan(O2[0, :, 1].float()).all()
    assert torch.equal(O2[0, :, 0], O[0, :, 0]) and torch.equal(O2[1:], O[1:]) and torch.equal(lse2, lse)
    z = f["one"].clone()
    z[0, 1, r] = float("nan")
    O3, lse3 = call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=z, v_scale=f["one"])
    Kn = f["Kd"].clone()
    Kn[0, 1, r] = float("nan")
    Ob, lseb = call(nv, c, Q, Kn, f["Vd"], branch)
    for got, ref in ((O3, Ob), (lse3, lseb)):
        assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got.nan_to_num(0.0), ref.nan_to_num(0.0))
    O1, lse1 = call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=f["one"], v_scale=f["one"])
    assert not torch.equal(O3[0, :, 1], O1[0, :, 1]) and torch.equal(O3[0, :, 0], O1[0, :, 0]) and torch.equal(O3[1:], O1[1:])


@pytest.mark.parametrize("branch", BRANCHES)
def test_table_entry_outside_the_pool_makes_the_sequence_inactive(nv, branch):
    c, Q = get_case("set", "S1_mixed", 64)
    f = fp8_case(c, branch)
    pl = fp8_pools(c, f, branch, PAGE[branch])
    ref = paged8(nv, c, Q, pl, branch)
    j = (key_rows(BANDS[branch], 4100, 1)[1] - 1) // PAGE[branch]  # sequence 3 (t = 4100): the entry of its last key row
    for bad in (pl["n_pages"], -1):
        table = [list(r) for r in pl["table"]]
        table[3][j] = bad
        O, lse = paged8(nv, c, Q, pl, branch, table=table)
        torch.cuda.synchronize()
        assert not O[3].any() and bool((lse[3] == -float("inf")).all())
        keep = [0, 1, 2, 4]
        assert torch.equal(O[keep], ref[0][keep]) and torch.equal(lse[keep], ref[1][keep])


@pytest.mark.parametrize("branch", BRANCHES)
def test_paged_quantiser_on_pages_of_the_branch(nv, branch):
    """quantize_kv_fp8_paged through a permuted table row (pages of 1024 rows: the existing symbol; 64 rows: nsa_paged_kv_quantize_fp8_rows)
    equals quantize_kv_fp8 on the contiguous tensor: bytes and scales, rows outside [t0, t1) untouched"""
    rows, D, n, t0, t1 = PAGE[branch], 64, 2 * PAGE[branch] + 37, 5, 2 * PAGE[branch] + 30
    X = torch.randn((1, G, n, D), generator=torch.Generator().manual_seed(rows)).to(BF16).cuda()
    X8, z = nv.quantize_kv_fp8(X, t0, t1)
    row, xp = [2, 0, 3], torch.zeros((5, G, rows, D), dtype=BF16, device="cuda")
    for j, p in enumerate(row):
        m = min(rows, n - rows * j)
        xp[p, :, :m] = X[0, :, rows * j:rows * j + m]
    o8, oz = torch.full(xp.shape, 0.5, device="cuda").to(FP8), torch.full(xp.shape[:3], 7.0, device="cuda")
    nv.quantize_kv_fp8_paged(xp, torch.tensor(row, dtype=torch.int32, device="cuda"), t0, t1, o8, oz)
    for j, p in enumerate(row):
        lo, hi = max(t0, rows * j) - rows * j, min(t1, rows * j + rows) - rows * j
        assert torch.equal(o8.view(torch.uint8)[p, :, lo:hi], X8.view(torch.uint8)[0, :, rows * j + lo:rows * j + hi])
        assert torch.equal(oz[p, :, lo:hi], z[0, :, rows * j + lo:rows * j + hi])
        assert (oz[p, :, :lo] == 7).all() and (oz[p, :, hi:] == 7).all() and (o8[p, :, hi:].float() == 0.5).all()
    assert (oz[[1, 4]] == 7).all()


@pytest.mark.parametrize("branch", BRANCHES)
def test_declines_name_the_limit(nv, branch):
    c, Q = get_case("set", "S3_boundaries", 64)
    f = fp8_case(c, branch)
    K8, V8, one = f["K8"], f["V8"], f["one"]
    with pytest.raises(RuntimeError, match="bf16 queries"):
        call(nv, c, Q.half(), K8, V8, branch, k_scale=one, v_scale=one)
    with pytest.raises(RuntimeError, match="need both"):
        call(nv, c, Q, K8, V8, branch, k_scale=one)
    with pytest.raises(RuntimeError, match="unit row stride"):
        call(nv, c, Q, K8, V8, branch, k_scale=one, v_scale=one.repeat_interleave(2, dim=-1)[..., ::2])
    with pytest.raises(RuntimeError, match="belong to FP8"):
        call(nv, c, Q, f["Kd"], f["Vd"], branch, k_scale=one, v_scale=one)
    with pytest.raises(RuntimeError, match="need the per-sequence positions t_pos"):
        nv.band_attention_hip(Q, K8, V8, t0=1052, k_scale=one, v_scale=one, **BANDS[branch])
    with pytest.raises(RuntimeError, match="forward only"):
        call(nv, c, Q.clone().requires_grad_(True), K8, V8, branch, k_scale=one, v_scale=one)
