"""GPU: the paged layer decode with FP8 (e4m3) mirrors of the attended pools (nsa_layer_decode_paged_fp8, NSAAttention.decode_paged on an
NSA_PagedKV built with kv_dtype = torch.float8_e4m3fn).

Pools come from test_hip_layer_decode_paged.paged_of (B = 1 prefills scattered into poisoned pages); the mirrors start as a poison pattern
(byte 0x2A, scale -3) with the sequences' earlier rows quantised by the public quantiser.  Slots: two pages of token rows (1022 + 4 rows; 1024
at S = 1), compressed row 63 emitted into the last row of compressed page 0 from raw rows 1008 .. 1039, row 64 into page 1, a slot at -1 and a
slot whose needed table entry is n_pages.  The torch expression of a mirror row runs on the CPU, as in test_hip_decode_fp8.

Measured on the MI355X (max|y - float64| over the live slots, FP8 call / bf16 call, bound 2 x bf16): see DESIGN.md 4.6e."""
import pytest
import torch
import torch.nn.functional as F

from test_hip_layer_decode_paged import CAP, MAX_PAGES, is_live, model, paged_of, pools
from test_hip_layer_decode_ragged import CACHES, pool_of, same_bits
from test_hip_layer_decode_rows import ncmp

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
MIRRORED = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_cmp", "_V_cmp")
POSITIONS = {4: [1022, 1036, 1052, -1, 1036], 1: [1024, 1039, 1055, -1, 1039]}
T_MAX, N_PAGES = 1055, 12
BAD = {(4, 1): N_PAGES}
CASES = [("m7c", 1), ("m7c", 4), ("d128", 1), ("d128", 4)]


def rows_pp(name):
    return 64 if "cmp" in name else 1024


def span(name, p, S):
    """the rows of pool `name` a call at position p writes"""
    return (ncmp(p), ncmp(p + S)) if "cmp" in name else (p, p + S)


def quant_ref(X):
    """bf16 rows [..., D] -> (bytes uint8, scale fp32, bad) by the torch expression, on the CPU; bad: rows with a NaN or an infinity"""
    Xf = X.float().cpu()
    amax = Xf.abs().amax(-1)
    bad = ~torch.isfinite(amax)
    sc = torch.where((amax == 0) | bad, torch.ones_like(amax), amax / 448)
    return (Xf / sc[..., None]).clamp(-448, 448).to(FP8).view(torch.uint8), sc, bad


def add_mirrors(pkv, positions):
    pkv.kv_dtype = FP8
    for name in MIRRORED:
        pool = getattr(pkv, name)
        setattr(pkv, name + "8", torch.full(pool.shape, 0x2A, dtype=torch.uint8, device="cuda").view(FP8))
        setattr(pkv, name + "_scale", torch.full(pool.shape[:3], -3.0, device="cuda"))
    for b, p in enumerate(positions):
        if p > 0:
            pkv._requantize(pkv.block_table[b], 0, p, 0, ncmp(p))
    torch.cuda.synchronize()
    return pkv


def mirrors(pkv):
    return {name: (getattr(pkv, name + "8").view(torch.uint8).cpu(), getattr(pkv, name + "_scale").cpu()) for name in MIRRORED}


def decode(m, x, pkv, positions):
    t_pos = torch.tensor(positions, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        y, _ = m.decode_paged(x, pkv, t_pos, t_max=T_MAX)
    torch.cuda.synchronize()
    return y, m._last_ranges.clone(), m._last_gates.clone().reshape(len(positions), x.shape[1], m.n_kv_groups, 3)


_RUN = {}


def run(name, S, order=5):
    """one FP8 call and one bf16 call on identical pools; shared by the tests, never modified"""
    if (name, S, order) not in _RUN:
        m, pos = model(name), POSITIONS[S]
        _, slabs, x = pool_of(name, pos, CAP, S)
        p8 = add_mirrors(paged_of(m, slabs, pos, S, n_pages=N_PAGES, order=order, bad=BAD), pos)
        p16 = paged_of(m, slabs, pos, S, n_pages=N_PAGES, order=order, bad=BAD)
        before = mirrors(p8)
        _RUN[(name, S, order)] = dict(m=m, x=x, pos=pos, p8=p8, p16=p16, before=before, out8=decode(m, x, p8, pos), out16=decode(m, x, p16, pos))
    return _RUN[(name, S, order)]


def check_mirrors(pkv, before, pos, S):
    """every row the call should have written is the torch expression of its bf16 row (a non-finite row: NaN scale, NaN bytes), every other
    row of every mirror is as it was -> the number of non-finite rows seen"""
    n_bad = 0
    for name, (got8, gotz) in mirrors(pkv).items():
        exp8, expz = before[name][0].clone(), before[name][1].clone()
        r = rows_pp(name)
        for b, p in enumerate(pos):
            if not is_live(pkv, b, p, S, T_MAX):
                continue
            for row in range(*span(name, p, S)):
                at = (pkv.table[b][row // r], slice(None), row % r)
                q, sc, bad = quant_ref(getattr(pkv, name)[at])
                for g in torch.nonzero(bad).flatten().tolist():
                    assert torch.isnan(gotz[at][g]) and bool(((got8[at][g] & 0x7F) == 0x7F).all()), (name, b, row, g)
                    q[g], sc[g] = got8[at][g], 0.0
                    gotz[at][g] = 0.0
                n_bad += int(bad.sum())
                exp8[at], expz[at] = q, sc
        assert torch.equal(got8, exp8) and torch.equal(gotz.view(torch.int32), expz.view(torch.int32)), name
    return n_bad


@pytest.mark.parametrize("name,S", CASES)
def test_writers_untouched_and_mirror_exact(name, S):
    R = run(name, S)
    m, pos = R["m"], R["pos"]
    assert [b for b, p in enumerate(pos) if not is_live(R["p8"], b, p, S, T_MAX)] == [3, 4]
    a, b = pools(R["p8"]), pools(R["p16"])
    for c in CACHES:
        assert same_bits(a[c], b[c]), c
    assert torch.equal(R["out8"][1], R["out16"][1]) and torch.equal(R["out8"][2][:3], R["out16"][2][:3])
    assert check_mirrors(R["p8"], R["before"], pos, S) == 0
    # a non-finite appended row: V_win element 0 overflows for slot 0 (its x column 0 is 2, the weight 3e38); Q, K and the ranges stay finite
    W, x = m.W_V_win.weight, R["x"].clone()
    x[0, :, 0] = 2.0
    saved = W[0, 0].item()
    _, slabs, _ = pool_of(name, pos, CAP, S)
    p8 = add_mirrors(paged_of(m, slabs, pos, S, n_pages=N_PAGES, order=5, bad=BAD), pos)
    before = mirrors(p8)
    try:
        with torch.no_grad():
            W[0, 0] = 3e38
        decode(m, x, p8, pos)
    finally:
        with torch.no_grad():
            W[0, 0] = saved
    assert check_mirrors(p8, before, pos, S) >= S


def gather(pool, table_b, n, r, scale=None):
    """rows [0, n) of a sequence through its table row -> float64 [G, n, D] (scale: the mirror's scale pool, dequantised)"""
    idx = torch.arange(n, device="cuda")
    pages = torch.tensor(table_b, device="cuda")[idx // r]
    X = pool[pages, :, idx % r].float().double()
    if scale is not None:
        X = X * scale[pages, :, idx % r].double()[..., None]
    return X.permute(1, 0, 2)


def reference(m, x, pkv, out, pos, S, fp8):
    """float64: Q from the module's weights and RoPE, three softmax attentions over the caches (fp8: the dequantised mirrors) -- the call's
    ranges, its window, n_cmp rows --, the call's gates, the mix, the output projection -> y [B, S, dim], zero for a slot that is not live"""
    from nsa_vibe_amd.nsa_attention import apply_rope

    _, ranges, gates = out
    G, h, D = m.n_kv_groups, m.h_per_group, m.d_k
    y = torch.zeros(x.shape, dtype=torch.float64, device="cuda")
    caches = {}
    for b, p in enumerate(pos):
        if not is_live(pkv, b, p, S, T_MAX):
            continue
        for name in MIRRORED:
            n = ncmp(p + S) if "cmp" in name else p + S
            caches[name] = gather(getattr(pkv, name + "8"), pkv.table[b], n, rows_pp(name), getattr(pkv, name + "_scale")) if fp8 else \
                gather(getattr(pkv, name), pkv.table[b], n, rows_pp(name))
        tpos = torch.arange(p, p + S, device="cuda")
        Q = apply_rope(F.linear(x[b:b + 1].double(), m.W_Q.weight.double()), tpos, scale=m.rope_scale).view(S, G, h, D)

        def attend(q, K, V, keep):  # q [G,h,D], K / V [G,n,D], keep [G,n] bool
            if not bool(keep.any()):
                return torch.zeros_like(q)
            s = torch.einsum("ghd,gnd->ghn", q, K) / D ** 0.5
            return torch.einsum("ghn,gnd->ghd", torch.softmax(s.masked_fill(~keep[:, None, :], float("-inf")), -1), V)

        for s in range(S):
            t = p + s
            k = torch.arange(p + S, device="cuda")
            sel = torch.zeros((G, p + S), dtype=torch.bool, device="cuda")
            for g in range(G):
                for lo, hi in ranges[b, s, g].tolist():
                    sel[g, lo:min(hi, t + 1)] = True
            win = ((k <= t) & (k > t - m.w)).expand(G, -1)
            cmp = (torch.arange(ncmp(p + S), device="cuda") < ncmp(t + 1)).expand(G, -1)
            O = [attend(Q[s], caches["_K_cmp"], caches["_V_cmp"], cmp), attend(Q[s], caches["_K_sel"], caches["_V_sel"], sel),
                 attend(Q[s], caches["_K_win"], caches["_V_win"], win)]
            mix = sum(gates[b, s, :, i].double()[:, None, None] * O[i] for i in range(3))
            y[b, s] = F.linear(mix.reshape(-1), m.out.weight.double())
    return y


@pytest.mark.parametrize("name,S", CASES)
def test_y_against_float64(name, S):
    R = run(name, S)
    m, x, pos = R["m"], R["x"], R["pos"]
    err = {}
    for key, pkv, fp8 in (("fp8", R["p8"], True), ("bf16", R["p16"], False)):
        y = R["out8" if fp8 else "out16"][0]
        ref = reference(m, x, pkv, R["out8" if fp8 else "out16"], pos, S, fp8)
        assert torch.isfinite(y[:3].float()).all() and torch.count_nonzero(y[3:]) == 0, key  # dead slots: exactly zero
        err[key] = (y.double() - ref).abs().max().item()
    print(f"{name} S={S}: max|y - float64| fp8 {err['fp8']:.3e}, bf16 {err['bf16']:.3e} (bound 2 x bf16 = {2 * err['bf16']:.3e})")
    assert err["fp8"] <= 2 * err["bf16"], err


@pytest.mark.parametrize("name,S", CASES)
def test_table_independence(name, S):
    a, b = run(name, S, None), run(name, S, 5)
    assert a["p8"].table != b["p8"].table
    assert torch.equal(a["out8"][0], b["out8"][0]) and torch.equal(a["out8"][1], b["out8"][1])
    for c in MIRRORED:
        for s in range(3):
            n = span(c, a["pos"][s], S)[1]
            u8, v8 = (gather(getattr(r["p8"], c + "8").view(torch.uint8), r["p8"].table[s], n, rows_pp(c)) for r in (a, b))
            uz, vz = (gather(getattr(r["p8"], c + "_scale").unsqueeze(-1), r["p8"].table[s], n, rows_pp(c)) for r in (a, b))
            assert torch.equal(u8, v8) and torch.equal(uz, vz), (c, s)


@pytest.mark.parametrize("name,S", CASES)
def test_prefill_fork_decode_through_the_allocator(name, S):
    m, T = model(name), 1045  # page 0 is closed at 1045 (>= 1040): the fork shares it and copies page 1
    torch.manual_seed(31)
    x0 = torch.randn(1, T, m.dim, device="cuda").to(torch.bfloat16)
    x = torch.randn(1, S, m.dim, device="cuda").to(torch.bfloat16).expand(2, S, m.dim).contiguous()
    ys = []
    for forked in (True, False):
        pkv = m.new_paged_kv(6, 2, MAX_PAGES, "cuda", torch.bfloat16, kv_dtype=FP8)
        with torch.no_grad():
            m.prefill_paged(x0, pkv, 0)
            if forked:
                pkv.fork(0, 1, T)
                assert pkv.shared_pages(1) == [pkv.pages[0][0]] and pkv.pages[1][1] != pkv.pages[0][1]
            else:
                m.prefill_paged(x0, pkv, 1)
        for b in range(2):
            pkv.ensure(b, T + S)
        ys.append(decode(m, x, pkv, [T, T])[0])
        for b in range(2):  # the purity invariant: every live mirror row is the quantisation of its bf16 row
            for c in MIRRORED:
                n, r = span(c, T, S)[1], rows_pp(c)
                q, sc, bad = quant_ref(gather(getattr(pkv, c), pkv.pages[b], n, r).to(torch.bfloat16))
                assert not bool(bad.any())
                assert torch.equal(gather(getattr(pkv, c + "8").view(torch.uint8), pkv.pages[b], n, r).to(torch.uint8).cpu(), q), (forked, b, c)
                assert torch.equal(gather(getattr(pkv, c + "_scale").unsqueeze(-1), pkv.pages[b], n, r)[..., 0].float().cpu(), sc), (forked, b, c)
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0][0], ys[0][1])
