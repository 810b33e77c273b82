"""GPU: the ragged layer decode with FP8 (e4m3) mirrors of the attended slabs (nsa_layer_decode_ragged_fp8, NSAAttention.decode_ragged on an
NSA_KV built with kv_dtype = torch.float8_e4m3fn), against the bf16 call on a pool of the same contents and against float64.
Pools: B = 5 slabs of 1152 tokens, filled through sequence_view + prefill (which requantises what it wrote) over mirrors that start as a
poison pattern (byte 0x2A, scale -3).  Positions: 1037 (compressed row 63, the last of a 64-row K_cmp chunk, completes inside S = 4), 1022
(the rows straddle token 1024 with the window's lower bound active), 20 (no compressed token before token 31: empty-interval rows, the first
one emitted at S = 16), -1 and S_max (padding).  m7c (D = 64) takes the dual band launch, the 128-wide layer one launch per branch.
Measured on the MI355X (max|y - float64| over the live slots, FP8 call / bf16 call, bound 2 x bf16): see DESIGN.md 4.6f."""
import pytest
import torch
import torch.nn.functional as F

from nsa_vibe_amd import batched_causal_attention_compressed, quantize_kv_fp8, sliding_window_attention
from nsa_vibe_amd.nsa_attention import apply_rope
from test_hip_layer_decode_ragged import CACHES, live, mod, same_bits
from test_hip_layer_decode_rows import ncmp

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
MIRRORED = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_cmp", "_V_cmp")
MIRRORS = [n + tail for n in MIRRORED for tail in ("8", "_scale")]
CAP = 1152
POS = [1037, 1022, 20, -1, CAP]
CASES = [(name, S) for name in ("m7c", "d128") for S in (1, 4, 16)]
_FILLED, _RUN = {}, {}


def filled(name):
    """the prefilled FP8 pool of a layer and the sequences' tokens; built once, never modified"""
    if name not in _FILLED:
        m = mod(name)
        kv = m.new_kv(len(POS), CAP, "cuda", torch.bfloat16, kv_dtype=FP8)
        for c in CACHES:
            getattr(kv, c).fill_(float("nan"))
        for c in MIRRORED:
            getattr(kv, c + "8").view(torch.uint8).fill_(0x2A)
            getattr(kv, c + "_scale").fill_(-3.0)
        torch.manual_seed(4100)
        xs = torch.randn(len(POS), CAP + 16, m.dim, device="cuda").to(torch.bfloat16)
        for b, p in enumerate(POS):
            if 0 < p < CAP:
                with torch.no_grad():
                    m(xs[b:b + 1, :p], kv.sequence_view(b), prefill=True)
        _FILLED[name] = (kv, xs)
    return _FILLED[name]


def run(name, S):
    """one FP8 call and one bf16 call on pools of identical contents; shared by the tests, never modified"""
    if (name, S) not in _RUN:
        m, (src, xs) = mod(name), filled(name)
        p8 = m.new_kv(len(POS), CAP, "cuda", torch.bfloat16, kv_dtype=FP8)
        p16 = m.new_kv(len(POS), CAP, "cuda", torch.bfloat16)
        for kv, names in ((p8, list(CACHES) + MIRRORS), (p16, CACHES)):
            for c in names:
                getattr(kv, c).copy_(getattr(src, c))
        before = {c: getattr(p8, c).clone() for c in MIRRORS}
        x = torch.stack([xs[b, p % CAP:p % CAP + S] if p > 0 else xs[b, :S] for b, p in enumerate(POS)])  # (padding slots: any tokens)
        te = max(p for p in POS if 0 <= p < CAP) + S - 1
        outs = []
        for kv in (p8, p16):
            with torch.no_grad():
                y, _ = m.decode_ragged(x, kv, torch.tensor(POS, dtype=torch.int32, device="cuda"), t_max=te)
            outs.append((y, m._last_ranges.clone(), m._last_gates.clone().reshape(len(POS), S, m.n_kv_groups, 3)))
        torch.cuda.synchronize()
        _RUN[(name, S)] = dict(m=m, x=x, te=te, p8=p8, p16=p16, before=before, out8=outs[0], out16=outs[1])
    return _RUN[(name, S)]


@pytest.mark.parametrize("name,S", CASES)
def test_writers_untouched_and_mirror_exact(name, S):
    R = run(name, S)
    p8, te = R["p8"], R["te"]
    assert [live(p, S, te) for p in POS] == [True, True, True, False, False]
    for c in CACHES:
        assert same_bits(getattr(p8, c), getattr(R["p16"], c)), c
    assert torch.equal(R["out8"][1], R["out16"][1])
    assert torch.count_nonzero(R["out8"][0][3:]) == 0 and torch.count_nonzero(R["out8"][1][3:]) == 0  # padding slots: exactly zero
    for c in MIRRORED:  # exactly the rows the call wrote are the quantiser's, every other row is as it was
        q, sc = quantize_kv_fp8(getattr(p8, c))
        exp8, expz = R["before"][c + "8"].view(torch.uint8).clone(), R["before"][c + "_scale"].clone()
        for b, p in enumerate(POS[:3]):
            lo, hi = (ncmp(p), ncmp(p + S)) if "cmp" in c else (p, p + S)
            exp8[b, :, lo:hi], expz[b, :, lo:hi] = q.view(torch.uint8)[b, :, lo:hi], sc[b, :, lo:hi]
        assert torch.equal(getattr(p8, c + "8").view(torch.uint8), exp8) and torch.equal(getattr(p8, c + "_scale"), expz), c


def reference(m, x, kv, out, S, fp8, band=None):
    """float64: Q from the module's weights and RoPE, three softmax attentions over the caches (fp8: the dequantised mirrors) -- the call's
    ranges, its window, n_cmp rows --, the call's gates, the mix, the output projection -> y [B, S, dim], zero for a padding slot.
    band = (O_cmp, O_win) [B,S,G,h,D]: these stand in for the two band branches"""
    _, ranges, gates = out
    G, h, D = m.n_kv_groups, m.h_per_group, m.d_k
    y = torch.zeros(x.shape, dtype=torch.float64, device="cuda")

    def attend(q, K, V, keep):  # q [G,h,D], K / V [G,n,D], keep [G,n] bool
        if not bool(keep.any()):
            return torch.zeros_like(q)
        s = torch.einsum("ghd,gnd->ghn", q, K) / D ** 0.5
        return torch.einsum("ghn,gnd->ghd", torch.softmax(s.masked_fill(~keep[:, None, :], float("-inf")), -1), V)

    for b, p in enumerate(POS[:3]):
        def slab(c):
            n = ncmp(p + S) if "cmp" in c else p + S
            X = getattr(kv, c + "8" if fp8 else c)[b, :, :n].float().double()
            return X * getattr(kv, c + "_scale")[b, :, :n].double()[..., None] if fp8 else X

        Kc, Vc, Ks, Vs, Kw, Vw = (slab(c) for c in ("_K_cmp", "_V_cmp", "_K_sel", "_V_sel", "_K_win", "_V_win"))
        Q = apply_rope(F.linear(x[b:b + 1].double(), m.W_Q.weight.double()), torch.arange(p, p + S, device="cuda"), scale=m.rope_scale).view(S, G, h, D)
        k = torch.arange(p + S, device="cuda")
        for s in range(S):
            t = p + s
            sel = torch.zeros((G, p + S), dtype=torch.bool, device="cuda")
            for g in range(G):
                for lo, hi in ranges[b, s, g].tolist():
                    sel[g, lo:min(hi, t + 1)] = True
            O = [attend(Q[s], Kc, Vc, (torch.arange(ncmp(p + S), device="cuda") < ncmp(t + 1)).expand(G, -1)), attend(Q[s], Ks, Vs, sel),
                 attend(Q[s], Kw, Vw, ((k <= t) & (k > t - m.w)).expand(G, -1))]
            if band is not None:
                O[0], O[2] = band[0][b, s].double(), band[1][b, s].double()
            mix = sum(gates[b, s, :, i].double()[:, None, None] * O[i] for i in range(3))
            y[b, s] = F.linear(mix.reshape(-1), m.out.weight.double())
    return y


@pytest.mark.parametrize("name,S", CASES)
def test_y_against_float64(name, S):
    R = run(name, S)
    err = {}
    for key, kv, fp8 in (("fp8", R["p8"], True), ("bf16", R["p16"], False)):
        out = R["out8" if fp8 else "out16"]
        assert torch.isfinite(out[0][:3].float()).all(), key
        err[key] = (out[0].double() - reference(R["m"], R["x"], kv, out, S, fp8)).abs().max().item()
    print(f"{name} S={S}: max|y - float64| fp8 {err['fp8']:.3e}, bf16 {err['bf16']:.3e} (bound 2 x bf16 = {2 * err['bf16']:.3e})")
    assert err["fp8"] <= 2 * err["bf16"], err


@pytest.mark.parametrize("S", [1, 4, 16])
def test_dual_launch_against_separate_fp8_launches(S):
    """m7c: y of the call (one dual launch, records merged by the finish kernel) against the composition whose two band branches are the
    public FP8 operators on the same mirrors (each combines in its own pass), the rest float64: within 1e-2"""
    R = run("m7c", S)
    m, kv, x = R["m"], R["p8"], R["x"]
    G, h, D = m.n_kv_groups, m.h_per_group, m.d_k
    t_pos = torch.tensor(POS, dtype=torch.int32, device="cuda")
    Q = torch.zeros((len(POS), S, G, h, D), dtype=torch.bfloat16, device="cuda")
    kw = dict(t_pos=t_pos, t_max=R["te"], scale=D ** -0.5)
    with torch.no_grad():
        for b, p in enumerate(POS[:3]):
            Q[b] = apply_rope(F.linear(x[b:b + 1].double(), m.W_Q.weight.double()), torch.arange(p, p + S, device="cuda"), scale=m.rope_scale).view(S, G, h, D)
        O_win = sliding_window_attention(Q, kv._K_win8, kv._V_win8, m.w, k_scale=kv._K_win_scale, v_scale=kv._V_win_scale, **kw)
        O_cmp = batched_causal_attention_compressed(Q, kv._K_cmp8, kv._V_cmp8, m.l, m.d, k_scale=kv._K_cmp_scale, v_scale=kv._V_cmp_scale, **kw)
        torch.cuda.synchronize()
        y_sep = reference(m, x, kv, R["out8"], S, True, band=(O_cmp, O_win))
    err = (R["out8"][0].double() - y_sep).abs().max().item()
    print(f"m7c S={S}: max|y(dual launch) - y(separate FP8 launches)| {err:.3e}")
    assert err <= 1e-2
