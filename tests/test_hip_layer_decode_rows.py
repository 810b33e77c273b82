"""GPU parity: the decode step of the whole layer for S consecutive tokens in one call (nsa_layer_decode_rows, NSAAttention.decode_rows).

The reference of every comparison is S calls of the existing single decode step (nsa_layer_decode_step through forward(prefill=False)) on a
clone of the same filled cache, never the code under test.  Where both sides project on the MFMA form (B >= 3) the cached rows, the pooled
tokens and the ranges are the single steps' bit for bit; y is compared to the bar of test_hip_extend.py (the band branches of the rows call
run another split count), the gates to the 1-ulp bar test_hip_gate.py holds every kernel copy of the gate to.  At B = 1 the single step
projects on the VALU form and the cached rows agree up to the rounding of the projection (test_hip_extend.py's bars).

Figures seen on the MI355X are printed by every comparison (pytest -s)."""
import ctypes

import pytest
import torch

from test_hip_extend import _clone_kv
from test_hip_gate import ULP1
from test_hip_selection import norm

pytestmark = pytest.mark.gpu

TOKEN_CACHES = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw")
READS = ("reads_pred", "reads_act_total", "reads_act_sel", "reads_act_cmp", "reads_act_win")


def ncmp(n_tok):
    return 0 if n_tok < 32 else (n_tok - 32) // 16 + 1


def module(dim=768, H=12, G=2, D=64, dtype=torch.bfloat16, seed=11):
    from nsa_vibe_amd.nsa_attention import NSAAttention

    torch.manual_seed(seed)
    m = NSAAttention(dim, H, G, D, D, l=32, d=16, l_sel=64, n_sel=16, w=512, selector="sequential")
    return m.cuda().to(dtype).eval()


def single_steps(m, x, kv):
    """S single decode steps on kv (modified in place) -> y [B,S,dim], ranges [B,S,G,n,2], gates [B,S,G,3]"""
    ys, rs, gs = [], [], []
    with torch.no_grad():
        for s in range(x.shape[1]):
            y, _ = m(x[:, s:s + 1], kv, prefill=False)
            ys.append(y)
            rs.append(m._last_ranges.clone().unsqueeze(1))
            gs.append(m._last_gates.clone().reshape(x.shape[0], 1, m.n_kv_groups, 3))
    return torch.cat(ys, dim=1), torch.cat(rs, dim=1), torch.cat(gs, dim=1)


def rows_cabi(m, x, kv):
    """one nsa_layer_decode_rows call through the C ABI on kv (modified in place) -> y, ranges, gates, the plan of the call"""
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _stream

    B, S, _ = x.shape
    t0, meta = kv.begin_rows(S)
    L, dev = _lib.lib(), x.device
    desc, _ = m._layer_desc()
    kd = kv.native_desc()
    plan = m.decode_rows_plan(B, S, kd.S_max, t0, int(meta.S_sel))
    ranges = torch.full((B, S, m.n_kv_groups, m.n_sel, 2), -7, dtype=torch.int32, device=dev)
    gates = torch.full((B, S, m.n_kv_groups, 3), float("nan"), dtype=torch.float32, device=dev)
    y = torch.full((B, S, m.dim), float("nan"), dtype=x.dtype, device=dev)
    nb = L.nsa_layer_decode_rows_workspace(ctypes.byref(desc), B, S, kd.S_max)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
    wptr = (ws.data_ptr() + 255) & ~255
    cptr, crows, cvals = meta.device_csc(dev)
    xc = x.contiguous()
    rc = L.nsa_layer_decode_rows(ctypes.byref(desc), ctypes.byref(kd), xc.data_ptr(), y.data_ptr(), t0, S, cptr.data_ptr(), crows.data_ptr(),
                                 cvals.data_ptr(), int(meta.S_sel), ranges.data_ptr(), gates.data_ptr(), wptr, nb, _stream(dev))
    _lib.check(rc, "nsa_layer_decode_rows")
    kv.end_rows(t0, S)
    torch.cuda.synchronize()
    return y, ranges, gates, plan


_CASES = {}


def case(name, B, t0, S, **mod):
    """module, tokens, the cache filled to t0 by one prefill, and the S single steps on a clone of it: built once per case and never modified
    (every test works on clones of kv0)"""
    if name not in _CASES:
        m = module(**mod)
        dtype = m.W_Q.weight.dtype
        torch.manual_seed(4321)
        x = torch.randn(B, t0 + S, m.dim, device="cuda").to(dtype)
        with torch.no_grad():
            kv0 = m.new_kv(B, t0 + 16, "cuda", dtype)
            m(x[:, :t0], kv0, prefill=True)
        kv_ref = _clone_kv(kv0)
        y, r, g = single_steps(m, x[:, t0:], kv_ref)
        torch.cuda.synchronize()
        _CASES[name] = dict(m=m, x=x, xn=x[:, t0:].contiguous(), kv0=kv0, kv_ref=kv_ref, y=y, ranges=r, gates=g, B=B, t0=t0, S=S, dtype=dtype)
    return _CASES[name]


def case1():
    return case("m7c", 3, 1052, 8)


def assert_ranges_equal(got, ref):
    for s in range(ref.shape[1]):
        assert norm(got[:, s].cpu().numpy()) == norm(ref[:, s].cpu().numpy()), s


def assert_old_rows_untouched(c, kv):
    t0, kv0 = c["t0"], c["kv0"]
    for name in TOKEN_CACHES:
        assert torch.equal(getattr(kv, name)[:, :, :t0], getattr(kv0, name)[:, :, :t0]), name
    for name in ("_K_cmp", "_V_cmp"):
        assert torch.equal(getattr(kv, name)[:, :, :ncmp(t0)], getattr(kv0, name)[:, :, :ncmp(t0)]), name


def assert_y(c, y, tag):
    ref = c["y"].float()
    err, bar = (y.float() - ref).abs().max().item(), 1e-2 * max(1.0, ref.abs().max().item())
    print(f"{tag}: max|y - single steps| {err:.3e} (bar {bar:.3e})")
    assert torch.isfinite(y.float()).all() and err <= bar, (tag, err, bar)


def assert_state(c, kv):
    ref = c["kv_ref"]
    assert (kv.t, kv.n_cmp) == (ref.t, ref.n_cmp) == (c["t0"] + c["S"], ncmp(c["t0"] + c["S"]))
    for name in READS:
        assert getattr(kv, name) == getattr(ref, name), name


def assert_bit_equal_case(c, kv, y, ranges, gates, tag):
    """case 1's assertions"""
    t0, S, ref = c["t0"], c["S"], c["kv_ref"]
    for name in TOKEN_CACHES:
        assert torch.equal(getattr(kv, name)[:, :, t0:t0 + S], getattr(ref, name)[:, :, t0:t0 + S]), name
    n0, n1 = ncmp(t0), ncmp(t0 + S)
    for name in ("_K_cmp", "_V_cmp"):
        assert torch.equal(getattr(kv, name)[:, :, n0:n1], getattr(ref, name)[:, :, n0:n1]), name
    assert_old_rows_untouched(c, kv)
    assert_ranges_equal(ranges, c["ranges"])
    assert_y(c, y, tag)
    eg = (gates - c["gates"]).abs().max().item()
    print(f"{tag}: max|gates - single steps| {eg:.3e} (bar {ULP1[c['dtype']] + 1e-7:.3e})")
    assert eg <= ULP1[c["dtype"]] + 1e-7, (tag, eg)


# ---- 1 / 4 / 5: bit equality through the C ABI ------------------------------------------------------------------------------------------
def check_cabi_bit_equal(c, tag):
    kv = _clone_kv(c["kv0"])
    y, ranges, gates, plan = rows_cabi(c["m"], c["xn"], kv)
    assert plan["route"] == 1, plan  # the selected branch ran its one-launch rows form
    assert_bit_equal_case(c, kv, y, ranges, gates, tag)
    assert_state(c, kv)
    return plan


def test_bit_equality_m7c():
    c = case1()
    assert ncmp(c["t0"]) == 64 and ncmp(c["t0"] + 4) == 65  # a compressed token is emitted inside the call (t = 1055)
    plan = check_cabi_bit_equal(c, "m7c B3 S8")
    assert plan["launches"] == 6


# ---- 2. the same through the module -----------------------------------------------------------------------------------------------------
def test_module_decode_rows_m7c():
    c = case1()
    m = c["m"]
    kv = _clone_kv(c["kv0"])
    with torch.no_grad():
        y, kv2 = m.decode_rows(c["xn"], kv)
    torch.cuda.synchronize()
    assert kv2 is kv and y.shape == c["y"].shape
    assert tuple(m._last_ranges.shape) == (3, 8, 2, 16, 2) and tuple(m._last_gates.shape) == (3, 8, 2, 3)
    assert_bit_equal_case(c, kv, y, m._last_ranges, m._last_gates, "module m7c B3 S8")
    assert_state(c, kv)
    assert m.get_fallback_counters()["total_fallbacks"] == 0
    with pytest.raises(RuntimeError):  # inference only
        with torch.enable_grad():
            m.decode_rows(c["xn"].clone().requires_grad_(True), _clone_kv(c["kv0"]))
    with pytest.raises(ValueError):
        m.decode_rows(torch.zeros(3, 17, 768, device="cuda", dtype=c["dtype"]), _clone_kv(c["kv0"]))


# ---- 3. the draft-verify shape ----------------------------------------------------------------------------------------------------------
def test_draft_verify_b1():
    c = case("b1", 1, 1000, 8)
    t0, S, ref = c["t0"], c["S"], c["kv_ref"]
    assert ncmp(t0 + 7) == 61 and ncmp(t0 + 8) == 62  # a compressed token is emitted at t = 1007
    kv = _clone_kv(c["kv0"])
    y, ranges, gates, plan = rows_cabi(c["m"], c["xn"], kv)
    assert plan["route"] == 1, plan
    assert_old_rows_untouched(c, kv)
    # the single steps project on the VALU form (B < 3), the rows call on the MFMA form: the new rows agree up to the rounding of the projection
    for name, lo, hi in [(n, t0, t0 + S) for n in TOKEN_CACHES] + [(n, ncmp(t0), ncmp(t0 + S)) for n in ("_K_cmp", "_V_cmp")]:
        a, b = getattr(kv, name)[:, :, lo:hi].float(), getattr(ref, name)[:, :, lo:hi].float()
        err, bar = (a - b).abs().max().item(), 2e-2 * max(1.0, b.abs().max().item())
        print(f"B1 {name}: max|rows - single steps| {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (name, err, bar)
    # every row has t + 1 <= 1008 <= n_sel l_sel: every block is selected whatever the scores round to -- no exemption
    assert t0 + S <= 16 * 64
    assert_ranges_equal(ranges, c["ranges"])
    assert_y(c, y, "B1 S8")
    assert_state(c, kv)


# ---- 4. D = 128 -----------------------------------------------------------------------------------------------------------------------
def test_bit_equality_d128():
    check_cabi_bit_equal(case("d128", 3, 1052, 4, dim=1536, H=12, G=2, D=128), "D128 B3 S4")


# ---- 5. f16, h = 4 --------------------------------------------------------------------------------------------------------------------
def test_bit_equality_f16_h4():
    check_cabi_bit_equal(case("f16h4", 3, 1052, 5, dim=512, H=8, G=2, D=64, dtype=torch.float16), "f16 h4 B3 S5")


# ---- 6. fp32: the chunk-loop rows epilogue ----------------------------------------------------------------------------------------------
def test_fp32_chunk_loop_rows():
    c = case("fp32", 2, 300, 3, dtype=torch.float32)
    t0, S, ref = c["t0"], c["S"], c["kv_ref"]
    kv = _clone_kv(c["kv0"])
    y, ranges, gates, plan = rows_cabi(c["m"], c["xn"], kv)
    assert plan["route"] == 0, plan  # the selected branch takes its separate launches
    assert_old_rows_untouched(c, kv)
    assert_ranges_equal(ranges, c["ranges"])
    for name, lo, hi in [(n, t0, t0 + S) for n in TOKEN_CACHES] + [(n, ncmp(t0), ncmp(t0 + S)) for n in ("_K_cmp", "_V_cmp")]:
        err = (getattr(kv, name)[:, :, lo:hi] - getattr(ref, name)[:, :, lo:hi]).abs().max().item() if hi > lo else 0.0
        print(f"fp32 {name}: max|rows - single steps| {err:.3e}")
        assert err <= 1e-3, (name, err)
    err = (y - c["y"]).abs().max().item()
    print(f"fp32 y: max|rows - single steps| {err:.3e}")
    assert torch.isfinite(y).all() and err <= 1e-3, err
    assert_state(c, kv)


# ---- 7. causality -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 4])
def test_causality(s):
    c = case1()
    m, t0 = c["m"], c["t0"]
    ka, kb = _clone_kv(c["kv0"]), _clone_kv(c["kv0"])
    with torch.no_grad():
        ya, _ = m.decode_rows(c["xn"], ka)
        ra = m._last_ranges.clone()
        x2 = c["xn"].clone()
        torch.manual_seed(99 + s)
        x2[:, s + 1:] = torch.randn_like(x2[:, s + 1:]) * 1.5
        yb, _ = m.decode_rows(x2, kb)
        rb = m._last_ranges.clone()
    torch.cuda.synchronize()
    assert not torch.equal(ya[:, s + 1:], yb[:, s + 1:])  # the later rows did change
    assert torch.equal(ya[:, :s + 1], yb[:, :s + 1])
    assert torch.equal(ra[:, :s + 1], rb[:, :s + 1])
    for name in TOKEN_CACHES:
        assert torch.equal(getattr(ka, name)[:, :, :t0 + s + 1], getattr(kb, name)[:, :, :t0 + s + 1]), name
    for name in ("_K_cmp", "_V_cmp"):
        assert torch.equal(getattr(ka, name)[:, :, :ncmp(t0 + s + 1)], getattr(kb, name)[:, :, :ncmp(t0 + s + 1)]), name


# ---- 8. truncate ------------------------------------------------------------------------------------------------------------------------
def test_truncate_after_rejected_drafts():
    c = case1()
    m, t0 = c["m"], c["t0"]
    torch.manual_seed(77)
    xb = torch.randn(3, 5, 768, device="cuda").to(c["dtype"])
    ka, kb = _clone_kv(c["kv0"]), _clone_kv(c["kv0"])
    with torch.no_grad():
        m.decode_rows(c["xn"], ka)          # 8 draft tokens ...
        ka.truncate(t0 + 3)                 # ... 3 accepted (the pooled token of t = 1055 is forgotten with the rest)
        assert (ka.t, ka.n_cmp) == (t0 + 3, 64)
        ya, ra, _ = single_steps(m, xb, ka)
        single_steps(m, c["xn"][:, :3], kb)
        yb, rb, _ = single_steps(m, xb, kb)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb) and torch.equal(ra, rb)
    assert (ka.t, ka.n_cmp) == (kb.t, kb.n_cmp) == (t0 + 8, 65)
    for name in TOKEN_CACHES:
        assert torch.equal(getattr(ka, name)[:, :, :ka.t], getattr(kb, name)[:, :, :kb.t]), name
    for name in ("_K_cmp", "_V_cmp"):
        assert torch.equal(getattr(ka, name)[:, :, :65], getattr(kb, name)[:, :, :65]), name
    for name in READS:
        assert getattr(ka, name) == getattr(kb, name) and len(getattr(ka, name)) == 8, name


# ---- 9. declined routes -----------------------------------------------------------------------------------------------------------------
def check_declined(c, m):
    ka, kb = _clone_kv(c["kv0"]), _clone_kv(c["kv0"])
    with torch.no_grad():
        ya, _ = m.decode_rows(c["xn"], ka)
        ra, ga = m._last_ranges, m._last_gates
    yb, rb, gb = single_steps(m, c["xn"], kb)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb) and torch.equal(ra, rb) and torch.equal(ga, gb)
    assert tuple(ra.shape) == (3, 8, 2, 16, 2) and tuple(ga.shape) == (3, 8, 2, 3)
    assert (ka.t, ka.n_cmp) == (kb.t, kb.n_cmp) == (c["t0"] + 8, 65)
    for name in TOKEN_CACHES:
        assert torch.equal(getattr(ka, name)[:, :, :ka.t], getattr(kb, name)[:, :, :kb.t]), name
    for name in ("_K_cmp", "_V_cmp"):
        assert torch.equal(getattr(ka, name)[:, :, :65], getattr(kb, name)[:, :, :65]), name
    for name in READS:
        assert getattr(ka, name) == getattr(kb, name), name


def test_declined_by_the_plan_switch(tune):
    c = case1()
    tune("LAYER_DECODE_ROWS", 0)
    check_declined(c, c["m"])


def test_declined_in_parity_mode(monkeypatch):
    c = case1()
    monkeypatch.setenv("NSA_FORCE_PARITY", "1")
    mp = module()  # the flag is read at construction; same seed, same weights
    assert mp._force_parity and torch.equal(mp.W_Q.weight, c["m"].W_Q.weight)
    check_declined(c, mp)


# ---- 10. run to run ---------------------------------------------------------------------------------------------------------------------
def test_run_to_run():
    c = case1()
    out = []
    for _ in range(2):
        kv = _clone_kv(c["kv0"])
        y, ranges, gates, _ = rows_cabi(c["m"], c["xn"], kv)
        out.append((y, ranges, gates, kv))
    (ya, ra, ga, ka), (yb, rb, gb, kb) = out
    assert torch.equal(ya, yb) and torch.equal(ra, rb) and torch.equal(ga, gb)
    for name in TOKEN_CACHES:
        assert torch.equal(getattr(ka, name)[:, :, :ka.t], getattr(kb, name)[:, :, :kb.t]), name
    for name in ("_K_cmp", "_V_cmp"):
        assert torch.equal(getattr(ka, name)[:, :, :ka.n_cmp], getattr(kb, name)[:, :, :kb.n_cmp]), name
