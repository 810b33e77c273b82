"""Host side of nsa_layer_decode_rows (no GPU: the workspace and plan queries make no HIP call, a refused call returns before its first one):
the workspace sizes, the plan's launch count and route with its LAYER_DECODE_ROWS switch, the argument checks, and NSA_KV.truncate."""
import ctypes

import pytest
import torch

from nsa_vibe_amd import _lib
from nsa_vibe_amd.kv_cache import NSA_KV

BF16, F32 = _lib.NSA_DT_BF16, _lib.NSA_DT_F32
STANDIN = 256  # an aligned value in a pointer's place: nothing on these paths dereferences it


def layer(dt=BF16, dim=768, G=2, h=6, D=64):
    d = _lib.NsaLayerDesc()
    d.dim, d.G, d.h, d.Dk, d.Dv = dim, G, h, D, D
    d.l, d.d, d.l_sel, d.n_sel, d.w = 32, 16, 64, 16, 512
    d.gate_hidden, d.dtype = 32, dt
    d.rope_base, d.rope_scale, d.gate_tau = 10000.0, 1.0, 1.0
    d.W_qkv = d.W_out = d.gate_w1 = d.gate_b1 = d.gate_w2 = d.gate_b2 = STANDIN
    return d


def cache(B=3, S_max=2048):
    k = _lib.NsaKvDesc()
    k.K_sel = k.V_sel = k.K_win = k.V_win = k.K_raw = k.V_raw = k.K_cmp = k.V_cmp = STANDIN
    k.B, k.S_max, k.n_cmp_max = B, S_max, (S_max - 32) // 16 + 1
    return k


def plan(d, B, S, t0, S_max=2048, S_sel=None):
    n, r = ctypes.c_int(-7), ctypes.c_int(-7)
    S_sel = -(-(t0 + S) // 64) if S_sel is None else S_sel
    rc = _lib.lib().nsa_layer_decode_rows_plan(ctypes.byref(d), B, S, S_max, t0, S_sel, ctypes.byref(n), ctypes.byref(r))
    return rc, n.value, r.value


def test_workspace_query():
    L, d = _lib.lib(), layer()
    ref = ctypes.byref(d)
    assert L.nsa_layer_decode_rows_workspace(None, 3, 8, 2048) == 0
    assert L.nsa_layer_decode_rows_workspace(ref, 0, 8, 2048) == 0
    assert L.nsa_layer_decode_rows_workspace(ref, 3, 0, 2048) == 0
    assert L.nsa_layer_decode_rows_workspace(ref, 3, 17, 2048) == 0
    for B in (1, 3, 16):
        one = L.nsa_layer_decode_rows_workspace(ref, B, 1, 2048)
        assert one > 0 and one >= L.nsa_layer_decode_step_workspace(ref, B, 2048)
        assert L.nsa_layer_decode_rows_workspace(ref, B, 16, 2048) >= one
    # every row has its projection, Q, four branch / mix buffers, ranges and gates
    NQ, NT = 2 * 6 * 64, 2 * 6 * 64 + 6 * 2 * 64
    assert L.nsa_layer_decode_rows_workspace(ref, 3, 8, 2048) >= 24 * (2 * NT + 2 * 5 * NQ + 4 * 2 * 16 * 2 + 4 * 2 * 3)


def test_plan_counts_launches_without_a_device():
    d = layer()
    assert plan(d, 3, 8, 1052) == (0, 6, 1)   # n_cmp 64 -> 65 inside the call: projection, pooling, rows step, band pair, finish, output
    assert plan(d, 3, 4, 1056) == (0, 5, 1)   # no compressed token due
    assert plan(d, 1, 8, 1000) == (0, 6, 1)
    rc, n, r = plan(layer(F32), 2, 3, 300)    # fp32: the selected branch on its separate launches, a launch per band branch
    assert rc == 0 and r == 0 and n > 6
    rc, n, r = plan(layer(D=128, dim=1536), 3, 4, 1052)  # D = 128: the rows form holds, the band branches are launched one each
    assert rc == 0 and r == 1 and n == 7
    rc, n, r = plan(d, 2, 4, 10)              # no compressed token yet: the rows form declines, the call still runs
    assert rc == 0 and r == 0 and n > 5
    for args, kw in [((3, 17, 1052), {}), ((3, 0, 1052), {}), ((0, 8, 1052), {}), ((3, 8, 2041), {}), ((3, 8, 1052), {"S_sel": 16})]:
        rc, n, r = plan(d, *args, **kw)
        assert rc != 0 and (n, r) == (0, -1), (args, kw)
    assert _lib.lib().nsa_layer_decode_rows_plan(None, 3, 8, 2048, 1052, 17, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) != 0


def test_plan_follows_the_switch(tune):
    d = layer()
    assert plan(d, 3, 8, 1052)[2] == 1 and plan(d, 1, 2, 1052)[2] == 1
    assert plan(d, 3, 1, 1052) == (0, 0, -1)  # the default rule: one token stays with the single step
    tune("LAYER_DECODE_ROWS", 0)
    assert plan(d, 3, 8, 1052) == (0, 0, -1)
    tune("LAYER_DECODE_ROWS", 1)
    assert plan(d, 3, 8, 1052) == (0, 6, 1)
    rc, n, r = plan(d, 3, 1, 1052)
    assert rc == 0 and r == 1 and n >= 4
    tune("DECODE_ROWS", 0)                    # the selected branch's own switch moves the route, not the decision
    rc, n, r = plan(d, 3, 8, 1052)
    assert rc == 0 and r == 0 and n > 6


def test_refusals_come_before_any_device_call():
    L, d, k = _lib.lib(), layer(), cache()
    dref, kref = ctypes.byref(d), ctypes.byref(k)

    def call(x=STANDIN, y=STANDIN, t0=1052, S=8, S_sel=17, kv=kref, desc=dref):
        return L.nsa_layer_decode_rows(desc, kv, x, y, t0, S, None, None, None, S_sel, None, None, None, 0, None)

    assert call(x=None) != 0 and "null pointer" in _lib.last_error()
    assert call(y=None) != 0 and "null pointer" in _lib.last_error()
    assert call(kv=None) != 0 and "null cache pointer" in _lib.last_error()
    assert call(desc=None) != 0 and "null layer descriptor" in _lib.last_error()
    assert call(t0=2041) != 0 and "exceed the cache capacity" in _lib.last_error()
    assert call(S=17) != 0 and "tokens per sequence" in _lib.last_error()
    assert call(S=0) != 0 and "tokens per sequence" in _lib.last_error()
    assert call(S_sel=16) != 0 and "does not cover" in _lib.last_error()
    assert call() != 0 and "workspace" in _lib.last_error()  # everything else in order: the missing workspace is what is left to refuse


def _kv(t, decoded):
    kv = NSA_KV(1, 2, 64, 64, 128, 32, 16, 64, 16, 512, "cpu", torch.float32)
    kv.t, kv.n_cmp = t, 0 if t < 32 else (t - 32) // 16 + 1
    for s in range(t - decoded, t):
        kv.append_reads(0 if s + 1 < 32 else (s + 1 - 32) // 16 + 1, s + 1)
    return kv


def test_truncate():
    kv = _kv(100, 100)  # every token decoded: one entry per token
    ptr = kv._K_sel.data_ptr()
    full = list(kv.reads_act_cmp)
    kv.truncate(70)
    assert (kv.t, kv.n_cmp) == (70, 3)
    for name in ("reads_pred", "reads_act_total", "reads_act_sel", "reads_act_cmp", "reads_act_win"):
        assert len(getattr(kv, name)) == 70, name
    assert kv.reads_act_cmp == full[:70] and kv._K_sel.data_ptr() == ptr and kv.K_sel.shape[2] == 70 and kv.K_cmp.shape[2] == 3
    kv.truncate(70)     # nothing to forget
    assert (kv.t, kv.n_cmp, len(kv.reads_pred)) == (70, 3, 70)
    kv.truncate(31)
    assert (kv.t, kv.n_cmp, len(kv.reads_pred)) == (31, 0, 31)
    kv.truncate(0)
    assert (kv.t, kv.n_cmp, kv.reads_pred) == (0, 0, [])
    kv = _kv(100, 40)   # 60 tokens by a prefill (no counters), 40 decoded: the counters of the forgotten decode steps go
    kept = list(kv.reads_act_win[:10])
    kv.truncate(70)
    assert (kv.t, kv.n_cmp, len(kv.reads_pred)) == (70, 3, 10) and kv.reads_act_win == kept
    kv.truncate(50)     # into the prefill: no counter is left
    assert (kv.t, kv.n_cmp, kv.reads_pred) == (50, 2, [])


def test_truncate_refuses_what_is_not_cached():
    kv = _kv(100, 0)
    for t in (101, -1):
        with pytest.raises(ValueError):
            kv.truncate(t)
    assert (kv.t, kv.n_cmp) == (100, 5)
