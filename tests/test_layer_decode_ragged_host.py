"""Host side of the layer's ragged call (no GPU): nsa_layer_decode_ragged, its workspace and plan queries, NSA_KV.sequence_view and
NSAAttention.decode_ragged.

The workspace and plan queries make no HIP call, and a refused call returns before its first one.  `dispatch_check <library> layer_ragged`
(csrc/dispatch_check.cpp: the library's host code against a HIP runtime that counts and refuses every launch) walks the call's route on
real pointers; this file asserts it: six launchers in order, the pooling grid, the position pointer and te in the argument blocks of the
four launches that depend on the position, no memset.  The default output of dispatch_check is what tests/test_dispatch_host.py compares
with its recorded file: these cases are not in it."""
import ctypes
import json
import os
import subprocess

import pytest
import torch

from conftest import ROOT
from test_layer_decode_rows_host import BF16, F32, STANDIN, cache, layer

INVALID = -1  # NSA_ERR_INVALID


def plan(d, B, S, t_max, S_max=2048, S_sel=None):
    from nsa_vibe_amd import _lib

    n, r = ctypes.c_int(-7), ctypes.c_int(-7)
    te = min(t_max, S_max - 1)
    S_sel = -(-(te + 1) // 64) if S_sel is None else S_sel
    rc = _lib.lib().nsa_layer_decode_ragged_plan(ctypes.byref(d) if d is not None else None, B, S, S_max, t_max, S_sel, ctypes.byref(n), ctypes.byref(r))
    return rc, n.value, r.value


def test_workspace_query():
    from nsa_vibe_amd import _lib

    L, d = _lib.lib(), layer()
    ref = ctypes.byref(d)
    assert L.nsa_layer_decode_ragged_workspace(None, 3, 8, 2048) == 0
    assert L.nsa_layer_decode_ragged_workspace(ref, 0, 8, 2048) == 0
    assert L.nsa_layer_decode_ragged_workspace(ref, 3, 0, 2048) == 0
    assert L.nsa_layer_decode_ragged_workspace(ref, 3, 17, 2048) == 0
    for B, S in ((1, 1), (3, 8), (16, 16), (64, 4)):
        need = L.nsa_layer_decode_ragged_workspace(ref, B, S, 2048)
        assert need > 0 and need >= L.nsa_layer_decode_rows_workspace(ref, B, S, 2048)
    d128 = layer(D=128, dim=1536)
    assert L.nsa_layer_decode_ragged_workspace(ctypes.byref(d128), 3, 4, 2048) >= L.nsa_layer_decode_rows_workspace(ctypes.byref(d128), 3, 4, 2048) > 0


def test_plan_counts_six_launches_always():
    d = layer()
    assert plan(d, 3, 8, 1059) == (0, 6, 1)   # projection, pooling, rows step, band pair, finish, output
    assert plan(d, 3, 8, 1063) == (0, 6, 1)   # no compressed token due anywhere: the pooling launch is counted all the same
    assert plan(d, 16, 1, 1059) == (0, 6, 1)  # S = 1 runs as six launches here (no riding form)
    assert plan(d, 3, 8, 5000) == (0, 6, 1)   # t_max beyond the capacity: te = S_max - 1
    rc, n, r = plan(layer(D=128, dim=1536), 3, 4, 1059)  # D = 128: one ragged launch per band branch, the gate kernel for the finish
    assert (rc, n, r) == (0, 7, 1)


def test_plan_declines_without_a_scalar_route(tune):
    assert plan(layer(F32), 3, 8, 1059) == (0, 0, -1)
    assert plan(layer(), 3, 8, 70000, S_max=131072) == (0, 0, -1)
    assert plan(layer(D=128, dim=1536), 3, 4, 20000, S_max=32768) == (0, 0, -1)
    odd = layer()
    odd.l_sel = 128
    assert plan(odd, 3, 8, 1059, S_sel=17) == (0, 0, -1)
    tune("DECODE_UNFUSED", 1)
    assert plan(layer(), 3, 8, 1059) == (0, 0, -1)


def test_plan_refuses_bad_arguments():
    d = layer()
    for args, kw in [((3, 17, 1059), {}), ((3, 0, 1059), {}), ((0, 8, 1059), {}), ((3, 8, -1), {}), ((3, 8, 1059), {"S_sel": 16}), ((3, 8, 5000), {"S_sel": 31})]:
        rc, n, r = plan(d, *args, **kw)
        assert rc != 0 and (n, r) == (0, -1), (args, kw)
    rc, n, r = plan(None, 3, 8, 1059)
    assert rc != 0 and (n, r) == (0, -1)


def test_refusals_come_before_any_device_call(tune):
    from nsa_vibe_amd import _lib

    L = _lib.lib()

    def call(d=None, k=None, x=STANDIN, y=STANDIN, t_pos=STANDIN, t_max=1059, S=8, S_sel=17, null_desc=False, null_kv=False):
        d = layer() if d is None else d
        k = cache() if k is None else k
        rc = L.nsa_layer_decode_ragged(None if null_desc else ctypes.byref(d), None if null_kv else ctypes.byref(k), x, y, t_pos, t_max, S, None, None, None,
                                       S_sel, None, None, None, 0, None)
        return rc, _lib.last_error()

    def refused(what, **kw):
        rc, err = call(**kw)
        assert rc == INVALID and what in err, (kw, rc, err)

    refused("null pointer", x=None)
    refused("null pointer", y=None)
    refused("null cache pointer", null_kv=True)
    refused("null layer descriptor", null_desc=True)
    refused("null position array", t_pos=None)
    refused("t_pos must be 4-byte aligned", t_pos=STANDIN + 2)
    refused("tokens per sequence", S=17)
    refused("tokens per sequence", S=0)
    refused("must not be negative", t_max=-1)
    refused("does not cover", S_sel=16)
    small = cache()
    small.n_cmp_max = 60
    refused("compressed cache too small", k=small)
    # every declined shape names its limit (there is no scalar route to stand in)
    refused("bf16 / f16 only", d=layer(F32))
    refused("more than 64 chunks", k=cache(S_max=131072), t_max=70000, S_sel=1094)
    refused("more than 16 chunks", d=layer(D=128, dim=1536), k=cache(S_max=32768), t_max=20000, S=4, S_sel=313)
    odd = layer()
    odd.l_sel = 128
    refused("default block geometry", d=odd)
    off = cache()
    off.K_sel = STANDIN + 2
    refused("16-byte aligned", k=off)
    tune("DECODE_UNFUSED", 1)
    refused("DECODE_UNFUSED = 1")
    tune("DECODE_UNFUSED", -1)
    refused("workspace")  # everything else in order: the missing workspace is what is left to refuse


@pytest.fixture(scope="module")
def routes():
    from nsa_vibe_amd import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    r = subprocess.run([os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH, "layer_ragged"], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_only_the_layer_ragged_cases(routes):
    assert routes and all(k.startswith("layer_decode_ragged/") for k in routes)


SIX = ["qkv_rope_append(rows, mfma) launch", "cmp_pool(ragged) launch", "decode_rows launch", "band_attn_fwd_dual launch", "decode_finish launch",
       "linear_small(mfma) launch"]


@pytest.mark.parametrize("case,B,S,te", [("m7c_B3_S8", 3, 8, 1059), ("m7c_B3_S8_no_token_due", 3, 8, 1063), ("m7c_B16_S1", 16, 1, 1059),
                                         ("t_max_beyond_capacity", 3, 8, 1071)])
def test_six_launches_carry_the_positions(routes, case, B, S, te):
    c = routes["layer_decode_ragged/" + case]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"] == SIX
    G, d = 2, 16
    assert c["geometry"][1].split("/")[:2] == [f"{B * G * -(-S // d)},1,1", "256,1,1"]   # pooling: B G ceil(S / d) blocks of the wide form
    assert c["geometry"][2].split("/")[0] == f"{B * S * G},1,1"                           # the selected branch: one workgroup per row
    assert routes["layer_decode_ragged/" + case + "_plan"]["launches"] == 6 and routes["layer_decode_ragged/" + case + "_plan"]["route"] == 1
    by_launch = {a["launch"]: a for a in c["args"]}
    assert sorted(by_launch) == [0, 1, 2, 3]
    rope, pool, step, band = by_launch[0]["rope"], by_launch[1]["pool"], by_launch[2]["step"], by_launch[3]
    for blk in (rope, pool, step, band["band_w"], band["band_c"]):
        assert blk["t_pos"] == "t_pos+20" and blk["t_max"] == te, blk  # the pointer as given (five int32 into the buffer) and te
    assert (rope["t0"], rope["B"], rope["S"], rope["S_max"]) == (0, B, S, 1072) and rope["Q_out"].startswith("ws+")
    assert (pool["S"], pool["G"], pool["nbg"], pool["n_cmp_max"]) == (S, G, B * G, 66)
    ncmp = (te + 1 - 32) // 16 + 1
    assert (step["S"], step["R"], step["S_cmp"]) == (S, B * S * G, ncmp)
    assert (band["band_w"]["K"], band["band_w"]["S_kv"], band["band_w"]["defer_combine"]) == ("K_win+0", te + 1, 1)
    assert (band["band_c"]["K"], band["band_c"]["S_kv"], band["band_c"]["defer_combine"]) == ("K_cmp+0", ncmp, 1)
    assert band["band_w"]["nsplit"] == band["band_c"]["nsplit"] > 1


def test_a_bound_below_the_rows_is_planned_from_position_zero(routes):
    """t_max < S - 1: no sequence can be live (the call gives zero rows); the launches are planned for te + 1 = 4 tokens, not from a negative
    position"""
    c = routes["layer_decode_ragged/t_max_below_S"]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"][:3] == SIX[:3] and c["launches"][-2:] == SIX[-2:]
    by = {a["launch"]: a for a in c["args"]}
    assert (by[0]["rope"]["t0"], by[0]["rope"]["t_max"], by[1]["pool"]["t_max"]) == (0, 3, 3)
    assert (by[2]["step"]["t_max"], by[2]["step"]["S_cmp"], by[2]["step"]["nchunk"]) == (3, 0, 0)
    bands = [a["band"] for a in c["args"] if "band" in a]
    assert all(b["t_max"] == 3 and b["t0"] == 0 and b["S_kv"] == 4 for b in bands)  # (the compressed branch has no token: its generic launch)
    assert routes["layer_decode_ragged/t_max_below_S_plan"]["rc"] == 0 and routes["layer_decode_ragged/t_max_below_S_plan"]["route"] == 1


def test_few_rows_project_on_the_chunk_loop(routes):
    c = routes["layer_decode_ragged/m7c_B1_S2_chunk_loop"]
    assert (c["rc"], c["memsets"]) == (0, 0)
    assert c["launches"] == ["qkv_rope_append(rows) launch"] + SIX[1:5] + ["linear_small(fast) launch"]
    rope = c["args"][0]["rope"]
    assert (rope["t_pos"], rope["t_max"], rope["t0"]) == ("t_pos+20", 1059, 0)


def test_d128_launches_the_band_branches_one_each(routes):
    c = routes["layer_decode_ragged/D128_B3_S4"]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"] == ["qkv_rope_append(rows, mfma) launch", "cmp_pool(ragged) launch", "decode_rows launch", "band_attn_fwd(split) launch",
                             "band_attn_combine launch", "band_attn_fwd(split) launch", "band_attn_combine launch", "gate_combine launch",
                             "linear_small(mfma) launch"]
    bands = [a["band"] for a in c["args"] if "band" in a]
    assert [b["K"] for b in bands] == ["K_win+0", "K_cmp+0"]
    assert all(b["t_pos"] == "t_pos+20" and b["t_max"] == 1059 and b["defer_combine"] == 0 for b in bands)
    assert routes["layer_decode_ragged/D128_B3_S4_plan"]["launches"] == 7  # (an undeferred split branch's combine is not counted, as in the rows plan)


@pytest.mark.parametrize("case,what", [("f32_declined", "bf16 / f16 only"), ("t_max70000_declined", "more than 64 chunks"),
                                       ("D128_t_max20000_declined", "more than 16 chunks"), ("S17_refused", "tokens per sequence"),
                                       ("null_t_pos", "null position array"), ("t_pos_2_bytes_off", "4-byte aligned"), ("no_workspace", "workspace"),
                                       ("DECODE_UNFUSED_1_declined", "DECODE_UNFUSED = 1")])
def test_refused_calls_launch_nothing(routes, case, what):
    c = routes["layer_decode_ragged/" + case]
    assert c["rc"] == INVALID and what in c["error"], c
    assert c["launches"] == [] and c["geometry"] == [] and c["memsets"] == 0


# ---- Python on CPU tensors ---------------------------------------------------------------------------------------------------------------
def _pool(B=3, cap=128):
    from nsa_vibe_amd.kv_cache import NSA_KV

    kv = NSA_KV(B, 2, 64, 64, cap, 32, 16, 64, 16, 512, "cpu", torch.float32)
    for name in ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp"):
        getattr(kv, name).zero_()
    return kv


def test_sequence_view_shares_storage():
    kv = _pool()
    kv.t, kv.n_cmp = 5, 0
    kv.append_reads(0, 5)
    v = kv.sequence_view(1, 70)
    assert (v.B, v.t, v.n_cmp, v.auto_grow, v.S_max) == (1, 70, 3, False, 128)
    assert v.reads_pred == [] and v._native == {} and v._native is not kv._native
    assert v._K_sel.shape == (1, 2, 128, 64) and v._K_cmp.shape[0] == 1 and v.K_sel.shape[2] == 70 and v.K_cmp.shape[2] == 3
    for name in ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp"):
        assert getattr(v, name).data_ptr() == getattr(kv, name)[1].data_ptr(), name
    one = torch.ones(1, 2, 1, 64)
    v.write_tokens(one, 2 * one, 3 * one, 4 * one, 5 * one, 6 * one)  # a write through the view is seen in the pool, in slab 1 alone
    assert v.t == 71 and torch.equal(kv._K_sel[1, :, 70], one[0, :, 0]) and torch.equal(kv._V_raw[1, :, 70], 6 * one[0, :, 0])
    assert kv._K_sel[0].abs().sum() == 0 and kv._K_sel[2].abs().sum() == 0
    assert (kv.t, kv.n_cmp, kv.reads_pred) == (5, 0, [kv.reads_pred[0]])  # the pool's own bookkeeping is not the view's
    with pytest.raises(RuntimeError):
        v.ensure_capacity(129)  # a view does not grow
    assert kv.sequence_view(0).t == 0
    for bad in (-1, 3):
        with pytest.raises(IndexError):
            kv.sequence_view(bad)
    with pytest.raises(ValueError):
        kv.sequence_view(0, 129)


def test_decode_ragged_refuses_before_any_native_call(monkeypatch):
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.nsa_attention import NSAAttention

    m = NSAAttention(768, 12, 2, 64, 64, l=32, d=16, l_sel=64, n_sel=16, w=512, selector="sequential").eval()
    kv = _pool()

    def no_native():
        raise AssertionError("a native call was made")

    monkeypatch.setattr(_lib, "lib", no_native)
    x = torch.zeros(3, 4, 768)
    pos = torch.tensor([10, 20, -1], dtype=torch.int32)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="HIP device tensors"):
            m.decode_ragged(x, kv, pos, t_max=30)          # CPU tensors
        with pytest.raises(RuntimeError, match="HIP device tensors"):
            m.decode_ragged(x, kv, [10, 20, -1])
        with pytest.raises(ValueError, match="int32"):
            m.decode_ragged(x, kv, pos.long(), t_max=30)   # wrong dtype
        with pytest.raises(ValueError, match="int32"):
            m.decode_ragged(x, kv, pos[:2], t_max=30)      # wrong length
        with pytest.raises(ValueError, match="positions for a batch"):
            m.decode_ragged(x, kv, [10, 20])
        with pytest.raises(ValueError, match="t_max"):
            m.decode_ragged(x, kv, pos)                    # a tensor of positions without t_max
        with pytest.raises(RuntimeError, match="reserve"):
            m.decode_ragged(x, kv, pos, t_max=128)         # t_max + 1 beyond the capacity: not grown
        with pytest.raises(RuntimeError, match="reserve"):
            m.decode_ragged(x, kv, [10, 125, -1])          # ... derived from host positions too
        with pytest.raises(ValueError, match="1 to 16"):
            m.decode_ragged(torch.zeros(3, 17, 768), kv, pos, t_max=30)
    assert (kv.t, kv.n_cmp) == (0, 0)
