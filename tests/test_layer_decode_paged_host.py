"""Host side of the layer's paged call (no GPU): nsa_layer_decode_paged, its workspace and plan queries.

`dispatch_check <library> layer_paged` (csrc/dispatch_check.cpp: the library's host code against a HIP runtime that counts and refuses every
launch) walks the call's route on real pointers; this file asserts it: the launchers in order and their count against the plan, both
writers' argument blocks as given (the pools, the capacities, the table block), the position array of every launch behind the pre-pass --
the workspace's t_live, never the caller's t_pos --, no memset, and every decline with its message and no launch.  The default output of
dispatch_check is what tests/test_dispatch_host.py compares with its recorded file: these cases are not in it."""
import ctypes
import json
import os
import subprocess

import pytest

from conftest import ROOT
from test_layer_decode_rows_host import F32, layer

INVALID = -1  # NSA_ERR_INVALID


@pytest.fixture(scope="module")
def routes():
    from nsa_vibe_amd import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    r = subprocess.run([os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH, "layer_paged"], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_only_the_layer_paged_cases(routes):
    assert routes and all(k.startswith("layer_decode_paged/") for k in routes)


BAND = ["band_attn_fwd(split) launch", "band_attn_combine launch"]
TEN = ["paged_live launch", "qkv_rope_append(paged, mfma) launch", "cmp_pool(paged) launch", "decode_paged launch"] + BAND + BAND + \
      ["decode_finish launch", "linear_small(mfma) launch"]
POOLS = ("K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw")


def table_block(max_pages, stride=None):
    return {"table": "table+28", "stride": max_pages + 3 if stride is None else stride, "n_pages": 7, "max_pages": max_pages}


@pytest.mark.parametrize("case,B,S,D,max_pages,te,stride", [("m7c_B3_S8", 3, 8, 64, 2, 1059, None), ("m7c_B16_S1", 16, 1, 64, 2, 1059, None),
                                                             ("D128_B3_S4", 3, 4, 128, 2, 1059, None), ("t_max_beyond_capacity", 3, 8, 64, 2, 2047, None),
                                                             ("max_pages_2pow20", 3, 8, 64, 1 << 20, 1059, 1 << 20)])
def test_launches_blocks_and_positions(routes, case, B, S, D, max_pages, te, stride):
    c = routes["layer_decode_paged/" + case]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"] == (TEN if D == 64 else TEN[:8] + ["gate_combine launch", TEN[9]])
    p = routes["layer_decode_paged/" + case + "_plan"]
    assert (p["rc"], p["launches"], p["route"]) == (0, len(c["launches"]), 1) and p["workspace"] > 0
    G, d = 2, 16
    assert c["geometry"][0].split("/")[:2] == [f"{-(-B // 4)},1,1", "256,1,1"]               # the pre-pass: one wave per sequence
    assert c["geometry"][2].split("/")[:2] == [f"{B * G * -(-S // d)},1,1", "256,1,1"]        # pooling: B G ceil(S / d) blocks of the wide form
    assert c["geometry"][3].split("/")[0] == f"{B * S * G},1,1"                                # the selected branch: one workgroup per row
    by = {a["launch"]: a for a in c["args"]}
    assert sorted(by) == [0, 1, 2, 3, 4, 6]
    live, rope, pool, step = by[0]["live"], by[1]["rope"], by[2]["pool"], by[3]["step"]
    pg = table_block(max_pages, stride)
    cap = max_pages * 1024
    # the pre-pass reads the caller's positions and writes the verdicts into the workspace
    assert (live["t_pos"], live["pg"], live["B"], live["S"], live["te"]) == ("t_pos+20", pg, B, S, te)
    t_live = live["t_live"]
    assert t_live.startswith("ws+") and int(t_live[3:]) % 256 == 0 and int(t_live[3:]) + 4 * B <= p["workspace"]
    # both writers' blocks as given
    assert [rope[k] for k in POOLS] == [k + "+0" for k in POOLS] and rope["proj"] == "ws+0" and rope["Q_out"].startswith("ws+")
    assert (rope["B"], rope["S"], rope["G"], rope["h"], rope["Dk"], rope["Dv"], rope["S_max"], rope["t0"]) == (B, S, G, 6, D, D, cap, 0)
    assert (rope["rope_base"], rope["inv_scale"], rope["pg"]) == (10000, 1, pg)
    assert (pool["K_raw"], pool["V_raw"], pool["K_cmp"], pool["V_cmp"]) == ("K_raw+0", "V_raw+0", "K_cmp+0", "V_cmp+0")
    assert (pool["nbg"], pool["S_max"], pool["n_cmp_max"], pool["Dk"], pool["Dv"], pool["l"], pool["d"]) == (B * G, cap, max_pages * 64, D, D, 32, 16)
    assert (pool["rope_base"], pool["inv_scale"], pool["S"], pool["G"], pool["pg"]) == (10000, 1, S, G, pg)
    # the readers: the pools with their page strides, the table, and the same verdicts
    ncmp = (te + 1 - 32) // 16 + 1
    assert (step["S"], step["R"], step["S_cmp"], step["Kc"], step["csb"]) == (S, B * S * G, ncmp, "K_cmp+0", G * 64 * D)
    assert (step["table"], step["table_stride"], step["n_pages"]) == (pg["table"], pg["stride"], 7)
    w, cm = by[4], by[6]
    assert (w["band"]["K"], w["band"]["V"], w["band"]["ksb"], w["band"]["ksg"], w["band"]["S_kv"]) == ("K_win+0", "V_win+0", G * 1024 * D, 1024 * D, cap)
    assert (w["band"]["a"], w["band"]["dd"], w["band"]["w"], w["band_table"]["shift"]) == (0, 1, 512, 10)
    assert (cm["band"]["K"], cm["band"]["V"], cm["band"]["ksb"], cm["band"]["ksg"], cm["band"]["S_kv"]) == ("K_cmp+0", "V_cmp+0", G * 64 * D, 64 * D, max_pages * 64)
    assert (cm["band"]["a"], cm["band"]["dd"], cm["band_table"]["shift"]) == (32, 16, 6)
    for blk in (w, cm):
        assert (blk["band_table"]["table"], blk["band_table"]["stride"], blk["band_table"]["n_pages"]) == (pg["table"], pg["stride"], 7)
        assert blk["band"]["nsplit"] > 1 and blk["band"]["defer_combine"] == 0  # each branch combines its own splits: O is final for the finish
    # every launch behind the pre-pass takes the workspace's t_live as its position array, and the bound te
    for blk in (rope, pool, step, w["band"], cm["band"]):
        assert blk["t_pos"] == t_live and blk["t_max"] == te, blk


def test_few_rows_project_on_the_chunk_loop(routes):
    c = routes["layer_decode_paged/m7c_B1_S2_chunk_loop"]
    assert (c["rc"], c["memsets"]) == (0, 0)
    assert c["launches"] == [TEN[0], "qkv_rope_append(paged) launch"] + TEN[2:9] + ["linear_small(fast) launch"]
    by = {a["launch"]: a for a in c["args"]}
    rope = by[1]["rope"]
    assert rope["t_pos"] == by[0]["live"]["t_live"] and (rope["t_max"], rope["t0"], rope["S_max"], rope["pg"]) == (1059, 0, 2048, table_block(2))
    assert routes["layer_decode_paged/m7c_B1_S2_chunk_loop_plan"]["launches"] == 10


def test_many_rows_run_the_bands_unsplit(routes):
    c = routes["layer_decode_paged/m7c_B600_S3_unsplit_bands"]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"] == TEN[:4] + ["band_attn_fwd launch", "band_attn_fwd launch"] + TEN[8:]
    assert routes["layer_decode_paged/m7c_B600_S3_unsplit_bands_plan"]["launches"] == 8
    t_live = c["args"][0]["live"]["t_live"]
    assert all(a[k]["t_pos"] == t_live for a in c["args"][1:] for k in ("rope", "pool", "step", "band") if k in a)


def test_a_bound_below_the_rows_is_planned_from_position_zero(routes):
    c = routes["layer_decode_paged/t_max_below_S"]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"][:4] == TEN[:4] and c["launches"][-2:] == TEN[-2:]
    by = {a["launch"]: a for a in c["args"]}
    assert (by[0]["live"]["te"], by[1]["rope"]["t_max"], by[2]["pool"]["t_max"], by[3]["step"]["t_max"], by[3]["step"]["S_cmp"]) == (3, 3, 3, 3, 0)
    assert routes["layer_decode_paged/t_max_below_S_plan"]["route"] == 1


@pytest.mark.parametrize("case,what", [
    ("f32_declined", "bf16 / f16 only"), ("D96_declined", "Dk = Dv in {64, 128} and the default block geometry only"), ("h17_declined", "h <= 16"),
    ("w0_declined", "w >= 1"), ("t_max70000_declined", "more than 64 chunks"), ("D128_t_max20000_declined", "more than 16 chunks"),
    ("S17_refused", "tokens per sequence"), ("null_t_pos", "null position array"), ("t_pos_2_bytes_off", "t_pos must be 4-byte aligned"),
    ("null_table", "null block table"), ("table_2_bytes_off", "block table must be 4-byte aligned"),
    ("table_stride_below_max_pages", "row stride of at least max_pages = 2 (got 1)"), ("max_pages0", "max_pages = 0, must be in [1, 2^20]"),
    ("max_pages_above_2pow20", "max_pages = 1048577, must be in [1, 2^20]"), ("n_pages0", "n_pages = 0"), ("null_pool", "null pool pointer"),
    ("K_win_2_bytes_off", "eight pools must be 16-byte aligned"), ("no_workspace", "workspace"), ("DECODE_UNFUSED_1_declined", "DECODE_UNFUSED = 1")])
def test_declines_name_the_limit_and_launch_nothing(routes, case, what):
    c = routes["layer_decode_paged/" + case]
    assert c["rc"] == INVALID and c["error"].startswith("layer_decode_paged: ") and what in c["error"], c
    assert c["launches"] == [] and c["geometry"] == [] and c["memsets"] == 0 and c["args"] == []


@pytest.mark.parametrize("case", ["f32_declined", "D96_declined", "h17_declined", "w0_declined", "t_max70000_declined", "D128_t_max20000_declined",
                                  "DECODE_UNFUSED_1_declined"])
def test_the_plan_reports_a_declined_shape(routes, case):
    p = routes["layer_decode_paged/" + case + "_plan"]
    assert (p["rc"], p["launches"], p["route"]) == (0, 0, -1)


# ---- the queries through ctypes: no HIP call ------------------------------------------------------------------------------------------------
def plan(d, B, S, max_pages, t_max, S_sel=None):
    from nsa_vibe_amd import _lib

    n, r = ctypes.c_int(-7), ctypes.c_int(-7)
    te = min(t_max, max_pages * 1024 - 1)
    S_sel = -(-(te + 1) // 64) if S_sel is None else S_sel
    rc = _lib.lib().nsa_layer_decode_paged_plan(ctypes.byref(d) if d is not None else None, B, S, max_pages, t_max, S_sel, ctypes.byref(n), ctypes.byref(r))
    return rc, n.value, r.value


def test_plan_and_workspace_queries(tune):
    from nsa_vibe_amd import _lib

    L, d = _lib.lib(), layer()
    assert plan(d, 3, 8, 2, 1059) == (0, 10, 1)
    assert plan(d, 600, 3, 2, 1059) == (0, 8, 1)     # many rows: the band branches run unsplit, no combine launches
    assert plan(d, 3, 8, 2, 5000) == (0, 10, 1)      # t_max beyond the capacity: te = max_pages 1024 - 1
    assert plan(layer(D=128, dim=1536), 3, 4, 2, 1059) == (0, 10, 1)
    assert plan(layer(F32), 3, 8, 2, 1059) == (0, 0, -1)
    assert plan(d, 3, 8, 128, 70000) == (0, 0, -1)
    for args, kw in [((3, 17, 2, 1059), {}), ((3, 0, 2, 1059), {}), ((0, 8, 2, 1059), {}), ((3, 8, 0, 1059), {}), ((3, 8, (1 << 20) + 1, 1059), {}),
                     ((3, 8, 2, -1), {}), ((3, 8, 2, 1059), {"S_sel": 16})]:
        rc, n, r = plan(d, *args, **kw)
        assert rc != 0 and (n, r) == (0, -1), (args, kw)
    assert plan(None, 3, 8, 2, 1059)[0] != 0
    tune("DECODE_UNFUSED", 1)
    assert plan(d, 3, 8, 2, 1059) == (0, 0, -1)
    ref = ctypes.byref(d)
    ws = L.nsa_layer_decode_paged_workspace
    assert ws(None, 3, 8, 2) == 0 and ws(ref, 0, 8, 2) == 0 and ws(ref, 3, 0, 2) == 0 and ws(ref, 3, 17, 2) == 0 and ws(ref, 3, 8, 0) == 0
    assert ws(ref, 3, 8, (1 << 20) + 1) == 0
    assert ws(ref, 3, 8, 2) >= L.nsa_layer_decode_ragged_workspace(ref, 3, 8, 2048) + 4 * 3
    assert ws(ref, 3, 8, 1 << 20) == ws(ref, 3, 8, 128)  # it does not grow with max_pages beyond the contexts the unsplit forms reach
