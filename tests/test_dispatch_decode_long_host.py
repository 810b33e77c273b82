"""Host side of the long-row form of the ragged / paged decode step (no GPU): switch DECODE_LONG, plan form 3.

`dispatch_check <library> decode_long` (csrc/dispatch_check.cpp: the library's host code against a HIP runtime that counts and refuses every
launch) walks nsa_sel_decode_ragged, nsa_sel_decode_paged, nsa_layer_decode_ragged and nsa_layer_decode_paged on the shapes the unsplit
forms decline.  With the switch at 1 each is ONE decode_rows / decode_paged launch of R workgroups, NS = 1, nchunk of the largest row, the
position pointer as given, a null workspace, no memset, plan {launches 1, form 3}; t_max = 131,071 is accepted and 131,072 declined with
the message that names the limit; a shape inside the unsplit forms keeps form 0 / 1; with the switch back at 0 the three old messages
return verbatim; the layer calls keep the launch counts and workspaces of their in-range plans."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

INVALID = -1  # NSA_ERR_INVALID
LIMIT = ("t_max is beyond the long-row form: at most 131,072 tokens per sequence (t_max <= 131,071), 128 chunks of 64 compressed tokens and 2048 "
         "selection blocks per row")


def ncmp(t):
    return 0 if t + 1 < 32 else (t + 1 - 32) // 16 + 1


@pytest.fixture(scope="module")
def routes():
    from nsa_vibe_amd import _lib

    assert _lib.get_tuning("DECODE_LONG") == 0 or "NSA_HIP_DECODE_LONG" in os.environ  # the default: off
    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    r = subprocess.run([os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH, "decode_long"], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_the_switch_and_only_the_long_cases(routes, tune):
    tune("DECODE_LONG", 1)
    from nsa_vibe_amd import _lib

    assert _lib.get_tuning("DECODE_LONG") == 1
    assert routes and all(k.split("/")[0] in ("sel_decode_ragged", "sel_decode_paged", "layer_decode_ragged", "layer_decode_paged") for k in routes)
    assert all(k.split("/")[1].startswith(("long_", "off_", "in_range_")) for k in routes)


# case -> (B, S, D, t_max, waves per row)
LONG = {
    "long_D128_t_max20000": (3, 1, 128, 20000, 8),
    "long_t_max70000": (1, 1, 64, 70000, 16),
    "long_B200_t_max40000": (200, 1, 64, 40000, 8),
    "long_t_max131071": (1, 1, 64, 131071, 16),
}


@pytest.mark.parametrize("entry,launcher", [("sel_decode_ragged", "decode_rows launch"), ("sel_decode_paged", "decode_paged launch")])
@pytest.mark.parametrize("case", sorted(LONG))
def test_long_rows_are_one_launch_in_form_3(routes, tune, entry, launcher, case):
    tune("DECODE_LONG", 1)
    B, S, D, t_max, nw = LONG[case]
    c = routes[f"{entry}/{case}"]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0), c
    assert c["launches"] == [launcher]
    (geom,) = c["geometry"]
    grid, block, lds = geom.split("/")
    R = B * S * 2
    assert grid == f"{R},1,1" and block == f"{nw * 64},1,1"
    # V tiles of the waves + the tail (+ three K tiles of the forced-block prefetch on 16 waves) (+ the table entries of the paged form)
    tile = 8192 if D == 64 else 16384
    want = nw * tile + 1024 + 4 * 200 + (3 * tile if nw == 16 else 0) + (512 if entry == "sel_decode_paged" else 0)
    assert int(lds) == want <= 160 * 1024
    assert c["plan"] == {"rc": 0, "launches": 1, "form": 3}
    s = c["step"]
    assert s["t_pos"] == "t_pos+20"
    assert (s["R"], s["S"], s["G"], s["NS"], s["nchunk"], s["t_max"]) == (R, S, 2, 1, (ncmp(t_max) + 63) // 64, t_max)
    assert s["nchunk"] <= 128 and s["S_sel"] <= 2048
    if entry == "sel_decode_paged":
        assert (s["block_table"], s["capacity"]) == ("table+28", (t_max // 1024 + 1) * 1024)


def test_the_limit_is_the_launch_with_128_chunks(routes, tune):
    tune("DECODE_LONG", 1)
    for entry in ("sel_decode_ragged", "sel_decode_paged"):
        s = routes[f"{entry}/long_t_max131071"]["step"]
        assert (s["nchunk"], s["S_cmp"], s["S_sel"]) == (128, 8191, 2048)
    c = routes["sel_decode_ragged/long_D128_S4_t_max131071"]
    assert c["rc"] == 0 and c["launches"] == ["decode_rows launch"] and c["geometry"][0].startswith("24,1,1/512,1,1/")
    assert c["plan"]["form"] == 3 and c["step"]["nchunk"] == 128
    c = routes["sel_decode_paged/long_t_max131071_max_pages4096"]  # a pool far larger than any live row: planned from t_max
    assert c["rc"] == 0 and c["plan"] == {"rc": 0, "launches": 1, "form": 3} and c["step"]["nchunk"] == 128 and c["step"]["capacity"] == 4096 * 1024


@pytest.mark.parametrize("entry,who", [("sel_decode_ragged", "decode_ragged"), ("sel_decode_paged", "decode_paged")])
def test_past_the_limit_declines_with_the_new_message(routes, tune, entry, who):
    tune("DECODE_LONG", 1)
    c = routes[f"{entry}/long_t_max131072_declined"]
    assert c["rc"] == INVALID and c["launches"] == [] and c["memsets"] == 0 and c["step"] is None
    assert c["error"].startswith(f"{who}: {LIMIT}"), c["error"]
    assert c["plan"] == {"rc": 0, "launches": 0, "form": -1}


def test_shapes_inside_the_unsplit_forms_keep_their_form(routes, tune):
    tune("DECODE_LONG", 1)
    for entry in ("sel_decode_ragged", "sel_decode_paged"):
        c = routes[f"{entry}/long_t_max100_form0"]
        assert c["rc"] == 0 and c["plan"] == {"rc": 0, "launches": 1, "form": 0} and c["step"]["nchunk"] == 1
    c = routes["sel_decode_ragged/long_t_max40000_form1"]
    assert c["rc"] == 0 and c["plan"] == {"rc": 0, "launches": 1, "form": 1} and c["step"]["nchunk"] == 40


def test_the_step_switch_still_declines(routes, tune):
    tune("DECODE_LONG", 1)
    c = routes["sel_decode_ragged/long_DECODE_STEP_0_declined"]
    assert c["rc"] == INVALID and c["launches"] == [] and "switched off (DECODE_STEP = 0 or DECODE_UNFUSED = 1)" in c["error"]
    assert c["plan"] == {"rc": 0, "launches": 0, "form": -1}


OFF = {
    "off_D128_t_max20000_declined": "t_max is beyond the unsplit form at D = 128: more than 16 chunks of 64 compressed tokens per row",
    "off_t_max70000_declined": "t_max is beyond the unsplit forms at 16 waves per row: more than 64 chunks of 64 compressed tokens per row",
    "off_B200_t_max40000_declined": "t_max is beyond the unsplit forms at 8 waves per row (more than 256 rows): more than 32 chunks of 64 compressed tokens per row",
}


@pytest.mark.parametrize("entry,who", [("sel_decode_ragged", "decode_ragged"), ("sel_decode_paged", "decode_paged")])
@pytest.mark.parametrize("case", sorted(OFF))
def test_switch_off_brings_the_old_messages_back(routes, tune, entry, who, case):
    tune("DECODE_LONG", 0)
    c = routes[f"{entry}/{case}"]
    assert c["rc"] == INVALID and c["launches"] == [] and c["memsets"] == 0 and c["step"] is None
    assert c["error"].startswith(f"{who}: {OFF[case]} (B = "), c["error"]
    assert c["plan"] == {"rc": 0, "launches": 0, "form": -1}


@pytest.mark.parametrize("entry,sel", [("layer_decode_ragged", "decode_rows launch"), ("layer_decode_paged", "decode_paged launch")])
def test_layer_twins_keep_the_launch_counts_of_in_range_plans(routes, tune, entry, sel):
    tune("DECODE_LONG", 1)
    for long_case, near in (("long_t_max70000", "in_range_m7c_B3_S8"), ("long_t_max131071", "in_range_m7c_B3_S8"),
                            ("long_D128_t_max20000", "in_range_D128_B3_S4")):
        a, b = routes[f"{entry}/{long_case}"], routes[f"{entry}/{near}"]
        pa, pb = routes[f"{entry}/{long_case}_plan"], routes[f"{entry}/{near}_plan"]
        assert (a["rc"], a["error"]) == (0, "") and (b["rc"], b["error"]) == (0, ""), (a["error"], b["error"])
        assert a["launches"] == b["launches"] and a["launches"].count(sel) == 1  # the same launchers in the same order, one for the selected branch
        assert a["memsets"] == b["memsets"]
        assert (pa["rc"], pa["route"]) == (0, 1) and pa["launches"] == pb["launches"] >= 6
        (step,) = [x["step"] for x in a["args"] if "step" in x]
        assert step["t_pos"].startswith("t_pos+20" if entry == "layer_decode_ragged" else "ws+")  # (the paged layer hands on its verdicts in the workspace)
        assert step["nchunk"] == (ncmp(step["t_max"]) + 63) // 64 > (16 if "D128" in long_case else 64)
    # the paged workspace does not grow with the context (sized for 2^17 tokens at most)
    if entry == "layer_decode_paged":
        assert routes[f"{entry}/long_t_max70000_plan"]["workspace"] == routes[f"{entry}/long_t_max131071_plan"]["workspace"]
    c, p = routes[f"{entry}/long_t_max131072_declined"], routes[f"{entry}/long_t_max131072_declined_plan"]
    assert c["rc"] == INVALID and c["launches"] == [] and LIMIT in c["error"]
    assert (p["rc"], p["launches"], p["route"]) == (0, 0, -1)
    c, p = routes[f"{entry}/off_t_max70000_declined"], routes[f"{entry}/off_t_max70000_declined_plan"]
    assert c["rc"] == INVALID and c["launches"] == [] and OFF["off_t_max70000_declined"] in c["error"]
    assert (p["rc"], p["launches"], p["route"]) == (0, 0, -1)
