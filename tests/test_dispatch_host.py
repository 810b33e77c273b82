"""Host dispatch layer of the C ABI (no GPU): the workspace queries, the refusals that come before the first HIP call and the tuning
table answer what the commit before the dispatch layer was folded onto shared helpers (csrc/nsa_host.hpp) answered.

tests/dispatch_probe.py asks the library in a fresh process (no earlier test has touched a tuning switch); the sizes and tuning defaults
it prints are compared with tests/golden/dispatch_host_sizes.json, recorded by the same probe from that earlier commit's library.

What runs after the first HIP call is checked by nsa_vibe_amd/dispatch_check (csrc/dispatch_check.cpp, built beside the library): a host
program that answers the library's HIP calls itself -- hipMalloc from the heap, memsets on host memory, every kernel launch counted and
refused -- and so walks each entry point's route on real pointers: the launchers in order, each launch's grid / block / LDS bytes, the
memsets, the status and the message.  tests/golden/dispatch_host_launches.json is its output on that earlier commit's library."""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def probe():
    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}  # no switch seeded from the environment, the product library
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dispatch_probe.py")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "dispatch_host_sizes.json")) as f:
        return json.load(f)


def test_workspace_sizes_are_the_recorded_ones(probe, recorded):
    sizes, want = probe["sizes"], recorded["sizes"]
    assert sorted(sizes) == sorted(want)
    wrong = {k: (sizes[k], want[k]) for k in want if sizes[k] != want[k]}
    assert not wrong, wrong
    # the table covers what the folding could confuse: the scorer's route changes at S = 64 for decode-normalised rows only, so an extend
    # from an empty cache and a prefill of the same rows keep different sizes from there on, and equal ones below
    for B in (1, 8):
        assert sizes[f"prefill/m7c_bf16/B{B}/S63"] == sizes[f"extend/m7c_bf16/B{B}/S63/t0"]
    for S in (64, 100):
        assert sizes[f"prefill/m7c_bf16/B1/S{S}"] != sizes[f"extend/m7c_bf16/B1/S{S}/t0"]
    assert sizes["scores_rows/m7c_bf16/B1/S64/t0/norm0/v0"] != sizes["scores_rows/m7c_bf16/B1/S64/t0/norm1/v0"]
    assert sizes["scores_rows/m7c_bf16/B1/S1/t0/norm0/v0"] == 0  # S < l: no compressed token, nothing to score
    assert all(v > 0 for k, v in sizes.items() if not k.startswith("scores_rows/"))


def test_tuning_defaults_are_the_recorded_ones(probe, recorded):
    assert probe["tuning"] == recorded["tuning"]
    assert len(probe["tuning"]) == 23


INVALID = -1  # NSA_ERR_INVALID
REFUSED = {
    "prefill/null_desc": "layer_prefill: null layer descriptor",
    "extend/null_desc": "layer_extend: null layer descriptor",
    "prefill/zero_desc": "layer_prefill: bad geometry (Dk, Dv must be even)",
    "extend/zero_desc": "layer_extend: bad geometry (Dk, Dv must be even)",
    "prefill/null_cache": "layer_prefill: null cache pointer",
    "extend/null_cache": "layer_extend: null cache pointer",
    "prefill/capacity": "layer_prefill: 129 tokens exceed the cache capacity 128",
    "extend/capacity": "layer_extend: tokens [100,129) exceed the cache capacity 128",
    "extend/negative_t0": "layer_extend: tokens [-1,28) exceed the cache capacity 128",
    "prefill/bad_S_sel": "layer_prefill: block metadata (S_sel=1) does not cover 100 tokens",
    "extend/bad_S_sel": "layer_extend: block metadata (S_sel=1) does not cover 100 tokens",
    "prefill/bad_selector": "layer_prefill: unknown selector 7",
    "prefill/no_workspace": "layer_prefill: workspace missing, misaligned or too small",
    "extend/no_workspace": "layer_extend: workspace missing, misaligned or too small",
    "prefill/small_workspace": "layer_prefill: workspace missing, misaligned or too small",
    "extend/small_workspace": "layer_extend: workspace missing, misaligned or too small",
    "prefill/misaligned_workspace": "layer_prefill: workspace missing, misaligned or too small",
    "prefill/cmp_cache_small": "layer_prefill: compressed cache too small",
    "extend/cmp_cache_small": "layer_extend: compressed cache too small",
    "decode/position": "layer_decode_step: position 128 outside the cache capacity 128",
    "decode/bad_S_sel": "layer_decode_step: block metadata (S_sel=1) does not cover token 100",
    "decode/no_workspace": "layer_decode_step: workspace missing, misaligned or too small",
    "decode/small_workspace": "layer_decode_step: workspace missing, misaligned or too small",
    "sel_attn_fwd/mfma_f32": "sel_attn_fwd: MFMA variant requested but shape/dtype/alignment unsupported",
    "sel_attn_fwd/mfma_unaligned": "sel_attn_fwd: MFMA variant requested but shape/dtype/alignment unsupported",
    "band_attn_fwd/mfma_f32": "band_attn_fwd: MFMA variant requested but shape/dtype/alignment unsupported",
    "band_attn_bwd/no_workspace": "band_attn_bwd: workspace missing, misaligned or too small",
    "tuning/unknown": "unknown tuning switch 'nope'",
    "tuning/decode_stop": "DECODE_STOP is a measurement aid of the TIMELINE build (make TIMELINE=1)",
}


@pytest.mark.parametrize("label", sorted(REFUSED))
def test_refusals_keep_their_status_and_message(probe, label):
    assert probe["refused"][label] == [INVALID, REFUSED[label]]


def test_decode_stop_accepts_zero(probe):
    assert probe["refused"]["tuning/decode_stop_zero"][0] == 0
    assert set(probe["refused"]) == set(REFUSED) | {"tuning/decode_stop_zero"}


# ---- routes on real pointers: the library's host code against a HIP runtime that refuses every launch

@pytest.fixture(scope="module")
def routes():
    from nsa_vibe_amd import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    r = subprocess.run([os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def recorded_routes():
    with open(os.path.join(GOLDEN, "dispatch_host_launches.json")) as f:
        return json.load(f)


def test_routes_are_the_recorded_ones(routes, recorded_routes):
    """Same launches in the same order with the same grids, same memsets, same status and message, for every case."""
    assert sorted(routes) == sorted(recorded_routes)
    wrong = {k: (routes[k], recorded_routes[k]) for k in recorded_routes if routes[k] != recorded_routes[k]}
    assert not wrong, wrong


def launches(case):
    return [name.removesuffix(" launch") for name in case["launches"]]


def test_unaligned_operands_keep_the_generic_kernels(routes):
    assert launches(routes["sel_attn_fwd/aligned"])[0] == "sel_attn_fwd_mfma"
    for case in ("K_2_bytes_off", "K_8_bytes_off", "kss_not_8"):
        assert launches(routes[f"sel_attn_fwd/{case}"]) == ["sel_attn_fwd_generic"], case
    assert launches(routes["sel_attn_bwd/aligned"]) == ["bwd_delta", "bwd_dq_rows", "bwd_hitmap", "bwd_dkdv"]
    for case in ("K_2_bytes_off", "dO_8_bytes_off", "workspace_one_byte_short", "generic_asked"):
        assert launches(routes[f"sel_attn_bwd/{case}"]) == ["sel_attn_bwd_generic"], case
    assert launches(routes["band_attn_fwd/aligned"])[0] == "band_attn_fwd(split)"
    for case in ("K_2_bytes_off", "O_4_bytes_off"):
        assert launches(routes[f"band_attn_fwd/{case}"]) == ["band_attn_fwd_generic"], case
    assert launches(routes["band_attn_bwd/aligned"]) == ["band_ranges", "bwd_delta", "band_attn_bwd_dq", "bwd_hitmap", "bwd_dkdv"]
    assert routes["band_attn_bwd/workspace_exact"]["launches"] == routes["band_attn_bwd/aligned"]["launches"]
    for case in ("K_2_bytes_off", "dO_8_bytes_off"):
        assert launches(routes[f"band_attn_bwd/{case}"]) == ["band_ranges", "sel_attn_bwd_generic"], case


@pytest.mark.parametrize("entry, message", [
    ("sel_attn_fwd", "sel_attn_fwd: MFMA variant requested but shape/dtype/alignment unsupported"),
    ("sel_attn_bwd", "sel_attn_bwd: MFMA variant requested but shape/dtype/alignment/workspace unsupported"),
    ("band_attn_fwd", "band_attn_fwd: MFMA variant requested but shape/dtype/alignment unsupported"),
    ("band_attn_bwd", "band_attn_bwd: MFMA variant requested but shape/dtype/alignment unsupported"),
])
def test_forced_mfma_variant_fails_on_unaligned_operands(routes, entry, message):
    case = routes[f"{entry}/forced_mfma_unaligned"]
    assert (case["rc"], case["error"]) == (INVALID, message)
    assert launches(case) == (["band_ranges"] if entry == "band_attn_bwd" else [])  # the band backward lists its ranges before it decides
    assert routes["sel_attn_fwd/forced_mfma_aligned"]["rc"] == 0


def test_backward_zeroes_dK_dV_on_the_generic_route_only(routes):
    """The program fills dK, dV and dQ with 0xff before each call; the memsets are carried out on its host memory."""
    for case in ("sel_attn_bwd/K_2_bytes_off", "sel_attn_bwd/generic_asked", "band_attn_bwd/K_2_bytes_off"):
        assert routes[case]["dK_zero"] and routes[case]["dV_zero"] and not routes[case]["dQ_zero"], case
        assert routes[case]["memsets"] == 2, case
    for case in ("sel_attn_bwd/aligned", "band_attn_bwd/aligned"):  # the MFMA route writes every element itself (its one memset: the hit maps)
        assert not routes[case]["dK_zero"] and not routes[case]["dV_zero"] and routes[case]["memsets"] == 1, case
    empty = routes["sel_attn_bwd/no_ranges"]  # nothing selected: all three gradients are zero, no launch
    assert empty["dK_zero"] and empty["dV_zero"] and empty["dQ_zero"] and empty["launches"] == [] and empty["memsets"] == 3
    fwd = routes["sel_attn_fwd/no_ranges"]
    assert fwd["O_zero"] and fwd["launches"] == [] and fwd["memsets"] == 2  # O and lse


def test_both_scale_spellings(routes):
    """scale <= 0 asks for 1/sqrt(Dk) (Dk = 64: 0.125), a positive scale is handed to the kernel as given."""
    for entry in ("sel_attn_fwd", "sel_attn_bwd", "band_attn_fwd"):
        assert routes[f"{entry}/scale_default"]["scale"] == 0.125
        assert routes[f"{entry}/scale_given"]["scale"] == 0.25
    assert routes["sel_attn_fwd/scale_negative"]["scale"] == 0.125
    for entry in ("sel_scores_rows/generic_scale", "pcmp_all/scale"):
        assert [routes[f"{entry}_{s}"]["scale"] for s in ("0", "-1", "0.25")] == [0.125, 0.125, 0.25]


def test_workspace_checks_on_real_pointers(routes):
    for entry in ("layer_prefill", "layer_extend", "layer_decode_step", "band_attn_bwd"):
        short = routes[f"{entry}/workspace_one_byte_short"]
        assert (short["rc"], short["error"], short["launches"]) == (INVALID, f"{entry}: workspace missing, misaligned or too small", [])
    for case in ("layer_prefill/workspace_exact", "layer_extend/to_capacity_workspace_exact", "layer_decode_step/workspace_exact"):
        assert routes[case]["rc"] == 0 and routes[case]["launches"], case


def test_extend_accepts_exactly_its_capacity(routes):
    full = routes["layer_extend/to_capacity"]  # tokens [924, 1024) of a cache of 1024
    assert full["rc"] == 0 and launches(full)[0] == "rope_cache_append" and launches(full)[-1] == "gate_combine"
    past = routes["layer_extend/past_capacity"]
    assert (past["rc"], past["error"], past["launches"]) == (INVALID, "layer_extend: tokens [925,1025) exceed the cache capacity 1024", [])
    at = routes["layer_decode_step/position_at_capacity"]
    assert (at["rc"], at["error"]) == (INVALID, "layer_decode_step: position 1024 outside the cache capacity 1024")


def test_prefill_alone_decides_on_SEL_FUSE_and_the_alignment_of_K_cmp(routes):
    # 1024 rows: the attention takes the selector into its launch when SEL_FUSE asks for it -- from the prefill only
    assert "select_topn" in launches(routes["layer_prefill/S512"])
    assert "select_topn" not in launches(routes["layer_prefill/S512_SEL_FUSE"])
    assert routes["layer_extend/t0_S512_SEL_FUSE"] == routes["layer_extend/t0_S512"]
    assert routes["layer_extend/t0_S100_SEL_FUSE"] == routes["layer_extend/t0_S100"]
    assert launches(routes["sel_select_attn_fwd/S512_SEL_FUSE"]) == ["sel_attn_blocks_mfma"]
    assert launches(routes["sel_select_attn_fwd/S512_two_launches"]) == ["select_topn", "sel_attn_blocks_mfma"]
    assert launches(routes["sel_select_attn_fwd/S512_SEL_FUSE_K_2_bytes_off"]) == ["select_topn", "sel_attn_fwd_generic"]
    # an unaligned K_cmp: the generic scorer and the generic compressed branch, for both entry points
    for case in ("layer_prefill/S512_K_cmp_8_bytes_off", "layer_extend/t0_S512_K_cmp_8_bytes_off"):
        assert launches(routes[case])[2:4] == ["pcmp", "map_pcmp"] and "band_attn_fwd_generic" in launches(routes[case]), case
    # no compressed token yet: no scorer launch, zero scores
    assert launches(routes["layer_prefill/S16_no_compressed_token"])[:2] == ["rope_cache_append", "select_topn"]
    # an extend from an empty cache normalises per row: from 64 rows on it leaves the decode-shaped scorer, the prefill of the same rows keeps it
    assert launches(routes["layer_prefill/S100"])[2:4] == ["decode_logits", "decode_pgrp"]
    assert launches(routes["layer_extend/t0_S100"])[2] == "scores_mfma32"
    assert launches(routes["layer_extend/t100_S28"])[2:4] == ["decode_logits", "decode_pgrp"]
    assert launches(routes["sel_scores_rows/S63_norm1"]) == launches(routes["sel_scores_rows/S64_norm0"]) == ["decode_logits", "decode_pgrp"]
    assert launches(routes["sel_scores_rows/S64_norm1"]) == ["scores_mfma32"]


def test_layer_decode_step_routes(routes):
    assert launches(routes["layer_decode_step/t100"]) == ["qkv_rope_append(fast)", "decode_step", "linear_small_mix"]  # three launches
    assert launches(routes["layer_decode_step/t31_first_compressed_token"])[1] == "cmp_pool(wide)"
    assert launches(routes["layer_decode_step/D128_t100"])[:2] == ["qkv_rope_append(fast)", "decode_step"]


# ---- the scorer and selector family: the argument blocks of its launches (csrc/sel_scores_params.hpp), member by member

def blocks(case, key):
    """the argument blocks named `key` of a case's launches, in launch order"""
    return [a[key] for a in case["args"] if key in a]


def test_generic_scorer_walks_its_rows_in_workspace_sized_chunks(routes):
    case = routes["sel_scores_rows/v1_10_rows_workspace_of_3"]  # ten rows, room for three
    assert launches(case) == ["pcmp", "map_pcmp"] * 4
    assert [(p["row0"], p["nrows"]) for p in blocks(case, "PcmpParams")] == [(0, 3), (3, 3), (6, 3), (9, 1)]
    maps = blocks(case, "MapParams")
    assert [m["R"] for m in maps] == [3, 3, 3, 1]
    assert [m["p_grp"] for m in maps] == [f"p_grp+{4 * r0 * m['S_sel']}" for r0, m in zip((0, 3, 6, 9), maps)]  # fp32 [R, S_sel] rows
    assert all(p["p_cmp"] == m["p_cmp"] == "ws+0" for p, m in zip(blocks(case, "PcmpParams"), maps))


def test_q0_norm_l_d_land_in_the_members_of_those_names(routes):
    """q0 = 100, norm = 1, l = 32, d = 16: four neighbouring ints that differ pairwise, on every route"""
    (p,) = blocks(routes["sel_scores_rows/q0_100_v1"], "PcmpParams")
    assert (p["q0"], p["norm"], p["l"], p["d"]) == (100, 1, 32, 16)
    for p in blocks(routes["sel_scores_rows/q0_100_v3"], "DecodeParams"):  # both kernels of the decode-shaped pair
        assert (p["q0"], p["norm"], p["l"], p["d"], p["stencil"]) == (100, 1, 32, 16, 0)
    (p,) = blocks(routes["sel_scores_rows/q0_100_v0"], "ScoresMfmaParams")
    assert (p["q0"], p["norm"], p["l"], p["d_stride"]) == (100, 1, 32, 16)
    (sp,) = blocks(routes["sel_scores_select_rows/mfma32_q0_100"], "SelectParams")[1:]  # the select kernel's: rows select at t0 = q0
    assert (sp["t0"], sp["S"], sp["G"], sp["R"]) == (100, 64, 2, 128)


def test_causal_skip_2_leaves_p_grp_unwritten(routes):
    """the tiled scorer zero-fills p_grp unless the caller reads only what the second sweep writes (causal_skip = 2)"""
    assert [routes[f"sel_scores_rows/causal_skip_{s}"]["memsets"] for s in (0, 1, 2)] == [1, 1, 0]
    for s in (0, 1, 2):
        case = routes[f"sel_scores_rows/causal_skip_{s}"]
        assert launches(case) == ["scores_mfma32"] and blocks(case, "ScoresMfmaParams")[0]["causal_skip"] == s
    empty = routes["sel_scores_rows/S_cmp_0"]  # no compressed token: zero scores, no launch
    assert (empty["rc"], empty["launches"], empty["memsets"]) == (0, [], 1)


def test_selection_inside_the_scorer_launch_gets_the_select_kernels_block(routes):
    """nsa_sel_scores_select_rows on the 32x32x16 route: the SelectParams handed to the scorer launch (SCORES_SELECT 1) and to the
    select_topn launch behind it (default) are the same block, member for member -- there is no field the scorer kernel's selection does not
    take from it (its row function is the select kernel's own)."""
    for mode in ("sequential", "batched"):
        inside = routes[f"sel_scores_select_rows/mfma32_{mode}_SCORES_SELECT_1"]
        behind = routes[f"sel_scores_select_rows/mfma32_{mode}"]
        assert launches(inside) == ["scores_mfma32"] and launches(behind) == ["scores_mfma32", "select_topn"]
        (sp_inside,) = blocks(inside, "SelectParams")
        none, sp_behind = blocks(behind, "SelectParams")
        assert sp_inside == sp_behind and sp_inside["out"] == "ranges+0" and sp_inside["p_grp"] == "p_grp+0"
        assert none["out"] == "null" and none["R"] == 0  # the scorer launch without a selection carries an empty block
        assert blocks(inside, "ScoresMfmaParams") == blocks(behind, "ScoresMfmaParams")
    for mode, message in (("sequential", "select (sequential): out_width must be n_top"),
                          ("batched", "select (batched): out_width 2 != nsa_batched_ranges_width()")):
        wrong = routes[f"sel_scores_select_rows/{mode}_wrong_out_width"]
        assert (wrong["rc"], wrong["error"], wrong["launches"]) == (INVALID, message, [])


def test_unaligned_K_cmp_keeps_the_generic_scorer(routes):
    """K_cmp 8 bytes off its 16-byte alignment: pcmp + map_pcmp from nsa_sel_scores_select_rows and from the layer calls; nsa_sel_scores_rows
    itself never leaves the route of a shape (variant 0 refuses, as a forced variant 2 does): its callers ask for variant 1."""
    assert launches(routes["sel_scores_select_rows/K_cmp_8_bytes_off"]) == ["pcmp", "map_pcmp", "select_topn"]
    assert blocks(routes["sel_scores_select_rows/K_cmp_8_bytes_off"], "PcmpParams")[0]["Kc"] == "Kc+8"
    assert launches(routes["sel_scores_rows/K_cmp_8_bytes_off_v1"]) == launches(routes["sel_scores_rows/css_not_8_v1"]) == ["pcmp", "map_pcmp"]
    refusal = ("sel_scores: MFMA route needs bf16/f16, Dk in {64,128}, h <= 16, l = 2d, l' = 4d and 16-byte aligned rows "
               "(pass variant 1 for the generic route)")
    for case in ("K_cmp_8_bytes_off", "css_not_8", "K_cmp_8_bytes_off_forced_v2", "css_not_8_forced_v2"):
        assert (routes[f"sel_scores_rows/{case}"]["rc"], routes[f"sel_scores_rows/{case}"]["error"]) == (INVALID, refusal), case
    for case in ("layer_prefill/S512_K_cmp_8_bytes_off", "layer_extend/t0_S512_K_cmp_8_bytes_off", "layer_prefill/S100_K_cmp_8_bytes_off",
                 "layer_extend/t0_S100_K_cmp_8_bytes_off"):
        assert launches(routes[case])[2:4] == ["pcmp", "map_pcmp"], case


def test_decode_step_separate_launches_and_their_blocks(routes):
    fused = routes["sel_decode_step/t100_DECODE_STEP_0"]
    assert launches(fused) == ["decode_score_select", "sel_attn_decode_wg"]
    (a,) = fused["args"]
    assert (a["cand"], a["t_token"], a["DecodeParams"]["stencil"], a["SelectParams"]["t0"], a["SelectParams"]["out"]) == (1, 100, 1, 100, "ranges+0")
    other = routes["sel_decode_step/t100_DECODE_STEP_0_geometry_16_16_32"]["args"][0]  # l != 2d: the CSC arrays, not the stencil
    assert (other["DecodeParams"]["stencil"], other["SelectParams"]["l_sel"], other["SelectParams"]["l_sel_shift"]) == (0, 32, 5)
    unfused = routes["sel_decode_step/t100_DECODE_STEP_0_DECODE_UNFUSED_1"]
    assert launches(unfused) == ["decode_logits", "decode_pgrp", "select_topn", "sel_attn_decode_wg"]
    logits, pgrp = blocks(unfused, "DecodeParams")
    (sp,) = blocks(unfused, "SelectParams")
    assert logits == pgrp and logits["p_grp"] == sp["p_grp"] and sp == dict(a["SelectParams"], p_grp=sp["p_grp"])


# ---- the few-row projection family (csrc/layer_fused.hip: proj_route): form, template instance and operands of every launch

def proj(case):
    """the family's launches of a case: [(launcher, record)], the record as dispatch_check's run_proj prints it"""
    names = launches(case)
    return [(names[p["launch"]], p) for p in case["proj"]]


def lin(routes, M, N, K, tag=""):
    ((name, p),) = proj(routes[f"linear_small/{tag}M{M}_N{N}_K{K}"])
    assert (p["M"], p["N"], p["K"], p["W"], p["out"]) == (M, N, K, "W_lin+0", "out+0")
    return name, p["kernel"]


def test_linear_small_forms_change_where_the_route_says(routes):
    for M in (1, 2):
        for N, K in ((40, 8), (37, 520), (36, 1032), (36, 3072), (36, 4096), (4097, 8), (4100, 1000), (4100, 1536)):
            assert lin(routes, M, N, K)[0] == "linear_small(fast)", (M, N, K)
        assert lin(routes, M, 36, 4104)[0] == "linear_small"  # past the all-loads-first form's 8 chunks
    for case in ("M2_N37_K520_A_2_bytes_off", "M2_N4100_K1000_A_2_bytes_off", "f32_M1_N36_K1032", "f32_M2_N4100_K1000", "f32_M5_N37_K520",
                 "M3_N40_K40", "M3_N40_K64_A_2_bytes_off"):
        assert launches(routes[f"linear_small/{case}"]) == ["linear_small"], case
    for M, N, K in ((3, 40, 64), (9, 36, 2016), (9, 36, 2048), (70, 37, 1024)):
        assert lin(routes, M, N, K)[0] == "linear_small(mfma)"
    assert routes["linear_small/M70_N37_K1024"]["geometry"] == ["3,2,1/256,1,1/0"]  # ragged column tile, second row tile
    for case in ("M0_N40_K8", "M1_N0_K8"):
        assert (routes[f"linear_small/{case}"]["rc"], routes[f"linear_small/{case}"]["launches"]) == (0, [])


def test_linear_small_template_instances(routes):
    """Two launches share a kernel ordinal exactly when they run the same template instance: the chunk tiers (2, 4, 6, 8 x 512 elements),
    four weight rows per wave from N = 4096 on with at most two chunks, 4 or 8 MFMA waves.  A larger tier would give the same bits."""
    k = {(N, K): lin(routes, 1, N, K)[1] for N, K in ((40, 8), (37, 520), (36, 1032), (36, 3072), (36, 4096), (36, 4104), (4097, 8), (4100, 1000),
                                                      (4100, 1536))}
    assert all(lin(routes, 2, N, K)[1] == v for (N, K), v in k.items())  # one and two rows: the same instances
    assert k[40, 8] == k[37, 520] and k[4097, 8] == k[4100, 1000] and k[4100, 1536] == k[36, 1032]
    assert len({k[40, 8], k[36, 1032], k[36, 3072], k[36, 4096], k[36, 4104], k[4097, 8]}) == 6
    assert routes["linear_small/M1_N4100_K1000"]["geometry"] == ["257,1,1/256,1,1/0"]  # 16 columns per workgroup
    assert routes["linear_small/M1_N4100_K1536"]["geometry"] == ["1025,1,1/256,1,1/0"]  # three chunks: one weight row per wave
    assert lin(routes, 2, 4100, 1000, "f32_")[1] != lin(routes, 1, 36, 1032, "f32_")[1] == lin(routes, 5, 37, 520, "f32_")[1]
    four, eight = lin(routes, 9, 36, 2016)[1], lin(routes, 9, 36, 2048)[1]
    assert four == lin(routes, 3, 40, 64)[1] == lin(routes, 70, 37, 1024)[1] != eight
    assert routes["linear_small/M9_N36_K2048"]["geometry"] == ["3,1,1/512,1,1/0"]
    for epi in (1, 2):  # the epilogue is an argument, not an instance
        for M, N, K in ((1, 37, 520), (1, 36, 4104), (3, 40, 64)):
            ((_, p),) = proj(routes[f"linear_small/M{M}_N{N}_K{K}_epi{epi}"])
            assert (p["kernel"], p["epi"], p["res"]) == (lin(routes, M, N, K)[1], epi, "res+0" if epi == 2 else "null")


def test_block_step_folds_both_norms_where_the_route_takes_them(routes):
    for case, x in (("B1", "x+0"), ("B2", "x+0"), ("B1_x_2_bytes_off", "x+2"), ("dim776_B3", "x+0")):
        c = routes[f"block_decode_step/{case}"]
        assert "rmsnorm_rows" not in launches(c), case
        (_, qkv), (_, out), (_, fc1), (_, fc2) = proj(c)
        assert (qkv["A"], qkv["norm_w"], fc1["norm_w"], fc1["A"]) == (x, "norm1_w+0", "norm2_w+0", out["out"]), case
        assert (out["epi"], out["res"], fc1["epi"], fc2["epi"], fc2["res"], fc2["out"]) == (2, x, 1, 2, out["out"], "y+0"), case
    assert launches(routes["block_decode_step/B1_x_2_bytes_off"])[0] == "qkv_rope_append"  # the chunk loop
    assert launches(routes["block_decode_step/dim776_B3"]) == ["qkv_rope_append", "decode_step", "linear_small_mix", "linear_small", "linear_small(mfma)"]
    c = routes["block_decode_step/B3"]  # the MFMA form reads normalised rows: both norms are launches of their own, into the workspace
    assert launches(c) == ["rmsnorm_rows", "qkv_rope_append(mfma)", "decode_step", "linear_small_mix", "rmsnorm_rows", "linear_small(mfma)", "linear_small(mfma)"]
    (_, qkv), (_, out), (_, fc1), (_, fc2) = proj(c)
    assert qkv["A"].startswith("ws+") and fc1["A"].startswith("ws+") and fc1["A"] != out["out"]
    assert {qkv["norm_w"], fc1["norm_w"], fc2["norm_w"]} == {"null"} and (out["res"], fc2["res"]) == ("x+0", out["out"])
    assert fc1["kernel"] != fc2["kernel"]  # K = 3072: eight waves


def test_model_step_lm_head(routes):
    for vocab in (131, 4100):
        for tail in ("", "_next_tokens"):
            one, three = routes[f"model_decode_step/vocab{vocab}_B1{tail}"], routes[f"model_decode_step/vocab{vocab}_B3{tail}"]
            name, head = proj(one)[-1]
            assert (name, head["norm_w"], head["W"], head["out"], head["N"], head["epi"]) == ("linear_small(fast)", "norm_f_w+0", "W_lm+0", "logits+0", vocab, 0)
            name, head3 = proj(three)[-1]
            assert (name, head3["norm_w"], head3["out"]) == ("linear_small(mfma)", "null", "logits+0") and head3["A"] != proj(three)[-2][1]["out"]
            assert launches(three)[-(3 if tail else 1) - 1] == "rmsnorm_rows"
            assert (launches(one)[-2:] == ["argmax_part", "argmax_final"]) == bool(tail)
            assert len(proj(one)) == 9 and len(proj(three)) == 9  # two blocks of four, the head
    # four weight rows per wave at vocab 4100, as nsa_linear_small at the same N with one chunk pair
    assert proj(routes["model_decode_step/vocab4100_B1"])[-1][1]["kernel"] == lin(routes, 1, 4100, 1000)[1]
    assert proj(routes["model_decode_step/vocab131_B1"])[-1][1]["kernel"] == lin(routes, 1, 37, 520)[1]


def test_layer_step_mix_rides_in_the_projection_up_to_32_rows(routes):
    for B in (2, 3, 32):
        c = routes[f"layer_decode_step/B{B}_t100"]
        assert launches(c) == ["qkv_rope_append(fast)" if B <= 2 else "qkv_rope_append(mfma)", "decode_step", "linear_small_mix"]
        _, mix = proj(c)[-1]
        assert (mix["M"], mix["G"], mix["W"], mix["out"], mix["epi"], mix["res"]) == (B, 2, "W_out+0", "y+0", 0, "null")
        assert len({mix["A"], mix["Os"], mix["Ow"], mix["gates"]}) == 4
    assert launches(routes["layer_decode_step/B33_t100"]) == ["qkv_rope_append(mfma)", "decode_step", "decode_finish", "linear_small(mfma)"]
    assert launches(routes["layer_decode_step/B33_t100_DECODE_BAND_3"]) == ["qkv_rope_append(mfma)", "decode_step", "linear_small_mix"]
    mixes = [proj(routes[f"layer_decode_step/B{B}_t100"])[-1][1]["kernel"] for B in (2, 3, 32)]
    assert mixes[0] != mixes[1] == mixes[2] == proj(routes["layer_decode_step/B33_t100_DECODE_BAND_3"])[-1][1]["kernel"]
    one, two = routes["layer_decode_rows/B1_t100_S2"], routes["layer_decode_rows/B2_t100_S2"]  # B S rows: the MFMA form from four rows on
    assert (launches(one)[0], launches(one)[-1]) == ("qkv_rope_append(rows)", "linear_small(fast)")
    assert (launches(two)[0], launches(two)[-1]) == ("qkv_rope_append(rows, mfma)", "linear_small(mfma)")
    assert [(p["M"], p["B"], p["S"], p["t0"]) for p in (proj(one)[0][1], proj(two)[0][1])] == [(2, 1, 2, 100), (4, 2, 2, 100)]


# ---- the attention family: the argument blocks of its launches (csrc/sel_attn_params.hpp), member by member

def attn(routes, label, key="SelAttnParams"):
    """(launcher names, the blocks named `key` in launch order) of a case of the attention family"""
    case = routes[label]
    assert case["rc"] == 0, (label, case["error"])
    return launches(case), blocks(case, key)


BASE = dict(Q="Q+0", K="K+0", V="V+0", G=2, h=6, Dk=64, Dv=64, scale=0.125)


def has(block, **want):
    return {k: block[k] for k in want} == want


def test_selection_attention_forms_and_their_members(routes):
    """The form of a selection-attention forward and what its block carries: rows of 1024 and more take the block form (row form at D = 128 or
    with a K row stride other than 64, one row per wave where 16 / h < 2), fewer rows split the keys of a row over waves."""
    for label, lse in (("sel_attn_fwd/blocks", "null"), ("sel_attn_fwd/blocks_lse", "lse+0")):
        names, (p,) = attn(routes, label)
        assert names == ["sel_attn_blocks_mfma"]
        assert has(p, **BASE, ranges="ranges+0", O="O+0", lse=lse, R=1024, S=512, S_kv=512, n=16, ksb=65536, ksg=32768, kss=64, vsb=65536, vsg=32768, vss=64)
        assert has(p, part="null", nsplit=1, map_mode=1, defer_combine=0, fuse_select=0, select="null", tpw=2, nw=1, ks_ws="ws+0", ks_r1=0, ks_r2=0)
        assert routes[label]["args"][0]["cand"] == 0 and routes[label]["args"][0]["SelectParams"]["R"] == 0
    names, (p,) = attn(routes, "sel_attn_fwd/D128_S512_rows")
    assert names == ["sel_attn_rows_mfma"] and has(p, Dk=128, Dv=128, tpw=2, nw=1, wave_lds=16720, ksb=131072, kss=128, part="null", nsplit=1)
    names, (p,) = attn(routes, "sel_attn_fwd/S512_kss72_rows")
    assert names == ["sel_attn_rows_mfma"] and has(p, kss=72, ksg=36864, ksb=73728, vss=64, vsg=32768, tpw=2)
    names, (p,) = attn(routes, "sel_attn_fwd/S512_kss72_h16_one_row_per_wave")
    assert names == ["sel_attn_fwd_mfma"] and has(p, h=16, part="null", nsplit=1, map_mode=1, tpw=0, wave_lds=0)
    for label in ("sel_attn_fwd/split_base_shape", "sel_attn_fwd/S128_Skv32768", "sel_attn_fwd/D128_base_shape"):  # 256 rows: eight splits
        names, (p, c) = attn(routes, label)
        assert names == ["sel_attn_fwd_mfma", "sel_attn_combine"] and p == c, label
        assert has(p, R=256, part="ws+0", nsplit=8, defer_combine=0, ks_ws="null", ks_bytes=0), label


def test_selection_attention_decode_routes(routes):
    """S = 1: one workgroup per row without lse; with lse the split route and its combine, one split without a usable workspace."""
    for label, S_kv in (("sel_attn_fwd/S1_decode_wg", 128), ("sel_attn_fwd/S1_V_slab_under_2GiB", (1 << 24) - 1)):
        names, (a,) = attn(routes, label, "DecAttnArgs")
        assert names == ["sel_attn_decode_wg"] and routes[label]["geometry"] == ["2,1,1/1024,1,1/131600"]
        assert a == dict(Q="Q+0", K="K+0", V="V+0", O="O+0", G=2, h=6, S_kv=S_kv, n=16, ksb=2 * S_kv * 64, ksg=S_kv * 64, kss=64, vsb=2 * S_kv * 64, vsg=S_kv * 64,
                         vss=64, c2=0.180336878)
        assert routes[label]["args"][0]["ranges"] == "ranges+0"
    names, (p, c) = attn(routes, "sel_attn_fwd/S1_lse_split")
    assert names == ["sel_attn_fwd_mfma", "sel_attn_combine"] and p == c
    assert has(p, lse="lse+0", R=2, S=1, part="ws+0", nsplit=16, defer_combine=0, map_mode=0)
    for label in ("sel_attn_fwd/S1_lse_null_workspace", "sel_attn_fwd/S1_lse_workspace_8_bytes_off"):
        names, (p,) = attn(routes, label)
        assert names == ["sel_attn_fwd_mfma"] and has(p, part="null", nsplit=1, ks_ws="null"), label
    big = routes["sel_attn_fwd/S1_V_slab_2GiB"]  # past the decode workgroup's bound the MFMA launcher refuses the slab
    assert (big["rc"], big["error"], big["launches"]) == (INVALID, "MFMA kernel: one (b,g) K/V slab must be smaller than 2 GiB (buffer addressing)", [])


def test_key_split_form_and_its_members(routes):
    names, (p,) = attn(routes, "sel_attn_fwd/S512_Skv32768_key_split")  # every row below 32768: zone 0, no record, no combine
    assert names == ["sel_attn_blocks_mfma"]
    assert has(p, part="ws+0", ks_ws="ws+0", ks_bytes=64 << 20, ks_r1=512, ks_r2=512, ks_w1=16, ks_w2=16, ks_wa=2, ks_wb=0, ks_wc=0, nw=16)
    names, (p,) = attn(routes, "sel_attn_fwd/S512_Skv33280_key_split_rows_in_two")  # every row from 32768 on: two key classes
    assert names == ["sel_attn_blocks_mfma", "sel_attn_ksplit_combine"]
    assert has(p, part="ws+0", ks_r1=0, ks_r2=512, ks_w1=0, ks_w2=16, ks_wa=0, ks_wb=2, ks_wc=0, nw=17)
    merge = routes["sel_attn_fwd/S512_Skv33280_key_split_rows_in_two"]["args"][1]
    assert merge == dict(launch=1, ml="ws+0", acc="ws+196608", O="O+0", lse="null", nbg=2, S=512, G=2, h=6, r1=0, r2=512)
    names, (p,) = attn(routes, "sel_attn_fwd/S512_Skv32768_null_workspace")  # no workspace: the plain block form
    assert names == ["sel_attn_blocks_mfma"] and has(p, part="null", ks_ws="null", ks_bytes=0, ks_w2=0, ks_wa=0)


def test_generic_kernel_and_launcher_refusals_of_the_selection_forward(routes):
    for label in ("sel_attn_fwd/variant_1", "sel_attn_fwd/f32", "sel_attn_fwd/h32"):
        names, (p,) = attn(routes, label)
        assert names == ["sel_attn_fwd_generic"] and has(p, part="null", nsplit=1, ks_ws="null", scale=0.125, R=256), label
    # variant 0 with an operand only the launcher tests: refused there, not routed to the generic kernel
    for label in ("sel_attn_fwd/O_4_bytes_off", "sel_attn_fwd/S512_O_4_bytes_off"):
        assert (routes[label]["rc"], routes[label]["error"], routes[label]["launches"]) == (INVALID, "MFMA kernel: Q/K/V must be 16-byte aligned", []), label
    slab = routes["sel_attn_fwd/slab_2GiB"]
    assert (slab["rc"], slab["error"], slab["launches"]) == (INVALID, "MFMA kernel: one (b,g) K/V slab must be smaller than 2 GiB (buffer addressing)", [])
    # the band forward tests both before it chooses: the generic kernel, no refusal
    names, (p,) = attn(routes, "band_attn_fwd/slab_2GiB_generic", "BandAttnParams")
    assert names == ["band_attn_fwd_generic"] and has(p, S_kv=1 << 20, kss=1024, ksg=1 << 30, ksb=1 << 31)
    assert launches(routes["band_attn_fwd/O_4_bytes_off"]) == ["band_attn_fwd_generic"]


def test_selection_backward_members_on_both_routes(routes):
    want = dict(Q="Q+0", K="K+0", V="V+0", ranges="ranges+0", O="O+0", lse="lse+0", dO="dO+0", dQ="dQ+0", dK="dK+0", dV="dV+0", R=256, S=128, G=2, h=6, Dk=64, Dv=64,
                S_kv=128, n=16, ksb=16384, ksg=8192, kss=64, vsb=16384, vsg=8192, vss=64, scale=0.125, skip_delta_dq=0)
    names, (dq, dkdv) = attn(routes, "sel_attn_bwd/mfma_members", "SelAttnBwdParams")
    assert names == ["bwd_delta", "bwd_dq_rows", "bwd_hitmap", "bwd_dkdv"] and dq == dkdv == want
    assert blocks(routes["sel_attn_bwd/mfma_members"], "delta") == ["ws+0", "ws+0"]
    names, (p,) = attn(routes, "sel_attn_bwd/generic_members", "SelAttnBwdParams")
    assert names == ["sel_attn_bwd_generic"] and p == want
    names, (dq, dkdv) = attn(routes, "sel_attn_bwd/D128_members", "SelAttnBwdParams")
    assert dq == dkdv == dict(want, Dk=128, Dv=128, ksb=32768, ksg=16384, kss=128, vsb=32768, vsg=16384, vss=128, scale=0.5)


def test_parity_modes_members(routes):
    for label in ("sel_attn_first_key_parity/members", "sel_attn_first_key_parity/f32"):
        (a,) = routes[label]["args"]
        assert launches(routes[label]) == ["sel_first_key"]
        assert a == dict(launch=0, V="V+0", ranges="ranges+0", O="O+0", R=256, S=128, G=2, h=6, Dv=64, n=16, S_kv=128, vsb=16384, vsg=8192, vss=64), label
    names, (p,) = attn(routes, "sel_attn_head_causal_parity/members")
    assert names == ["sel_head_causal"] and has(p, **BASE, ranges="ranges+0", O="O+0", lse="null", R=256, S=128, S_kv=128, n=16, ksb=16384, vsg=8192, nsplit=0)


SLIDING = dict(a=0, dd=1, c=0)
COMPRESSED = dict(a=32, dd=16, c=1, w=1 << 30)


def test_band_forward_members(routes):
    names = launches(routes["band_attn_fwd/sliding_members"])
    (p,) = blocks(routes["band_attn_fwd/sliding_members"], "BandAttnParams")
    (c,) = blocks(routes["band_attn_fwd/sliding_members"], "SelAttnParams")  # the combine launch takes the selection family's block
    assert names == ["band_attn_fwd(split)", "band_attn_combine"]
    assert has(p, **BASE, **SLIDING, O="O+0", lse="lse+0", B=1, S=128, S_kv=128, t0=7, w=64, ksb=16384, ksg=8192, kss=64, vsb=16384, vsg=8192, vss=64)
    assert has(p, part="ws+0", nsplit=16, defer_combine=0, tpw=2, map_mode=0)
    assert has(c, O="O+0", lse="lse+0", R=256, h=6, part="ws+0", nsplit=16, Q="null", S_kv=0)
    (p,) = blocks(routes["band_attn_fwd/compressed_members"], "BandAttnParams")
    assert has(p, **BASE, **COMPRESSED, lse="null", S_kv=13, t0=100, ksb=1664, ksg=832, part="ws+0", nsplit=16)
    for label, geometry, S_kv in (("S4096_sliding_members", dict(SLIDING, t0=0, w=64), 4096), ("S4096_compressed_members", dict(COMPRESSED, t0=0), 255)):
        names, (p,) = attn(routes, f"band_attn_fwd/{label}", "BandAttnParams")  # 4096 token groups: no split
        assert names == ["band_attn_fwd"] and has(p, **geometry, S=4096, S_kv=S_kv, part="null", nsplit=1, tpw=2, map_mode=1), label
    names, (p,) = (launches(routes["band_attn_fwd/S1_split"]), blocks(routes["band_attn_fwd/S1_split"], "BandAttnParams"))
    assert names == ["band_attn_fwd(split)", "band_attn_combine"] and has(p, S=1, t0=127, part="ws+0", nsplit=16, defer_combine=0)
    names, (p,) = attn(routes, "band_attn_fwd/S1_null_workspace", "BandAttnParams")
    assert names == ["band_attn_fwd"] and has(p, part="null", nsplit=1)
    for label in ("band_attn_fwd/generic_members", "band_attn_fwd/w_0"):
        names, (p,) = attn(routes, label, "BandAttnParams")
        assert names == ["band_attn_fwd_generic"] and has(p, part="null", nsplit=0, scale=0.125), label


def test_band_backward_members_and_its_generic_fallback(routes):
    case = routes["band_attn_bwd/mfma_members"]
    assert launches(case) == ["band_ranges", "bwd_delta", "band_attn_bwd_dq", "bwd_hitmap", "bwd_dkdv"]
    roff = case["args"][0]["ranges"]  # the ranges sit behind the selection backward's workspace
    assert has(case["args"][0], R=256, S=128, G=2, S_kv=13, t0=100, **COMPRESSED)
    (bp,) = blocks(case, "BandAttnParams")
    assert has(bp, **BASE, **COMPRESSED, O="null", lse="null", B=1, S=128, S_kv=13, t0=100, part="null", nsplit=0)
    assert blocks(case, "BandBwdExtra") == [dict(dO="dO+0", lse="lse+0", delta="ws+0", dQ="dQ+0")]
    (p,) = blocks(case, "SelAttnBwdParams")
    assert has(p, ranges=roff, O="O+0", lse="lse+0", dO="dO+0", dQ="dQ+0", dK="dK+0", dV="dV+0", R=256, n=1, S_kv=13, skip_delta_dq=1, scale=0.125)
    for label in ("band_attn_bwd/generic_fallback", "band_attn_bwd/f32_fallback"):
        names, (p,) = attn(routes, label, "SelAttnBwdParams")  # one range per row, the ranges in the workspace, dK / dV zeroed by the host
        assert names == ["band_ranges", "sel_attn_bwd_generic"] and routes[label]["memsets"] == 2, label
        assert has(p, ranges=routes[label]["args"][0]["ranges"], n=1, skip_delta_dq=0, dK="dK+0", dV="dV+0") and p["ranges"].startswith("ws+"), label
    assert routes["band_attn_bwd/f32_fallback"]["args"][0]["ranges"] == "ws+0"  # no MFMA workspace in front of the ranges


def test_select_and_attend_fuses_only_without_key_split(routes):
    fused = routes["sel_select_attn_fwd/S512_SEL_FUSE_members"]
    assert launches(fused) == ["sel_attn_blocks_mfma"]
    (a,) = fused["args"]
    assert has(a["SelAttnParams"], fuse_select=1, select="set", ranges="ranges+0", n=16, R=1024, ks_ws="null", part="null") and a["cand"] == 1
    assert has(a["SelectParams"], p_grp="p_grp+0", out="ranges+0", R=1024, S=512, G=2, t0=0, S_sel=8, l_sel=64, n_top=16, force_init=1, force_local=2, W=16)
    two = routes["sel_select_attn_fwd/S512_two_launches_members"]
    assert launches(two) == ["select_topn", "sel_attn_blocks_mfma"]
    (sp,), (p,) = blocks(two, "SelectParams"), blocks(two, "SelAttnParams")  # the attention launch of the two carries an empty selector block
    assert sp["R"] == 0 and sp["out"] == "null" and two["args"][0]["cand"] == 0 and has(p, fuse_select=0, select="null", ks_ws="ws+0")
    assert {k: v for k, v in p.items() if k not in ("fuse_select", "select", "ks_ws", "ks_bytes")} == \
           {k: v for k, v in a["SelAttnParams"].items() if k not in ("fuse_select", "select", "ks_ws", "ks_bytes")}
    split = routes["sel_select_attn_fwd/S32768_SEL_FUSE_members"]  # the attention would split the keys over XCD groups: two launches
    assert launches(split) == ["select_topn", "sel_attn_blocks_mfma"]  # (S_kv = S: every row below 32768, no record to merge)
    assert has(blocks(split, "SelAttnParams")[0], fuse_select=0, part="ws+0", ks_ws="ws+0", ks_r1=32768)


def test_layer_calls_build_their_three_branches(routes):
    """nsa_layer_prefill / _extend / _decode_step / _decode_rows: K / V and strides of each branch, the band geometry, the scratch of each."""
    cache = dict(ksb=131072, ksg=65536, kss=64, vsb=131072, vsg=65536, vss=64)
    cmp_cache = dict(ksb=8064, ksg=4032, kss=64, vsb=8064, vsg=4032, vss=64)
    for label, S, t0, n_cmp in (("layer_prefill/S100_attention", 100, 0, 5), ("layer_extend/t100_S28_attention", 28, 100, 7)):
        case = routes[label]
        sel = blocks(case, "SelAttnParams")[0]
        assert has(sel, K="K_sel+0", V="V_sel+0", ranges="ranges+0", lse="null", S=S, S_kv=t0 + S, n=16, R=2 * S, **cache) and sel["part"].startswith("ws+"), label
        win, cmp_ = blocks(case, "BandAttnParams")
        assert has(win, K="K_win+0", V="V_win+0", Q=sel["Q"], S=S, S_kv=t0 + S, t0=t0, w=512, **SLIDING, **cache), label
        assert has(cmp_, K="K_cmp+0", V="V_cmp+0", Q=sel["Q"], S=S, S_kv=n_cmp, t0=t0, **COMPRESSED, **cmp_cache), label
        assert win["part"] == cmp_["part"] and len({sel["O"], win["O"], cmp_["O"]}) == 3, label  # one band scratch, used in turn
    fused = routes["layer_prefill/S512_SEL_FUSE_attention"]["args"][0]
    assert has(fused["SelAttnParams"], fuse_select=1, select="set", K="K_sel+0", S=512, S_kv=512, n=16) and fused["SelectParams"]["out"] == "ranges+0"
    # the single step: the band pair rides on the decode step's launch, merged in the workgroup
    (a,) = routes["layer_decode_step/t100_attention"]["args"]
    pair = a["DecBandPair"]
    assert has(a["DecAttnArgs"], K="K_sel+0", V="V_sel+0", S_kv=101, n=16, **cache) and (pair["mg_on"], pair["n_sel"], pair["n_w"]) == (1, 2, 2)
    assert has(pair["w"], K="K_win+0", V="V_win+0", S=1, S_kv=101, t0=100, w=512, nsplit=16, defer_combine=1, **SLIDING, **cache)
    assert has(pair["c"], K="K_cmp+0", V="V_cmp+0", S=1, S_kv=5, t0=100, nsplit=16, defer_combine=1, **COMPRESSED, **cmp_cache)
    assert pair["w"]["part"] != pair["c"]["part"] and pair["w"]["O"] != pair["c"]["O"] and pair["w"]["Q"] == pair["c"]["Q"] == a["DecAttnArgs"]["Q"]
    # its separate launches: the decode workgroup (or the deferred split) and the dual band launch with the same two blocks
    wg = routes["layer_decode_step/t100_DECODE_STEP_0_attention"]
    assert launches(wg) == ["qkv_rope_append(fast)", "decode_score_select", "sel_attn_decode_wg", "band_attn_fwd_dual", "decode_finish", "linear_small(fast)"]
    dual = [x for x in wg["args"] if "BandAttnParams1" in x][0]
    assert dual["BandAttnParams"] == pair["w"] and dual["BandAttnParams1"] == pair["c"] and dual["grid0"] == 8
    split = routes["layer_decode_step/t100_DECODE_STEP_0_DECODE_WG_0_attention"]
    (p,) = blocks(split, "SelAttnParams")
    assert launches(split)[2:4] == ["sel_attn_fwd_mfma", "band_attn_fwd_dual"]  # no combine launch: the finish kernel merges
    assert has(p, K="K_sel+0", S=1, S_kv=101, nsplit=16, defer_combine=1) and p["part"].startswith("ws+")
    d128 = routes["layer_decode_step/D128_t100_DECODE_STEP_0_attention"]  # Dv = 128: no deferred combine, one band launch each
    assert launches(d128)[3:7] == ["band_attn_fwd(split)", "band_attn_combine", "band_attn_fwd(split)", "band_attn_combine"]
    win, cmp_ = blocks(d128, "BandAttnParams")
    assert has(win, K="K_win+0", Dk=128, defer_combine=0, **SLIDING) and has(cmp_, K="K_cmp+0", defer_combine=0, **COMPRESSED) and win["part"] != cmp_["part"]
    # S rows per sequence: the rows form's attention block, and the same band pair at S = 4
    rows = routes["layer_decode_rows/t100_S4_attention"]
    assert launches(rows) == ["qkv_rope_append(rows, mfma)", "decode_rows", "band_attn_fwd_dual", "decode_finish", "linear_small(mfma)"]
    assert has(rows["args"][0]["DecAttnArgs"], K="K_sel+0", V="V_sel+0", S_kv=104, n=16, **cache) and rows["args"][0]["DecBandPair"]["n_sel"] == 0xFFFFFFFF
    dual = rows["args"][1]
    assert has(dual["BandAttnParams"], K="K_win+0", S=4, S_kv=104, t0=100, w=512, defer_combine=1, **SLIDING)
    assert has(dual["BandAttnParams1"], K="K_cmp+0", S=4, S_kv=5, t0=100, defer_combine=1, **COMPRESSED)
    for label in ("layer_decode_rows/t100_S4_DECODE_ROWS_0_attention", "layer_decode_rows/t100_S4_DECODE_STEP_0_DECODE_WG_0_attention"):
        (p, c) = blocks(routes[label], "SelAttnParams")  # the separate launches of the rows call: the attention with its own combine
        assert p == c and has(p, K="K_sel+0", S=4, S_kv=104, R=8, n=16, defer_combine=0) and p["nsplit"] > 1, label
