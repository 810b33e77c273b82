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
