"""Host side of the band forward family (no GPU): the five forms behind one host path -- nsa_band_attn_fwd, _ragged, _paged, _ragged_fp8 and
_paged_fp8 -- reproduce a recording made before they were folded onto it.

`dispatch_check <library> band_fp8` (csrc/dispatch_check.cpp: the library's host code against a HIP runtime that counts and refuses every
launch) walks the two FP8 entry points on real pointers: the three forms of the plan at both head dimensions, the page geometries, and every
decline the C ABI can reach, alone and two at a time.  tests/golden/dispatch_band_family.json holds that output together with the band
entries of the `ragged`, `band_paged` and default modes, all four recorded with this probe from the library of the commit before the fold.
The product must give the same: launch names in order, grid, block, LDS bytes, memsets, every member of every argument block, status and
message.  The LDS bytes of the FP8 launches are asserted from the kernels' layout, not read back."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

MODES = {"band_fp8": "band_fp8", "ragged": "ragged", "band_paged": "band_paged", "default": None}
FORMS = ["ragged", "paged"]


def _routes(mode):
    from nsa_vibe_amd import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    cmd = [os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH] + ([mode] if mode else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_band_family.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def routes():
    return {name: _routes(mode) for name, mode in MODES.items()}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_band_entries_reproduce_the_recording(routes, recorded, mode):
    now = {k: v for k, v in routes[mode].items() if "band" in k}
    want = recorded[mode]
    assert list(now) == list(want)
    for k in want:
        assert now[k] == want[k], k


def test_only_the_fp8_band_cases(routes):
    assert routes["band_fp8"] and all(k.startswith(("band_attn_fwd_ragged_fp8/", "band_attn_fwd_paged_fp8/")) for k in routes["band_fp8"])


# case -> launchers, D, nsplit, tokens per wave
SPLIT, UNSPLIT = ["band_attn_fwd_fp8(split) launch", "band_attn_combine launch"], ["band_attn_fwd_fp8 launch"]
RUNS = [("sliding_B5_S1_split", SPLIT, 64, 16, 2), ("compressed_B5_S3_split", SPLIT, 64, 16, 2), ("sliding_B600_S3_unsplit", UNSPLIT, 64, 1, 2),
        ("sliding_B600_S256_nt3", UNSPLIT, 64, 1, 8), ("sliding_D128_B5_S1_split", SPLIT, 128, 16, 2), ("sliding_D128_B600_S256_nt2", UNSPLIT, 128, 1, 5),
        ("unsplit_needs_no_workspace", UNSPLIT, 64, 1, 2)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case,launches,D,nsplit,tpw", RUNS)
def test_fp8_launches_and_lds(routes, form, case, launches, D, nsplit, tpw):
    """the plan's three forms; four waves with two stages of (32 rows of D bytes + 32 fp32 scales for K and V each): 4 * 2 * (32 D + 256) bytes
    of LDS, no LDS in the combine pass; positions, scales and (paged) the table in their blocks as given"""
    c = routes["band_fp8"][f"band_attn_fwd_{form}_fp8/{case}"]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"] == launches
    lds = [int(g.split("/")[2]) for g in c["geometry"]]
    assert lds[0] == 4 * 2 * (32 * D + 256) == {64: 18432, 128: 34816}[D] and lds[1:] == [0] * (len(launches) - 1)
    assert all(g.split("/")[1] == "256,1,1" for g in c["geometry"])
    a = c["args"][0]
    bp, z, pt = a["BandAttnParams"], a["BandFp8Scales"], a["BandPageTable"]
    assert (bp["nsplit"], bp["tpw"], bp["Dk"], bp["Dv"], bp["kss"], bp["vss"]) == (nsplit, tpw, D, D, D, D)
    assert (bp["K"], bp["V"], bp["t_pos"], z["k_scale"], z["v_scale"]) == ("K8+0", "V8+0", "t_pos+20", "k_scale+12", "v_scale+36")
    assert (bp["part"] == "ws+0") == (nsplit > 1)
    assert (pt["table"], pt["shift"] > 0) == (("table+28", True) if form == "paged" else ("null", False))
    if nsplit > 1:
        comb = c["args"][1]["SelAttnParams"]
        assert (comb["O"], comb["lse"], comb["part"], comb["nsplit"], comb["h"]) == (bp["O"], bp["lse"], "ws+0", nsplit, bp["h"])
        assert comb["R"] == bp["B"] * bp["S"] * bp["G"]


@pytest.mark.parametrize("case,rows,max_pages,k_page", [("sliding_page_rows32", 32, 129, 2 * 32 * 64), ("sliding_page_rows65536", 65536, 1, 2 * 65536 * 64),
                                                        ("k_page_stride_3GiB", 1024, 5, 3 << 30), ("max_pages_2pow20", 1024, 1 << 20, 2 * 1024 * 64)])
def test_fp8_page_geometry_arrives_as_given(routes, case, rows, max_pages, k_page):
    c = routes["band_fp8"]["band_attn_fwd_paged_fp8/" + case]
    assert (c["rc"], c["error"], c["launches"]) == (0, "", SPLIT)
    bp, pt = c["args"][0]["BandAttnParams"], c["args"][0]["BandPageTable"]
    assert pt == {"table": "table+28", "stride": max_pages if case == "max_pages_2pow20" else max_pages + 3, "n_pages": 40, "shift": rows.bit_length() - 1}
    assert (bp["ksb"], bp["ksg"], bp["vsb"], bp["vsg"]) == (k_page, rows * 64, 2 * rows * 64, rows * 64)
    assert bp["S_kv"] == min(max_pages * rows, 2 ** 31 - 1)


BOTH = {
    "dtype7_declined": "unknown dtype 7", "B_minus1": "negative size", "dd_below_1": "need dd >= 1, t_max >= 0", "t_max_minus1": "need dd >= 1, t_max >= 0",
    "f16_declined": "bf16 queries only (got dtype 2)", "f32_declined": "bf16 queries only (got dtype 0)", "Dk_ne_Dv_declined": "(got Dk = 64, Dv = 128, h = 6)",
    "D96_declined": "(got Dk = 96, Dv = 96, h = 6)", "h17_declined": "(got Dk = 64, Dv = 64, h = 17)", "w0_declined": "w = 0, the window must hold at least one key",
    "null_Q": "null pointer", "null_t_pos": "null pointer", "null_k_scale": "null scale", "null_v_scale": "null scale",
    "k_scale_2_bytes_off": "t_pos and the scales must be 4-byte aligned", "t_pos_2_bytes_off": "t_pos and the scales must be 4-byte aligned",
    "k_row_stride_not_D": "row stride 128 / 64 bytes, must be D = 64", "K8_8_bytes_off": "must be 16-byte aligned", "O_4_bytes_off": "O 8-byte aligned",
    "k_plane_stride_not_16": "strides in multiples of 16 bytes", "no_workspace": "workspace missing, misaligned or too small: the plan splits a row over 16 waves",
    "workspace_64_bytes": "needs 261120 bytes", "workspace_8_bytes_off": "workspace missing, misaligned or too small",
    # two limits in one call: the first check's message
    "f16_and_w0": "bf16 queries only", "D96_and_f32": "bf16 queries only", "null_k_scale_and_k_row_stride_not_D": "null scale",
    "null_t_pos_and_null_v_scale": "null pointer", "K8_8_bytes_off_and_no_workspace": "must be 16-byte aligned", "B0_and_w0": "w = 0",
}
RAGGED_ONLY = {"S_kv0_declined": "S_kv = 0, the caches must hold at least one row", "S_kv0_and_null_t_pos": "S_kv = 0",
               "S_kv_2pow25_plane_limit": "S_kv = 33554432 rows of 64 bytes leave the 32-bit offsets of one (b, g) plane",
               "S_kv_2pow25_and_no_workspace": "leave the 32-bit offsets"}
PAGED_ONLY = {"page_rows16_declined": "page_rows = 16 is not built", "page_rows96_declined": "page_rows = 96 is not built",
              "page_rows131072_declined": "page_rows = 131072 is not built", "max_pages_minus1": "max_pages = -1, must be in [1, 2^20]",
              "max_pages_above_2pow20": "max_pages = 1048577, must be in [1, 2^20]", "n_pages0": "n_pages = 0", "null_table": "null block table",
              "table_2_bytes_off": "the block table must be 4-byte aligned", "table_stride_below_max_pages": "row stride of at least max_pages = 5 (got 4)",
              "page_rows16_and_n_pages0": "page_rows = 16 is not built", "w0_and_page_rows96": "w = 0", "null_table_and_null_Q": "null block table",
              "B0_and_n_pages0": "n_pages = 0"}
DECLINED = [("ragged", k, v) for k, v in {**BOTH, **RAGGED_ONLY}.items()] + [("paged", k, v) for k, v in {**BOTH, **PAGED_ONLY}.items()]
NO_ROWS = [("ragged", "B0_no_launch"), ("paged", "B0_no_launch"), ("paged", "B0_and_null_table")]


@pytest.mark.parametrize("form,case,limit", DECLINED)
def test_fp8_declines_name_their_limit(routes, form, case, limit):
    """NSA_ERR_INVALID with the entry point's name and the limit in the message, no launch, no memset: there is no fallback"""
    c = routes["band_fp8"][f"band_attn_fwd_{form}_fp8/{case}"]
    assert c["rc"] == -1 and c["launches"] == [] and c["memsets"] == 0 and c["args"] == []
    assert c["error"].startswith(f"band_attn_fwd_{form}_fp8: ") and limit in c["error"], c["error"]


def test_fp8_every_case_is_asserted(routes):
    """(a call without rows returns before anything is dereferenced; the largest plane under the 32-bit bound runs)"""
    for form, case in NO_ROWS + [("ragged", "S_kv_2pow25_minus1")]:
        c = routes["band_fp8"][f"band_attn_fwd_{form}_fp8/{case}"]
        assert (c["rc"], c["error"]) == (0, "") and c["launches"] == ([] if case.startswith("B0") else SPLIT)
    seen = {f"band_attn_fwd_{f}_fp8/{c}" for f, c, _ in DECLINED} | {f"band_attn_fwd_{f}_fp8/{r[0]}" for f in FORMS for r in RUNS}
    seen |= {f"band_attn_fwd_{f}_fp8/{c}" for f, c in NO_ROWS} | {"band_attn_fwd_ragged_fp8/S_kv_2pow25_minus1"}
    seen |= {"band_attn_fwd_paged_fp8/" + c for c in ("sliding_page_rows32", "sliding_page_rows65536", "k_page_stride_3GiB", "max_pages_2pow20")}
    assert {k for k, v in routes["band_fp8"].items() if isinstance(v, dict)} == seen  # (the others: "<case>_workspace", the query's answer)
