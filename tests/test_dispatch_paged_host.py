"""Host side of the paged decode step of the selected branch (no GPU): nsa_sel_decode_paged, its plan query and its Python operator.

`dispatch_check <library> paged` (csrc/dispatch_check.cpp: the library's host code against a HIP runtime that counts and refuses every
launch) walks the call's routes on real pointers; this file asserts them: one launch with one workgroup per row; the table pointer, its
stride, n_pages, the three page strides and t_max in the argument blocks as given; form and chunks planned from t_max alone, as the ragged
call plans them; the declines, each naming its limit; a page stride of 3 GiB accepted.  The default output of dispatch_check is what
tests/test_dispatch_host.py compares with its recorded file: these cases are not in it.

The Python operator refuses a bad block table, CPU tensors and a missing t_max before any native call."""
import json
import os
import subprocess

import pytest
import torch

from conftest import ROOT

INVALID = -1  # NSA_ERR_INVALID


def _routes(mode):
    from nsa_vibe_amd import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    r = subprocess.run([os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH, mode], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def routes():
    return _routes("paged")


@pytest.fixture(scope="module")
def ragged_routes():
    return _routes("ragged")


def test_only_the_paged_cases(routes):
    assert routes and all(k.startswith("sel_decode_paged/") for k in routes)


# case -> R = B S G, S, form, nchunk, t_max, max_pages
ONE_LAUNCH = [("t_max100", 6, 1, 0, 1, 100, 1), ("t_max100_S4", 24, 4, 0, 1, 100, 1), ("t_max20_no_compressed_token", 6, 1, 0, 0, 20, 1),
              ("t_max5000_max_pages9", 6, 1, 0, 5, 5000, 9), ("t_max40000_form1", 2, 1, 1, 40, 40000, 40), ("k_page_stride_3GiB", 6, 1, 0, 1, 100, 1)]


@pytest.mark.parametrize("case,R,S,form,nchunk,t_max,max_pages", ONE_LAUNCH)
def test_one_launch_with_the_table_in_the_argument_block(routes, case, R, S, form, nchunk, t_max, max_pages):
    """ONE launch of the paged instantiation: R = B S G workgroups of 16 waves, no memset, no scratch; the table pointer, its stride,
    n_pages, the page strides of the three pools, the positions and t_max arrive in the argument blocks as given; the capacity the kernel
    bounds positions with is max_pages * 1024"""
    c = routes["sel_decode_paged/" + case]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"] == ["decode_paged launch"]
    (geom,) = c["geometry"]
    grid, block, lds = geom.split("/")
    assert grid == f"{R},1,1" and block == "1024,1,1" and 0 < int(lds) <= 160 * 1024
    assert c["plan"] == {"rc": 0, "launches": 1, "form": form}
    s = c["step"]
    assert (s["R"], s["S"], s["G"], s["NS"], s["nchunk"], s["t_max"]) == (R, S, 2, 1, nchunk, t_max)
    assert s["block_table"] == "table+28" and s["t_pos"] == "t_pos+20"  # the pointers as given: seven / five int32 into their buffers
    assert (s["bt_stride"], s["n_pages"], s["capacity"]) == (max_pages + 3, 40, max_pages * 1024)
    assert (s["Q"], s["Kc"], s["K"], s["V"]) == ("Q+0", "Kc_pool+0", "K_pool+0", "V_pool+0")
    k_page = 3 << 29 if case == "k_page_stride_3GiB" else 2 * 1024 * 64  # elements; 64-bit end to end
    assert (s["kc_page_stride"], s["k_page_stride"], s["v_page_stride"]) == (2 * 64 * 64, k_page, 2 * 1024 * 64)


@pytest.mark.parametrize("case", ["t_max100", "t_max100_S4", "t_max20_no_compressed_token", "t_max40000_form1"])
def test_planned_from_t_max_like_the_ragged_call(routes, ragged_routes, case):
    """form, chunks, grid, block and the metadata bounds are those of nsa_sel_decode_ragged at the same t_max and row count; the paged
    launch asks for 512 bytes of LDS more (the sequence's table entries)"""
    p, r = routes["sel_decode_paged/" + case], ragged_routes["sel_decode_ragged/" + case]
    assert p["plan"] == r["plan"]
    for k in ("R", "G", "h", "S", "S_cmp", "S_sel", "NS", "nchunk", "t_max", "t_pos"):
        assert p["step"][k] == r["step"][k], k
    (gp,), (gr,) = p["geometry"], r["geometry"]
    assert gp.split("/")[:2] == gr.split("/")[:2]
    assert int(gp.split("/")[2]) == int(gr.split("/")[2]) + 512


DECLINED_SHAPES = {
    "D128_t_max20000_declined": "t_max is beyond the unsplit form at D = 128: more than 16 chunks",
    "t_max70000_declined": "t_max is beyond the unsplit forms at 16 waves per row: more than 64 chunks",
    "B200_t_max40000_declined": "t_max is beyond the unsplit forms at 8 waves per row (more than 256 rows): more than 32 chunks",
    "f32_declined": "needs bf16 / f16",
    "S17_declined": "1 <= S <= 16",
    "DECODE_STEP_0_declined": "switched off (DECODE_STEP = 0 or DECODE_UNFUSED = 1)",
    "page_tokens64_declined": "page_tokens = 64 is not built: pages of 1024 tokens only",
}


@pytest.mark.parametrize("case", sorted(DECLINED_SHAPES))
def test_declined_shapes_name_their_limit(routes, ragged_routes, case):
    """NSA_ERR_INVALID with the limit in the message and no launch; the plan query says launches 0, form -1 with status NSA_OK.  The
    shape declines carry the ragged call's message word for word"""
    c = routes["sel_decode_paged/" + case]
    assert c["rc"] == INVALID and c["launches"] == [] and c["memsets"] == 0 and c["step"] is None
    assert c["error"].startswith("decode_paged: ") and DECLINED_SHAPES[case] in c["error"], c["error"]
    assert c["plan"] == {"rc": 0, "launches": 0, "form": -1}
    if case != "page_tokens64_declined":
        assert c["error"] == ragged_routes["sel_decode_ragged/" + case]["error"].replace("decode_ragged: ", "decode_paged: ")


DECLINED_OPERANDS = {
    "null_table": "null block table",
    "max_pages_minus1": "max_pages = -1, must be in [1, 2^20]",
    "n_pages0": "n_pages = 0, the pools must hold at least one page",
    "table_stride_below_max_pages": "row stride of at least max_pages = 5 (got 4)",
    "K_pool_2_bytes_off": "16-byte aligned",
    "k_page_stride_not_8": "strides in multiples of 8 elements",
    "null_t_pos": "null pointer",
    "k_row_stride_2MiB": "outside the 32-bit offsets of one (page, group) plane",
}


@pytest.mark.parametrize("case", sorted(DECLINED_OPERANDS))
def test_declined_operands_name_their_limit(routes, case):
    c = routes["sel_decode_paged/" + case]
    assert c["rc"] == INVALID and c["launches"] == [] and c["memsets"] == 0
    assert c["error"].startswith("decode_paged: ") and DECLINED_OPERANDS[case] in c["error"], c["error"]
    if case in ("null_table", "n_pages0", "table_stride_below_max_pages", "K_pool_2_bytes_off", "k_page_stride_not_8", "null_t_pos"):
        assert c["plan"]["launches"] == 1  # (the plan query sees shapes only)


def test_workspace_query():
    from nsa_vibe_amd import _lib

    assert _lib.lib().nsa_sel_decode_paged_workspace(5, 3, 2, 6, 64, 64, 65, 17, 16, _lib.NSA_DT_BF16) == 0


def test_plan_operator_declines_other_page_sizes():
    import nsa_vibe_amd as nv

    assert nv.selection_decode_paged_plan(3, 1, 2, 6, 64, 64, 5, 2, 1, 16, 100) == {"launches": 1, "form": 0}
    assert nv.selection_decode_paged_plan(3, 1, 2, 6, 64, 64, 5, 2, 16, 16, 100, page_tokens=64) == {"launches": 0, "form": -1}
    assert nv.selection_decode_paged_plan(1, 1, 2, 6, 64, 64, 2499, 626, 40, 16, 40000) == {"launches": 1, "form": 1}


# ---- the Python operator: refusals before any native call (CPU and meta tensors only here; a meta tensor stands in for a device tensor on
# a machine without one: it is never read)

def test_selection_decode_paged_refusals():
    import nsa_vibe_amd as nv

    B, t = 3, 100
    m = nv.build_block_meta(t + 1, 32, 16, 64, 16, 512)
    Q = torch.zeros(B, 1, 2, 6, 64, dtype=torch.bfloat16)
    Kc = torch.zeros(4, 2, 64, 64, dtype=torch.bfloat16)
    K = torch.zeros(4, 2, 1024, 64, dtype=torch.bfloat16)
    table = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device="meta")  # noqa: E731
    pos = [100, 40, -1]
    with pytest.raises(RuntimeError, match="block_table must be a device int32 tensor"):
        nv.selection_decode_paged(Q, Kc, K, K, table(B, 2, dtype=torch.int64), m, 16, pos)
    with pytest.raises(RuntimeError, match="block_table must be a device int32 tensor"):
        nv.selection_decode_paged(Q, Kc, K, K, torch.zeros(B, 2, dtype=torch.int32), m, 16, pos)  # host memory
    with pytest.raises(RuntimeError, match="block_table must be a device int32 tensor"):
        nv.selection_decode_paged(Q, Kc, K, K, [[0, 1]] * B, m, 16, pos)
    with pytest.raises(RuntimeError, match="block_table must be a device int32 tensor"):
        nv.selection_decode_paged(Q, Kc, K, K, table(B * 2), m, 16, pos)
    with pytest.raises(RuntimeError, match=r"shape \(4, 2\) for B = 3"):
        nv.selection_decode_paged(Q, Kc, K, K, table(4, 2), m, 16, pos)
    with pytest.raises(RuntimeError, match="contiguous last dimension"):
        nv.selection_decode_paged(Q, Kc, K, K, table(B, 4)[:, ::2], m, 16, pos)
    with pytest.raises(RuntimeError, match="t_max .* is required with device positions"):
        nv.selection_decode_paged(Q, Kc, K, K, table(B, 2), m, 16, torch.empty(B, dtype=torch.int32, device="meta"))
    with pytest.raises(RuntimeError, match="contiguous int32 tensor"):
        nv.selection_decode_paged(Q, Kc, K, K, table(B, 2), m, 16, torch.empty(B, dtype=torch.int64, device="meta"), t_max=100)
    with pytest.raises(RuntimeError, match="4 entries for B = 3"):
        nv.selection_decode_paged(Q, Kc, K, K, table(B, 2), m, 16, pos + [7])
    with pytest.raises(RuntimeError, match="t_max must be in"):
        nv.selection_decode_paged(Q, Kc, K, K, table(B, 2), m, 16, pos, t_max=-1)
    with pytest.raises(RuntimeError, match="need HIP device tensors"):
        nv.selection_decode_paged(Q, Kc, K, K, table(B, 2), m, 16, pos)
