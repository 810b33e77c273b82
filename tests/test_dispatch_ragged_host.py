"""Host side of the ragged-batch entry points (no GPU): nsa_sel_decode_ragged, nsa_band_attn_fwd_ragged and their Python operators.

`dispatch_check <library> ragged` (csrc/dispatch_check.cpp: the library's host code against a HIP runtime that counts and refuses every
launch) walks their routes on real pointers; this file asserts them: one launch with one workgroup per row and the position pointer in
its argument block, planned from t_max alone; the declines, each naming its limit; and the band call's launches and split count.  The
default output of dispatch_check is what tests/test_dispatch_host.py compares with its recorded file: these cases are not in it.

The Python operators refuse CPU tensors, a bad t_pos and a missing t_max before any native call."""
import json
import os
import subprocess

import pytest
import torch

from conftest import ROOT

INVALID = -1  # NSA_ERR_INVALID


@pytest.fixture(scope="module")
def routes():
    from nsa_vibe_amd import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    r = subprocess.run([os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH, "ragged"], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_only_the_ragged_cases(routes):
    assert routes and all(k.startswith(("sel_decode_ragged/", "band_attn_fwd_ragged/")) for k in routes)


@pytest.mark.parametrize("case,R,S,form,nchunk", [("t_max100", 6, 1, 0, 1), ("t_max100_S4", 24, 4, 0, 1), ("t_max20_no_compressed_token", 6, 1, 0, 0),
                                                 ("t_max40000_form1", 2, 1, 1, 40), ("DECODE_ROWS_0_still_one_launch", 6, 1, 0, 1)])
def test_one_launch_with_the_position_pointer(routes, case, R, S, form, nchunk):
    """a ragged call is ONE launch of the rows form: R = B S G workgroups of 16 waves, the position array and t_max in the argument block,
    no memset, no scratch (the call passes a null workspace)"""
    c = routes["sel_decode_ragged/" + case]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"] == ["decode_rows launch"]
    (geom,) = c["geometry"]
    grid, block, lds = geom.split("/")
    assert grid == f"{R},1,1" and block == "1024,1,1" and int(lds) > 0
    assert c["plan"] == {"rc": 0, "launches": 1, "form": form}
    s = c["step"]
    assert s["t_pos"] == "t_pos+20"  # the pointer as given: five int32 into the buffer
    assert (s["R"], s["S"], s["G"], s["NS"], s["nchunk"]) == (R, S, 2, 1, nchunk)
    t_max = int(case.split("t_max")[1].split("_")[0]) if "t_max" in case else 100
    assert s["t_max"] == t_max
    assert (s["Q"], s["Kc"]) == ("Q+0", "K_cmp+0")


DECLINED = {
    "D128_t_max20000_declined": "t_max is beyond the unsplit form at D = 128: more than 16 chunks",
    "t_max70000_declined": "t_max is beyond the unsplit forms at 16 waves per row: more than 64 chunks",
    "B200_t_max40000_declined": "t_max is beyond the unsplit forms at 8 waves per row (more than 256 rows): more than 32 chunks",
    "f32_declined": "needs bf16 / f16",
    "S17_declined": "1 <= S <= 16",
    "DECODE_STEP_0_declined": "switched off (DECODE_STEP = 0 or DECODE_UNFUSED = 1)",
}


@pytest.mark.parametrize("case", sorted(DECLINED))
def test_declined_shapes_name_their_limit(routes, case):
    """no fallback exists (the separate launches take a scalar position): NSA_ERR_INVALID with the limit in the message, no launch, and
    the plan query says launches 0, form -1 with status NSA_OK"""
    c = routes["sel_decode_ragged/" + case]
    assert c["rc"] == INVALID and c["launches"] == [] and c["memsets"] == 0 and c["step"] is None
    assert c["error"].startswith("decode_ragged: ") and DECLINED[case] in c["error"], c["error"]
    assert c["plan"] == {"rc": 0, "launches": 0, "form": -1}


def test_unaligned_operand_and_null_positions(routes):
    c = routes["sel_decode_ragged/K_2_bytes_off"]
    assert c["rc"] == INVALID and c["launches"] == [] and "16-byte aligned" in c["error"]
    assert c["plan"]["launches"] == 1  # (the plan query sees shapes only)
    c = routes["sel_decode_ragged/null_t_pos"]
    assert c["rc"] == INVALID and c["launches"] == [] and c["error"] == "decode_ragged: null pointer"


@pytest.mark.parametrize("case,launches,nsplit,grid0", [
    ("sliding_B5_S1_split", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 40),      # 10 units x 16 splits, 4 waves a workgroup
    ("sliding_B5_S1_no_workspace", ["band_attn_fwd launch"], 1, 10),
    ("compressed_B5_S3_split", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 80),   # tpw = 2: two token groups per (b, g)
    ("sliding_B600_S3_unsplit", ["band_attn_fwd launch"], 1, 1200),
    ("sliding_f32_generic", ["band_attn_fwd_generic launch"], 0, 15)])
def test_band_call_is_planned_like_the_scalar_call(routes, case, launches, nsplit, grid0):
    """launches and split count follow from the row count (B, S, G, h, D), as for nsa_band_attn_fwd; the positions and t_max ride in the
    argument block and t0 is zero"""
    c = routes["band_attn_fwd_ragged/" + case]
    assert (c["rc"], c["error"]) == (0, "") and c["launches"] == launches
    assert c["geometry"][0].split("/")[0] == f"{grid0},1,1"
    (a,) = c["args"]
    P = a["BandAttnParams"]
    assert (P["t0"], P["nsplit"]) == (0, nsplit)
    assert P["part"] == ("ws+0" if nsplit > 1 else "null")
    p = routes["band_attn_fwd_ragged/" + case + "_positions"]
    assert p["t_pos"] == "t_pos+20" and p["t0"] == 0 and p["nsplit"] == nsplit
    assert p["t_max"] == {"sliding_B5_S1_split": 4100, "sliding_B5_S1_no_workspace": 4100, "compressed_B5_S3_split": 5002,
                          "sliding_B600_S3_unsplit": 1000, "sliding_f32_generic": 1000}[case]
    assert (p["workspace"] > 0) == (case in ("sliding_B5_S1_split", "sliding_B5_S1_no_workspace", "compressed_B5_S3_split"))


def test_scalar_workspace_query_is_the_ragged_one():
    from nsa_vibe_amd import _lib

    L = _lib.lib()
    for B, S in ((5, 1), (5, 3), (600, 3)):
        assert L.nsa_band_attn_fwd_ragged_workspace(B, S, 2, 6, 64, 64, _lib.NSA_DT_BF16) == L.nsa_band_attn_fwd_workspace(B, S, 2, 6, 64, 64, _lib.NSA_DT_BF16)
    assert L.nsa_sel_decode_ragged_workspace(5, 3, 2, 6, 64, 64, 65, 17, 16, _lib.NSA_DT_BF16) == 0


# ---- the Python operators: refusals before any native call (CPU tensors only here)

def _cpu_inputs(B=3, S=1, t=100):
    import nsa_vibe_amd as nv

    m = nv.build_block_meta(t + 1, 32, 16, 64, 16, 512)
    Q = torch.zeros(B, S, 2, 6, 64, dtype=torch.bfloat16)
    Kc = torch.zeros(B, 2, m.S_cmp, 64, dtype=torch.bfloat16)
    K = torch.zeros(B, 2, t + 1, 64, dtype=torch.bfloat16)
    return nv, m, Q, Kc, K


def test_selection_decode_ragged_refusals():
    nv, m, Q, Kc, K = _cpu_inputs()
    with pytest.raises(RuntimeError, match="need HIP device tensors"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, [100, 40, -1])
    with pytest.raises(RuntimeError, match="4 entries for B = 3"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, [100, 40, -1, 7])
    with pytest.raises(RuntimeError, match="must hold integers"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, [100.0, 40, -1])
    with pytest.raises(RuntimeError, match="must hold integers"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, torch.tensor([100.0, 40.0, -1.0]))
    with pytest.raises(RuntimeError, match="device int32 tensor"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, 100)
    with pytest.raises(RuntimeError, match="t_max must be in"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, [100, 40, -1], t_max=-1)
    # a tensor that is not in host memory is never read back: its dtype, its length and the bound are checked as given (a meta tensor stands
    # in for a device tensor on a machine without one)
    with pytest.raises(RuntimeError, match="t_max .* is required with device positions"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, torch.empty(3, dtype=torch.int32, device="meta"))
    with pytest.raises(RuntimeError, match="contiguous int32 tensor"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, torch.empty(3, dtype=torch.int64, device="meta"), t_max=100)
    with pytest.raises(RuntimeError, match="contiguous int32 tensor"):
        nv.selection_decode_ragged(Q, Kc, K, K, m, 16, torch.empty(4, dtype=torch.int32, device="meta"), t_max=100)


def test_band_operators_refusals():
    nv, m, Q, Kc, K = _cpu_inputs()
    for op in (lambda **kw: nv.sliding_window_attention(Q, K, K, 512, **kw), lambda **kw: nv.batched_causal_attention_compressed(Q, Kc, Kc, 32, 16, **kw),
               lambda **kw: nv.band_attention_hip(Q, K, K, w=512, **kw)):
        with pytest.raises(RuntimeError, match="need HIP device tensors"):
            op(t_pos=[100, 40, -1])
        with pytest.raises(RuntimeError, match="mutually exclusive"):
            op(t_pos=[100, 40, -1], t0=5)
        with pytest.raises(RuntimeError, match="2 entries for B = 3"):
            op(t_pos=[100, 40])
        with pytest.raises(RuntimeError, match="is required with device positions"):
            op(t_pos=torch.empty(3, dtype=torch.int32, device="meta"))
        with pytest.raises(RuntimeError, match="needs it"):
            op(t_max=100)
    Qg = Q.float().requires_grad_()
    with pytest.raises(RuntimeError, match="forward only"):
        nv.sliding_window_attention(Qg, K.float(), K.float(), 512, t_pos=[100, 40, -1])
