"""Host side of the paged band forward (no GPU): nsa_band_attn_fwd_paged, its workspace query and the block_table= keyword of the Python
operators.

`dispatch_check <library> band_paged` (csrc/dispatch_check.cpp: the library's host code against a HIP runtime that counts and refuses every
launch) walks the call's routes on real pointers; this file asserts them: launches and geometry equal to the `ragged` mode's band cases at
the same (B, S, G, h, D) -- the paged form adds no LDS --; the table pointer, its stride, n_pages and the page shift in an argument block
of their own, the page strides and the capacity in BandAttnParams, as given; a page stride of 3 GiB accepted; every decline with its
message and no launch.  The default output of dispatch_check is what tests/test_dispatch_host.py compares with its recorded file: these
cases are not in it.

The Python operators refuse a bad block table, CPU tensors, a missing t_max and inputs that require grad before any native call."""
import json
import os
import subprocess

import pytest
import torch

from conftest import ROOT

INVALID = -1  # NSA_ERR_INVALID
P = "band_attn_fwd_paged/"


def _routes(mode):
    from nsa_vibe_amd import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    r = subprocess.run([os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH, mode], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def routes():
    return _routes("band_paged")


@pytest.fixture(scope="module")
def ragged_routes():
    return _routes("ragged")


def test_only_the_band_paged_cases(routes):
    assert routes and all(k.startswith(P) for k in routes)


SAME_AS_RAGGED = ["sliding_B5_S1_split", "sliding_B5_S1_no_workspace", "compressed_B5_S3_split", "sliding_B600_S3_unsplit"]


@pytest.mark.parametrize("case", SAME_AS_RAGGED)
def test_launches_and_geometry_are_the_ragged_calls(routes, ragged_routes, case):
    """the same launchers in the same order with the same grid, block and LDS bytes (the paged form adds no LDS), the same split count,
    tokens per wave and workgroup map; the positions ride along as in the ragged call"""
    p, r = routes[P + case], ragged_routes["band_attn_fwd_ragged/" + case]
    assert (p["rc"], p["error"]) == (0, "") and (r["rc"], r["error"]) == (0, "")
    assert p["launches"] == r["launches"] and p["launches"]
    assert p["geometry"] == r["geometry"] and p["memsets"] == r["memsets"] == 0
    bp, br = p["args"][0]["BandAttnParams"], r["args"][0]["BandAttnParams"]
    for k in ("Q", "O", "lse", "B", "S", "G", "h", "Dk", "Dv", "scale", "t0", "a", "dd", "c", "w", "part", "nsplit", "map_mode", "tpw", "defer_combine"):
        assert bp[k] == br[k], k
    pp, rp = routes[P + case + "_positions"], ragged_routes["band_attn_fwd_ragged/" + case + "_positions"]
    for k in ("t_pos", "t_max", "t0", "nsplit", "workspace"):
        assert pp[k] == rp[k], k
    assert pp["workspace"] == pp["scalar_workspace"]


# case -> launchers, nsplit, tokens per wave, page rows, max_pages (what t_max needs), capacity
FORMS = [("sliding_B5_S1_split", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 2, 1024, 5),
         ("sliding_B5_S1_no_workspace", ["band_attn_fwd launch"], 1, 2, 1024, 5),
         ("compressed_B5_S3_split", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 2, 64, 5),
         ("sliding_B600_S3_unsplit", ["band_attn_fwd launch"], 1, 2, 1024, 1),
         ("sliding_B600_S256_nt3", ["band_attn_fwd launch"], 1, 8, 1024, 2),
         ("sliding_D128_B5_S1_split", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 2, 1024, 5),
         ("sliding_page_rows32", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 2, 32, 129),
         ("sliding_page_rows65536", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 2, 65536, 1),
         ("k_page_stride_3GiB", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 2, 1024, 5),
         ("max_pages_2pow20", ["band_attn_fwd(split) launch", "band_attn_combine launch"], 16, 2, 1024, 1 << 20)]


@pytest.mark.parametrize("case,launches,nsplit,tpw,rows,max_pages", FORMS)
def test_table_arguments_arrive_as_given(routes, case, launches, nsplit, tpw, rows, max_pages):
    """the form (split / unsplit NT = 1 / unsplit NT = 3 by the tokens per wave) planned from (B, S, G, h, D) alone; the table pointer, its
    stride, n_pages and log2(page_rows) in the second argument block; the page strides where the batch strides were, 64-bit end to end; the
    capacity max_pages * page_rows (bounded by the largest 32-bit position) in S_kv"""
    c = routes[P + case]
    assert (c["rc"], c["error"], c["memsets"]) == (0, "", 0)
    assert c["launches"] == launches
    a = c["args"][0]
    bp, pt = a["BandAttnParams"], a["BandPageTable"]
    assert (bp["nsplit"], bp["tpw"]) == (nsplit, tpw)
    assert pt == {"table": "table+28", "stride": max_pages if case == "max_pages_2pow20" else max_pages + 3, "n_pages": 40, "shift": rows.bit_length() - 1}
    D = bp["Dk"]
    k_page = 3 << 29 if case == "k_page_stride_3GiB" else 2 * rows * D
    assert (bp["K"], bp["V"]) == ("K_pool+0", "V_pool+0")
    assert (bp["ksb"], bp["ksg"], bp["kss"], bp["vsb"], bp["vsg"], bp["vss"]) == (k_page, rows * D, D, 2 * rows * D, rows * D, D)
    assert bp["S_kv"] == min(max_pages * rows, 2 ** 31 - 1)
    lds = int(c["geometry"][0].split("/")[2])
    assert lds == 4 * 2 * 32 * D * 2  # four waves, a K and a V tile of 32 rows each: the ragged form's, nothing added
    pos = routes[P + case + "_positions"]
    assert (pos["t_pos"], pos["nsplit"]) == ("t_pos+20", nsplit) and pos["workspace"] == pos["scalar_workspace"]


DECLINED = {
    "f32_declined": "the MFMA kernels only -- bf16 / f16, Dk = Dv in {64, 128}, h <= 16 (got dtype 0, Dk = 64, Dv = 64, h = 6)",
    "Dk_ne_Dv_declined": "the MFMA kernels only -- bf16 / f16, Dk = Dv in {64, 128}, h <= 16 (got dtype 1, Dk = 64, Dv = 128, h = 6)",
    "D96_declined": "(got dtype 1, Dk = 96, Dv = 96, h = 6)",
    "h17_declined": "(got dtype 1, Dk = 64, Dv = 64, h = 17)",
    "w_below_1_declined": "w = -1, the window must hold at least one key (w >= 1)",
    "null_table": "null block table",
    "null_t_pos": "null pointer",
    "max_pages_minus1": "max_pages = -1, must be in [1, 2^20]",
    "max_pages_above_2pow20": "max_pages = 1048577, must be in [1, 2^20]",
    "n_pages0": "n_pages = 0, the pools must hold at least one page",
    "table_stride_below_max_pages": "row stride of at least max_pages = 5 (got 4)",
    "page_rows16_declined": "page_rows = 16 is not built: a power of two in [32, 65536]",
    "page_rows96_declined": "page_rows = 96 is not built: a power of two in [32, 65536]",
    "page_rows131072_declined": "page_rows = 131072 is not built: a power of two in [32, 65536]",
    "K_pool_2_bytes_off": "16-byte aligned",
    "O_4_bytes_off": "O 8-byte aligned",
    "k_page_stride_not_8": "strides in multiples of 8 elements",
    "k_row_stride_2MiB_plane_limit": "outside the 32-bit offsets of one (page, group) plane (page_rows = 1024 rows: under 2 GiB)",
}


@pytest.mark.parametrize("case", sorted(DECLINED))
def test_declines_name_their_limit(routes, case):
    """NSA_ERR_INVALID with the limit in the message, no launch, no memset: there is no fallback"""
    c = routes[P + case]
    assert c["rc"] == INVALID and c["launches"] == [] and c["memsets"] == 0 and c["args"] == []
    assert c["error"].startswith("band_attn_fwd_paged: ") and DECLINED[case] in c["error"], c["error"]


def test_every_case_is_asserted(routes):
    seen = {P + c for c in DECLINED} | {P + f[0] for f in FORMS}
    assert {k for k in routes if not k.endswith("_positions")} == seen


@pytest.mark.parametrize("shape", [(5, 1, 2, 6, 64), (5, 3, 2, 6, 128), (32, 32, 2, 6, 64), (32, 256, 2, 6, 64), (600, 3, 2, 6, 64), (1, 1, 1, 16, 128)])
def test_workspace_query_is_the_scalar_calls(shape):
    from nsa_vibe_amd import _lib

    L = _lib.lib()
    B, S, G, h, D = shape
    for dt in (_lib.NSA_DT_BF16, _lib.NSA_DT_F16, _lib.NSA_DT_F32):
        assert L.nsa_band_attn_fwd_paged_workspace(B, S, G, h, D, D, dt) == L.nsa_band_attn_fwd_workspace(B, S, G, h, D, D, dt)
    assert (L.nsa_band_attn_fwd_paged_workspace(5, 1, 2, 6, 64, 64, _lib.NSA_DT_BF16) > 0) and L.nsa_band_attn_fwd_paged_workspace(32, 256, 2, 6, 64, 64, _lib.NSA_DT_BF16) == 0


# ---- the Python operators: refusals before any native call (CPU and meta tensors only here; a meta tensor stands in for a device tensor on
# a machine without one: it is never read)

@pytest.mark.parametrize("op", ["band", "sliding", "compressed"])
def test_block_table_refusals(op):
    import nsa_vibe_amd as nv

    B = 3
    Q = torch.zeros(B, 1, 2, 6, 64, dtype=torch.bfloat16)
    K = torch.zeros(4, 2, 64, 64, dtype=torch.bfloat16)
    table = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device="meta")  # noqa: E731
    pos = [100, 40, -1]

    def call(bt, t_pos=pos, Qx=Q, Kx=K, **kw):
        if op == "band":
            return nv.band_attention_hip(Qx, Kx, Kx, w=512, t_pos=t_pos, block_table=bt, **kw)
        if op == "sliding":
            return nv.sliding_window_attention(Qx, Kx, Kx, 512, t_pos=t_pos, block_table=bt, **kw)
        return nv.batched_causal_attention_compressed(Qx, Kx, Kx, 32, 16, t_pos=t_pos, block_table=bt, **kw)

    for bad in (table(B, 2, dtype=torch.int64), torch.zeros(B, 2, dtype=torch.int32), [[0, 1]] * B, table(B * 2)):
        with pytest.raises(RuntimeError, match="block_table must be a device int32 tensor"):
            call(bad)
    with pytest.raises(RuntimeError, match=r"shape \(4, 2\) for B = 3"):
        call(table(4, 2))
    with pytest.raises(RuntimeError, match="contiguous last dimension"):
        call(table(B, 4)[:, ::2])
    with pytest.raises(RuntimeError, match="block_table needs the per-sequence positions"):
        call(table(B, 2), t_pos=None)
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        call(table(B, 2), t0=5)
    with pytest.raises(RuntimeError, match="t_max .* is required with device positions"):
        call(table(B, 2), t_pos=torch.empty(B, dtype=torch.int32, device="meta"))
    with pytest.raises(RuntimeError, match="contiguous int32 tensor"):
        call(table(B, 2), t_pos=torch.empty(B, dtype=torch.int64, device="meta"), t_max=100)
    with pytest.raises(RuntimeError, match="4 entries for B = 3"):
        call(table(B, 2), t_pos=pos + [7])
    with pytest.raises(RuntimeError, match="t_max must be in"):
        call(table(B, 2), t_max=-1)
    with pytest.raises(RuntimeError, match="forward only: no input may require grad"):
        call(table(B, 2), Qx=torch.zeros(B, 1, 2, 6, 64, requires_grad=True))
    with pytest.raises(RuntimeError, match="forward only: no input may require grad"):
        call(table(B, 2), Kx=torch.zeros(4, 2, 64, 64, requires_grad=True))
    with pytest.raises(RuntimeError, match="need HIP device tensors"):
        call(table(B, 2))


def test_calls_without_block_table_are_untouched():
    """the ragged refusals keep their wording: the keyword defaults to None and the contiguous path is the one it was"""
    import nsa_vibe_amd as nv

    Q = torch.zeros(3, 1, 2, 6, 64, dtype=torch.bfloat16)
    K = torch.zeros(3, 2, 128, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="band attention: t_max is the bound of t_pos and needs it"):
        nv.sliding_window_attention(Q, K, K, 512, t_max=100)
    with pytest.raises(RuntimeError, match="need HIP device tensors"):
        nv.sliding_window_attention(Q, K, K, 512, t_pos=[100, 40, -1])
