"""Host side of the FP8 band calls (no GPU): nsa_band_attn_fwd_ragged_fp8 / _paged_fp8 with their workspace queries and
nsa_paged_kv_quantize_fp8_rows are exported, the workspace is the bf16 call's, and the C ABI's declines -- the ones the Python operators
cannot reach among them -- come back as NSA_ERR_INVALID with a message naming the limit, before anything is launched or dereferenced."""
import pytest

from nsa_vibe_amd import _lib

INVALID = -1  # NSA_ERR_INVALID
G, H, S_KV, W = 2, 6, 4096, 512
P = 0x10000  # a 16-byte aligned address that is never dereferenced: every case below is declined on the host


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported(L):
    for name in ("nsa_band_attn_fwd_ragged_fp8", "nsa_band_attn_fwd_ragged_fp8_workspace", "nsa_band_attn_fwd_paged_fp8",
                 "nsa_band_attn_fwd_paged_fp8_workspace", "nsa_paged_kv_quantize_fp8_rows"):
        assert hasattr(L, name), name


@pytest.mark.parametrize("B,S", [(5, 1), (5, 3), (32, 32), (32, 256), (600, 3)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("h", [1, 6, 16])
def test_workspace_is_the_bf16_calls(L, B, S, D, h):
    need = L.nsa_band_attn_fwd_ragged_workspace(B, S, G, h, D, D, _lib.NSA_DT_BF16)
    assert L.nsa_band_attn_fwd_ragged_fp8_workspace(B, S, G, h, D, D, _lib.NSA_DT_BF16) == need
    assert L.nsa_band_attn_fwd_paged_fp8_workspace(B, S, G, h, D, D, _lib.NSA_DT_BF16) == L.nsa_band_attn_fwd_paged_workspace(B, S, G, h, D, D, _lib.NSA_DT_BF16) == need


def ragged(L, *, dtype=_lib.NSA_DT_BF16, ks=P, vs=P, row=64, B=5, ws=(None, 0), w=W):
    return L.nsa_band_attn_fwd_ragged_fp8(P, P, P, ks, vs, P, None, P, S_KV - 1, B, 1, G, H, 64, 64, S_KV, G * S_KV * 64, S_KV * 64, row, G * S_KV * 64, S_KV * 64, 64,
                                          G * S_KV, S_KV, G * S_KV, S_KV, 0, 1, 0, w, dtype, 0.0, *ws, None)


def paged(L, *, page_rows=1024, ws=(None, 0)):
    return L.nsa_band_attn_fwd_paged_fp8(P, P, P, P, P, P, 4, 8, 4, page_rows, P, None, P, S_KV - 1, 5, 1, G, H, 64, 64, G * page_rows * 64, page_rows * 64, 64,
                                         G * page_rows * 64, page_rows * 64, 64, G * page_rows, page_rows, G * page_rows, page_rows, 0, 1, 0, W, _lib.NSA_DT_BF16, 0.0,
                                         *ws, None)


@pytest.mark.parametrize("kw,limit", [(dict(dtype=_lib.NSA_DT_F16), "bf16 queries only"), (dict(dtype=_lib.NSA_DT_F32), "bf16 queries only"),
                                      (dict(vs=None), "null scale"), (dict(ks=None), "null scale"), (dict(row=128), "row stride"), (dict(w=0), "w >= 1"),
                                      (dict(), "workspace missing"), (dict(ws=(P, 64)), "workspace missing")])
def test_ragged_declines_name_the_limit(L, kw, limit):
    """B S G = 10 rows plan 16 splits: a call without (or with too small) a workspace is declined, not run unsplit"""
    assert L.nsa_band_attn_fwd_ragged_fp8_workspace(5, 1, G, H, 64, 64, _lib.NSA_DT_BF16) > 64
    assert ragged(L, **kw) == INVALID and limit in _lib.last_error()


@pytest.mark.parametrize("kw,limit", [(dict(page_rows=16), "page_rows = 16 is not built"), (dict(page_rows=96), "page_rows = 96 is not built"),
                                      (dict(), "workspace missing")])
def test_paged_declines_name_the_limit(L, kw, limit):
    assert paged(L, **kw) == INVALID and limit in _lib.last_error()


def test_quantiser_declines_a_page_size_that_is_not_built(L):
    rc = L.nsa_paged_kv_quantize_fp8_rows(P, P, P, P, 4, 8, 48, G, 64, 0, 10, G * 48 * 64, 48 * 64, 64, G * 48 * 64, 48 * 64, 64, G * 48, 48, None)
    assert rc == INVALID and "power of two in [32, 65536]" in _lib.last_error()
