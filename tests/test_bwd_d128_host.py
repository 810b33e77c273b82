"""Host side of the D = 128 MFMA backward (no GPU): the workspace queries of the C ABI size the MFMA route at D = 128."""
from nsa_vibe_amd import _lib


def test_sel_bwd_workspace_d128():
    L = _lib.lib()
    args = (8, 4096, 2, 6, 128, 128, 4096, _lib.NSA_DT_BF16)
    mfma = L.nsa_sel_attn_bwd_workspace(*args, 0)
    assert mfma > 0
    assert L.nsa_sel_attn_bwd_workspace(*args, 1) == 0
    # the per-split dK / dV slabs are D wide: twice the D = 64 size of that part
    d64 = L.nsa_sel_attn_bwd_workspace(8, 4096, 2, 6, 64, 64, 4096, _lib.NSA_DT_BF16, 0)
    slab64 = 8 * 2 * 4096 * 64 * 4 * 2 * 8  # ns = 8 splits x [dK | dV] fp32
    assert mfma - d64 == slab64
    # fp32 and Dk != Dv stay on the generic kernel
    assert L.nsa_sel_attn_bwd_workspace(8, 4096, 2, 6, 128, 128, 4096, _lib.NSA_DT_F32, 0) == 0
    assert L.nsa_sel_attn_bwd_workspace(8, 4096, 2, 6, 192, 128, 4096, _lib.NSA_DT_BF16, 0) == 0


def test_band_bwd_workspace_d128():
    L = _lib.lib()
    args = (8, 4096, 2, 6, 128, 128, 4096, _lib.NSA_DT_BF16)
    generic = L.nsa_band_attn_bwd_workspace(*args, 1)
    assert generic > 0  # the range list is always reserved
    assert L.nsa_band_attn_bwd_workspace(*args, 0) > generic
