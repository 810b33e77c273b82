"""Host side of the ragged layer call with FP8 mirrors (no GPU): nsa_layer_decode_ragged_fp8 and its queries are exported, the workspace is the
bf16 call's, the plan is the bf16 plan + 1 launch (the mirror writer) with the same route, and every decline of its own comes back as
NSA_ERR_INVALID with a message naming the limit before anything is launched or dereferenced (the pointers below are aligned addresses
nobody owns)."""
import ctypes

import pytest

from nsa_vibe_amd import _lib
from test_layer_decode_rows_host import cache, layer

INVALID = -1  # NSA_ERR_INVALID
P = 0x10000  # a 256-byte aligned address that is never dereferenced: every call below is declined on the host
BF16, F16 = _lib.NSA_DT_BF16, _lib.NSA_DT_F16


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def plans(L, d, B, S, S_max, t_max):
    out = []
    S_sel = -(-(min(t_max, S_max - 1) + 1) // 64)
    for fn in (L.nsa_layer_decode_ragged_plan, L.nsa_layer_decode_ragged_fp8_plan):
        n, r = ctypes.c_int(-7), ctypes.c_int(-7)
        out.append((fn(ctypes.byref(d), B, S, S_max, t_max, S_sel, ctypes.byref(n), ctypes.byref(r)), n.value, r.value))
    return out


@pytest.mark.parametrize("B", [3, 600])
@pytest.mark.parametrize("S", [1, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_exported_workspace_is_the_bf16_calls_and_the_plan_adds_one_launch(L, B, S, D):
    for name in ("nsa_layer_decode_ragged_fp8", "nsa_layer_decode_ragged_fp8_workspace", "nsa_layer_decode_ragged_fp8_plan"):
        assert hasattr(L, name), name
    d = layer(D=D, dim=768 if D == 64 else 1536)
    ref = ctypes.byref(d)
    assert L.nsa_layer_decode_ragged_fp8_workspace(ref, B, S, 2048) == L.nsa_layer_decode_ragged_workspace(ref, B, S, 2048) > 0
    (rc, n, r), (rc8, n8, r8) = plans(L, d, B, S, 2048, 1059)
    assert (rc, r, rc8, r8) == (0, 1, 0, 1) and n8 == n + 1


def call(L, d, *, scale=P, mirror=P, S_max=2048, t_max=1059, desc=True):
    kd = cache(3, S_max)
    m8 = _lib.NsaKvFp8Desc()
    for name, _ in m8._fields_:
        setattr(m8, name, P)
    m8.V_cmp_scale, m8.K_win8 = scale, mirror
    S_sel = -(-(min(t_max, S_max - 1) + 1) // 64)
    return L.nsa_layer_decode_ragged_fp8(ctypes.byref(d), ctypes.byref(kd), ctypes.byref(m8) if desc else None, P, P, P, t_max, 4, P, P, P, S_sel, P, P, None, 0,
                                         None)


def test_declines_name_the_limit(L, tune):
    for kw, dt, limit in [(dict(), F16, "bf16 layer only"), (dict(scale=None), BF16, "null scale slab pointer"),
                          (dict(mirror=None), BF16, "null FP8 mirror slab pointer"), (dict(mirror=P + 8), BF16, "16-byte aligned"),
                          (dict(scale=P + 2), BF16, "4-byte aligned"), (dict(desc=False), BF16, "null FP8 mirror descriptor"),
                          (dict(t_max=-1), BF16, "t_max"), (dict(), BF16, "workspace")]:
        assert call(L, layer(dt), **kw) == INVALID and _lib.last_error().startswith("layer_decode_ragged_fp8: ") and limit in _lib.last_error(), (kw, _lib.last_error())
    d = layer()
    tune("DECODE_LONG", 1)  # the bf16 call then plans the long-row form; FP8 K/V have none
    (rc, n, r), fp8 = plans(L, d, 3, 4, 1 << 17, 70000)
    assert (rc, r) == (0, 1) and n > 0 and fp8 == (0, 0, -1)
    assert call(L, d, S_max=1 << 17, t_max=70000) == INVALID and "beyond the forms built for FP8 K/V caches" in _lib.last_error()
    assert plans(L, layer(F16), 3, 4, 2048, 1059)[1] == (0, 0, -1)
