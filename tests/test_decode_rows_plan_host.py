"""Host side of nsa_sel_decode_rows (no GPU: the plan query makes no HIP call): the shapes the one-launch rows form takes and declines, its
DECODE_ROWS switch and the measured default rule (S = 1 on a row of 32 chunks and more goes to the separate launches)."""
import ctypes

import pytest

from nsa_vibe_amd import _lib

BF16 = _lib.NSA_DT_BF16


def ncmp(t):
    return 0 if t + 1 < 32 else (t + 1 - 32) // 16 + 1


def plan(B, S, ctx, D=64, h=6, G=2, n=16, dt=BF16):
    """the plan for a cache of ctx tokens after the S new ones (t0 = ctx - S)"""
    n_l, f = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().nsa_sel_decode_rows_plan(B, S, G, h, D, D, ncmp(ctx - 1), -(-ctx // 64), ctx, n, dt, ctypes.byref(n_l), ctypes.byref(f))
    _lib.check(rc, "nsa_sel_decode_rows_plan")
    return n_l.value, f.value


def test_rows_plan_forms_and_declines():
    assert plan(3, 8, 1060) == (1, 0)
    assert plan(1, 8, 32804) == (1, 1)          # 33 chunks on 16 waves: four chunks per wave
    assert plan(1, 8, 32796) == (1, 0)          # 32 chunks: still two per wave
    assert plan(17, 8, 5008) == (1, 0)          # 272 rows: eight waves, 5 chunks
    assert plan(40, 8, 16384 + 64) == (1, 1)    # 640 rows on eight waves: 17 chunks exceed two per wave
    assert plan(3, 8, 1060, D=128) == (1, 0)
    assert plan(1, 8, 16384, D=128) == (1, 0)   # 16 chunks: the most D = 128 holds
    for args, kw in [((2, 17, 1069), {}), ((2, 8, 18), {}), ((1, 8, 20008), {"D": 128}), ((1, 8, 70000), {}), ((40, 8, 40000), {}),
                     ((3, 8, 1060), {"dt": _lib.NSA_DT_F32}), ((3, 8, 1060), {"D": 32}), ((3, 8, 1060), {"h": 17})]:
        launches, form = plan(*args, **kw)
        assert launches > 1 and form == -1, (args, kw)
    assert plan(3, 8, 1060, dt=_lib.NSA_DT_F16) == (1, 0)


def test_rows_plan_follows_the_switches(tune):
    assert plan(1, 1, 32768)[0] > 1             # the measured rule: S = 1 on a row of 32 chunks loses to the single step's team form
    assert plan(1, 1, 16384) == (1, 0) and plan(1, 2, 32768) == (1, 0)
    tune("DECODE_ROWS", 1)
    assert plan(1, 1, 32768) == (1, 0)
    tune("DECODE_ROWS", 0)
    assert plan(3, 8, 1060)[0] > 1
    tune("DECODE_ROWS", -1)
    tune("DECODE_UNFUSED", 1)
    assert plan(3, 8, 1060)[0] > 1
    tune("DECODE_UNFUSED", -1)
    tune("DECODE_STEP", 0)
    assert plan(3, 8, 1060)[0] > 1


def test_rows_workspace_and_refusals():
    L = _lib.lib()
    assert L.nsa_sel_decode_rows_workspace(3, 8, 2, 6, 64, 64, 65, 17, 16, BF16) >= 4 * 3 * 8 * 2 * 17
    assert L.nsa_sel_decode_rows_workspace(0, 8, 2, 6, 64, 64, 65, 17, 16, BF16) == 0
    n_l, f = ctypes.c_int(0), ctypes.c_int(0)
    assert L.nsa_sel_decode_rows_plan(3, 8, 2, 6, 64, 64, 65, 17, 4, 16, BF16, ctypes.byref(n_l), ctypes.byref(f)) != 0  # S_kv < S
    # a cache that does not hold the S tokens is refused before anything is launched (1 stands in for the device pointers)
    rc = L.nsa_sel_decode_rows(1, 1, 1, 1, None, None, None, 1, 1, 3, 8, 2, 6, 64, 64, 65, 17, 1059, 32, 16, 64, 16, 1052, *([64] * 9), BF16, 0.0, None, 0, None)
    assert rc != 0 and "cache must hold" in _lib.last_error()
