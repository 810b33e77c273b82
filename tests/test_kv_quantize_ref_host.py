"""The reference the quantiser tests use (tests/test_hip_kv_quantize.py), checked on the CPU against torch's own conversion before either is
used against the kernel: a table of the 127 non-negative finite OCP e4m3 values and an encoder that picks the nearest one in float64 --
ties to the even code, the sign carried (-0 -> 0x80), saturation at +-448, a NaN code for a NaN."""
import numpy as np
import torch

FP8 = torch.float8_e4m3fn


def e4m3_table():
    """value of code c = 0 .. 126 (0x7E = 448): m 2^-9 for the subnormals (exponent field 0), (1 + m / 8) 2^(e - 7) otherwise"""
    c = np.arange(127)
    e, m = c >> 3, (c & 7).astype(np.float64)
    return np.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * 2.0 ** (e.astype(np.float64) - 7))


TABLE = e4m3_table()


def encode_e4m3(x):
    """float64 array -> uint8 e4m3 codes: nearest table value, ties to the even code, saturating; NaN -> 0x7F with the sign"""
    x = np.asarray(x, dtype=np.float64)
    a = np.minimum(np.abs(np.nan_to_num(x, nan=0.0)), 448.0)
    hi = np.clip(np.searchsorted(TABLE, a, side="left"), 1, 126)  # TABLE[hi - 1] <= a <= TABLE[hi] (a = 0: hi = 1)
    lo = hi - 1
    d_lo, d_hi = a - TABLE[lo], TABLE[hi] - a  # both exact: a and the table values are dyadic and within one binade step
    code = np.where(d_lo < d_hi, lo, np.where(d_hi < d_lo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(np.isnan(x), 0x7F, code)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def all_bf16_up_to_448():
    """every bf16 value with |x| <= 448, both signs and both zeros: bit patterns 0 .. 0x43E0 and the same with the sign bit (34,754 values)"""
    mag = np.arange(0x43E0 + 1, dtype=np.int32)
    bits = np.concatenate([mag, mag | 0x8000]).astype(np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def test_table_is_the_e4m3_value_set():
    assert len(TABLE) == 127 and TABLE[0] == 0 and TABLE[1] == 2.0 ** -9 and TABLE[8] == 2.0 ** -6 and TABLE[126] == 448
    assert (np.diff(TABLE) > 0).all()
    back = torch.arange(127, dtype=torch.uint8).view(FP8).double().numpy()
    assert np.array_equal(back, TABLE)


def test_table_encoder_equals_torch_for_every_bf16_value_up_to_448():
    x = all_bf16_up_to_448()
    assert x.numel() == 2 * (0x43E0 + 1) and float(x.float().abs().max()) == 448
    want = x.to(FP8).view(torch.uint8).numpy()
    got = encode_e4m3(x.double().numpy())
    assert np.array_equal(got, want)
    assert got[0] == 0x00 and got[0x43E0 + 1] == 0x80  # +0 and -0
    # the classes the sweep must hold: every code is hit, every midpoint between adjacent codes is present (bf16 holds them all: a midpoint
    # needs five significant bits), and there are values below half the smallest subnormal
    assert set(got.tolist()) == set(range(127)) | set(range(128, 255))
    mids = (TABLE[:-1] + TABLE[1:]) / 2
    xs = set(x.double().numpy().tolist())
    assert all(m in xs and -m in xs for m in mids)
    assert sum(0 < v < 2.0 ** -10 for v in xs) > 1000


def test_encoder_edges():
    f = lambda *v: encode_e4m3(np.array(v, dtype=np.float64)).tolist()  # noqa: E731
    assert f(2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -10 * 1.001, -(2.0 ** -10)) == [0x00, 0x02, 0x01, 0x80]  # ties to even, just above a tie
    assert f(448, 449, 1e30, -1e30, np.inf, -np.inf) == [0x7E, 0x7E, 0x7E, 0xFE, 0x7E, 0xFE]  # saturation
    assert f(432, 431.9, 17, 19) == [0x7E, 0x7D, 0x58, 0x5A]  # 432: tie of 416 (0x7D) and 448 (0x7E) -> even; 17 -> 16, 19 -> 20
    assert f(np.nan)[0] & 0x7F == 0x7F
