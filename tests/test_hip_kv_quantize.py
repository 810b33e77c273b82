"""nsa_kv_quantize_fp8 / nsa_paged_kv_quantize_fp8 at the quantiser's edges: every bf16 value at exact power-of-two scales, rows whose scale is
an fp32 subnormal, append-sized row ranges, and rows that hold a NaN or an infinity.  The reference is the float64 table encoder of
tests/test_kv_quantize_ref_host.py (nearest e4m3 value, ties to the even code, sign carried, saturation at +-448), which that file checks
against torch's conversion on the CPU."""
import numpy as np
import pytest
import torch

from test_hip_selection import nv  # noqa: F401
from test_kv_quantize_ref_host import all_bf16_up_to_448, encode_e4m3

pytestmark = pytest.mark.gpu

FP8, BF16 = torch.float8_e4m3fn, torch.bfloat16
KS = (0, -8, 7, -120, 119)


def u8(X8):
    return X8.view(torch.uint8).cpu().numpy()


def reference(X):
    """bf16 rows [..., D] on the CPU -> (codes uint8, scale float32): scale = fp32(amax) / fp32(448) rounded to fp32 by numpy (1 for an
    all-zero row), codes = the float64 table encoder on the quotient x / scale as the quantiser defines it: the IEEE fp32 quotient (numpy's
    float32 division, subnormals kept).  That rounding is part of the format, not an error of the kernel: x / amax is a ratio of two 8-bit
    significands, so 448 x / amax lands on an e4m3 midpoint often (x = 3/32 amax: 42, between 40 and 44) and the inexact scale moves the
    exact quotient off it by parts in 10^8 -- the fp32 quotient is the midpoint again and ties to even, which is also what torch's
    (x.float() / scale).to(float8_e4m3fn) of the existing test gives.  The exact quotient in float64 would round the other way there."""
    x = X.float().numpy()
    amax = np.abs(x).max(-1)
    assert x.dtype == np.float32 and amax.dtype == np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(amax == 0, np.float32(1), amax / np.float32(448)).astype(np.float32)
        q32 = x / scale[..., None]
    assert q32.dtype == np.float32
    return encode_e4m3(q32.astype(np.float64)), scale


def sweep_rows(D):
    """[len(KS), 1, rows, D] bf16: plane j holds, at scale 2^k (k = KS[j]), rows whose element 0 is 448 2^k and whose other D - 1 elements
    run through v 2^k for every bf16 v with |v| <= 448 in bit-pattern order (formed in float64, rounded to bf16; the last row is padded with
    zeros).  Consecutive values of one column are D - 1 patterns apart, an odd step: every column meets every mantissa pattern, both
    signs, zeros, the e4m3 subnormal range, midpoints of every binade and values below half the smallest subnormal."""
    v = all_bf16_up_to_448().double()
    rows = -(-v.numel() // (D - 1))
    body = torch.zeros(rows * (D - 1), dtype=torch.float64)
    body[:v.numel()] = v
    X = torch.empty((len(KS), 1, rows, D), dtype=BF16)
    for j, k in enumerate(KS):
        X[j, 0, :, 0] = 448 * 2.0 ** k
        X[j, 0, :, 1:] = (body * 2.0 ** k).to(BF16).view(rows, D - 1)
    return X


@pytest.mark.parametrize("D", [64, 128])
def test_every_bf16_value_at_exact_scales(nv, D):
    """scales are exactly 2^k, so x / scale is exact and the bytes are e4m3_rne of the bf16 value the row holds, for all 34,754 values at
    each k in {0, -8, 7, -120, 119}.  At k = -120 the small end of the sweep has underflowed to bf16 (= fp32) subnormals and to zero on
    the way in; the reference reads the bf16 that resulted, so a kernel that flushes subnormal inputs or quotients fails here."""
    X = sweep_rows(D)
    X8, z = nv.quantize_kv_fp8(X.cuda())
    for j, k in enumerate(KS):
        assert bool((z[j] == 2.0 ** k).all()), k
        want = encode_e4m3(X[j].double().numpy() / 2.0 ** k)
        got = u8(X8[j])
        bad = np.argwhere(got != want)
        assert bad.size == 0, (k, bad[:4].tolist(), got[got != want][:4].tolist(), want[got != want][:4].tolist())
    sub = X[KS.index(-120)].float()
    assert bool(((sub != 0) & (sub.abs() < 2.0 ** -126)).any())  # subnormal inputs are present


@pytest.mark.parametrize("D", [64, 128])
def test_tiny_rows_with_subnormal_scales(nv, D):
    """amax in {2^-118, 2^-126, 2^-133}: amax / 448 is an fp32 subnormal.  One row per lane position of the maximum and sign, the other
    elements amax times fractions (many become bf16 subnormals or zero)"""
    gen = torch.Generator().manual_seed(D)
    amaxes = (2.0 ** -118, 2.0 ** -126, 2.0 ** -133)
    cols = (0, 7, 8, D // 2 + 3, D - 1)
    X = torch.empty((len(amaxes), 2, 2 * len(cols) + 3, D), dtype=BF16)
    for j, a in enumerate(amaxes):
        frac = torch.rand(X.shape[1:], generator=gen, dtype=torch.float64) * 2 - 1
        frac[:, 0] = torch.exp2(-torch.randint(0, 9, frac[:, 0].shape, generator=gen).double()) * frac[:, 0].sign()  # powers of two: exact quotients
        X[j] = (frac * a * 0.99).to(BF16)
        for i, col in enumerate(cols):
            X[j, :, 2 * i + 1, col], X[j, :, 2 * i + 2, col] = a, -a
    X8, z = nv.quantize_kv_fp8(X.cuda())
    codes, scale = reference(X)
    assert float(scale.max()) < 2.0 ** -126 and float(scale.min()) > 0
    print(f"tiny rows D={D}: scales differing {int((z.cpu().numpy() != scale).sum())} of {scale.size}, bytes differing {int((u8(X8) != codes).sum())} of {codes.size}")
    assert np.array_equal(z.cpu().numpy(), scale)
    assert np.array_equal(u8(X8), codes)


APPENDS = (1, 1, 7, 9, 3, 1, 19)


@pytest.mark.parametrize("D", [64, 128])
def test_append_sized_ranges(nv, D):
    """rows [0, 41) of a strided source by calls of 1, 1, 7, 9, 3, 1 and 19 rows (B = 3, G = 2: a launch of 6 to 114 rows, less than one
    workgroup's) into a mirror pre-filled with 0.5 / 7.0: after each call the rows done so far equal one call over [0, 41) and every other
    row still holds the fill; t1 == t0 touches nothing"""
    B, G, S, n = 3, 2, 50, sum(APPENDS)
    big = torch.randn((B, G, S, 2 * D), generator=torch.Generator().manual_seed(D + 1)).to(BF16)
    X = big.cuda()[..., D // 2:D // 2 + D]
    ref8, refz = nv.quantize_kv_fp8(X, 0, n)
    codes, scale = reference(X[:, :, :n].cpu())
    assert np.array_equal(u8(ref8[:, :, :n]), codes) and np.array_equal(refz[:, :, :n].cpu().numpy(), scale)
    out, sc = torch.full(X.shape, 0.5, device="cuda").to(FP8), torch.full(X.shape[:3], 7.0, device="cuda")
    nv.quantize_kv_fp8(X, 17, 17, out=out, scale_out=sc)
    assert bool((sc == 7).all()) and bool((out.float() == 0.5).all())
    t = 0
    for m in APPENDS:
        nv.quantize_kv_fp8(X, t, t + m, out=out, scale_out=sc)
        t += m
        assert torch.equal(out.view(torch.uint8)[:, :, :t], ref8.view(torch.uint8)[:, :, :t]) and torch.equal(sc[:, :, :t], refz[:, :, :t]), t
        assert bool((sc[:, :, t:] == 7).all()) and bool((out[:, :, t:].float() == 0.5).all()), t
    assert t == n


@pytest.mark.parametrize("D", [64, 128])
def test_append_sized_ranges_paged(nv, D):
    """the same appends through quantize_kv_fp8_paged on 32-row pages behind a permuted table row, twice: from row 0 the last call
    [22, 41) crosses the page edge at 32 inside the call; from row 23 the third call ends exactly on row 32, the fourth starts there and
    the last ends exactly on row 64.  After each call the pools equal the contiguous call's bytes and scales on the rows done so far and
    the fill everywhere else (the other pages included); t1 == t0 touches nothing"""
    G, rows = 2, 32
    X = torch.randn((1, G, 3 * rows, D), generator=torch.Generator().manual_seed(D + 2)).to(BF16).cuda()
    ref8, refz = nv.quantize_kv_fp8(X)
    row, xp = [3, 0, 2], torch.zeros((5, G, rows, D), dtype=BF16, device="cuda")
    for j, p in enumerate(row):
        xp[p] = X[0, :, rows * j:rows * j + rows]
    table = torch.tensor(row, dtype=torch.int32, device="cuda")
    for start in (0, 23):
        sched = np.cumsum((start,) + APPENDS).tolist()
        if start == 0:
            assert any(a < rows < b for a, b in zip(sched[:-1], sched[1:]))
        else:
            assert rows in sched[1:-1] and sched[-1] == 2 * rows
        o8, oz = torch.full(xp.shape, 0.5, device="cuda").to(FP8), torch.full(xp.shape[:3], 7.0, device="cuda")
        nv.quantize_kv_fp8_paged(xp, table, 9, 9, o8, oz)
        assert bool((oz == 7).all()) and bool((o8.float() == 0.5).all())
        for t0, t1 in zip(sched[:-1], sched[1:]):
            nv.quantize_kv_fp8_paged(xp, table, t0, t1, o8, oz)
            want8, wantz = torch.full(xp.shape, 0.5, device="cuda").to(FP8).view(torch.uint8), torch.full(xp.shape[:3], 7.0, device="cuda")
            for j, p in enumerate(row):
                lo, hi = max(start, rows * j), min(t1, rows * j + rows)
                if hi > lo:
                    want8[p, :, lo - rows * j:hi - rows * j] = ref8.view(torch.uint8)[0, :, lo:hi]
                    wantz[p, :, lo - rows * j:hi - rows * j] = refz[0, :, lo:hi]
            assert torch.equal(o8.view(torch.uint8), want8) and torch.equal(oz, wantz), (start, t0, t1)


@pytest.mark.parametrize("D", [64, 128])
def test_non_finite_rows(nv, D):
    """a row holding a NaN, a +inf or a -inf (at lane positions 0, 7, 8 and D - 1) gets a NaN scale and an e4m3 NaN code in every byte, so
    the FP8 calls give NaN where the bf16 calls would.  The bad rows are the odd rows of each plane: every wave (8 rows at D = 64, 4 at
    D = 128) holds finite rows on both sides of each, and those equal the reference bit for bit"""
    bads = [(v, col) for v in (float("nan"), float("inf"), -float("inf")) for col in (0, 7, 8, D - 1)]
    X = torch.randn((2, 2, 2 * len(bads) + 1, D), generator=torch.Generator().manual_seed(D + 3)).to(BF16)
    X[1, 1, 4] = 0  # a zero row between two bad ones: scale 1, bytes 0
    for i, (v, col) in enumerate(bads):
        X[:, :, 2 * i + 1, col] = v
    X[1, 0, 5, 20] = float("inf")  # two kinds in one row
    X8, z = nv.quantize_kv_fp8(X.cuda())
    got8, gotz = u8(X8), z.cpu().numpy()
    assert np.isnan(gotz[:, :, 1::2]).all()
    assert ((got8[:, :, 1::2] & 0x7F) == 0x7F).all()
    codes, scale = reference(X[:, :, 0::2])
    assert np.array_equal(gotz[:, :, 0::2], scale) and gotz[1, 1, 4] == 1
    assert np.array_equal(got8[:, :, 0::2], codes)
    assert bool(torch.isnan(X8[:, :, 1::2].float()).all())  # (what a reader of the cache sees)
