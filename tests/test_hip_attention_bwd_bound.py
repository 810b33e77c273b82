"""GPU: the attention backward kernels (nsa_sel_attn_bwd, nsa_band_attn_bwd through the C ABI) against the float64 reference, element by
element, inside the rounding bound of oracle.sel_attention_bwd_bound -- at the shapes of attention_bwd_cases.py, where the MFMA backward
takes each of its paths, and with sparse probe phases (dO on every s-th row) so that one wrong (row, key) term of dK / dV cannot hide under
the sum of all rows (test_attention_bwd_bound_host.py measures that power on the same inputs).

The kernels are fed the reference's own forward: O rounded to the activation dtype and the fp32 lse (-inf on rows without a key), so no
forward error enters.  dK / dV are the ABI's fp32 outputs, pre-filled with NaN (the callee writes them fully).  Per phase: finite outputs,
|got - ref| <= bound at every element, exact zeros where no term lands, and on the MFMA route two runs bitwise equal.
Worst |got - ref| / bound seen on the MI355X is recorded in the docstrings."""
import functools

import numpy as np
import pytest
import torch

import attention_bwd_cases as abc
from oracle import nsa_oracle as orc

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _dev(a, dtype):
    """device tensor of a (values already representable in dtype)"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DT[dtype]).cuda()


def _kv(a, dtype, pad):
    """K or V on the device; pad > 0: a [:, :, :S_kv] view of a buffer with `pad` more (NaN) rows per (b, g)"""
    t = _dev(a, dtype)
    if not pad:
        return t
    buf = torch.full((t.shape[0], t.shape[1], t.shape[2] + pad, t.shape[3]), float("nan"), dtype=t.dtype, device="cuda")
    buf[:, :, : t.shape[2]] = t
    return buf[:, :, : t.shape[2]]


def _scale(Dk):
    return float(np.float32(1.0 / np.sqrt(Dk)))


def bwd_hip(x, dO, O, lse, dtype, variant, band=None, pad=0):
    """nsa_sel_attn_bwd (band: nsa_band_attn_bwd with those a, dd, c, w) through the C ABI -> (dQ, dK, dV) as float64 numpy arrays.
    x: dict of float64 arrays (attention_bwd_cases.inputs); O float64 (rounded here), lse float64."""
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd._native import _DT, _stream

    B, S, G, h, Dk = x["Q"].shape
    S_kv, Dv = x["K"].shape[2], x["V"].shape[3]
    Q, K, V, dOd = _dev(x["Q"], dtype), _kv(x["K"], dtype, pad), _kv(x["V"], dtype, pad), _dev(dO, dtype)
    Od = _dev(orc.round_to(O, dtype), dtype)
    ld = torch.from_numpy(np.ascontiguousarray(lse, np.float32)).cuda()
    rg = torch.from_numpy(np.ascontiguousarray(x["ranges"], np.int32)).cuda()
    dQ = torch.full(Q.shape, float("nan"), dtype=Q.dtype, device="cuda")
    dK = torch.full((B, G, S_kv, Dk), float("nan"), dtype=torch.float32, device="cuda")
    dV = torch.full((B, G, S_kv, Dv), float("nan"), dtype=torch.float32, device="cuda")
    L, dt = _lib.lib(), _DT[DT[dtype]]
    size = L.nsa_band_attn_bwd_workspace if band else L.nsa_sel_attn_bwd_workspace
    nws = int(size(B, S, G, h, Dk, Dv, S_kv, dt, variant))
    ws = torch.empty(max(nws, 1) + 256, dtype=torch.uint8, device="cuda")
    wptr = (ws.data_ptr() + 255) & ~255
    ks, vs = K.stride()[:3], V.stride()[:3]
    if band:
        rc = L.nsa_band_attn_bwd(Q.data_ptr(), K.data_ptr(), V.data_ptr(), Od.data_ptr(), ld.data_ptr(), dOd.data_ptr(), dQ.data_ptr(),
                                 dK.data_ptr(), dV.data_ptr(), B, S, G, h, Dk, Dv, S_kv, *ks, *vs, 0, band["a"], band["dd"], band["c"],
                                 min(band["w"], 2 ** 31 - 1), dt, _scale(Dk), variant, wptr if nws else None, nws, _stream(Q.device))
        _lib.check(rc, "nsa_band_attn_bwd")
    else:
        rc = L.nsa_sel_attn_bwd(Q.data_ptr(), K.data_ptr(), V.data_ptr(), rg.data_ptr(), Od.data_ptr(), ld.data_ptr(), dOd.data_ptr(),
                                dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), B, S, G, h, Dk, Dv, S_kv, rg.shape[3], *ks, *vs, dt,
                                _scale(Dk), variant, wptr if nws else None, nws, _stream(Q.device))
        _lib.check(rc, "nsa_sel_attn_bwd")
    torch.cuda.synchronize()
    return tuple(t.double().cpu().numpy() for t in (dQ, dK, dV))


@functools.lru_cache(maxsize=2)
def _inputs(name, dtype, Dk, Dv):
    return abc.inputs(name, dtype, Dk, Dv)


def check_case(name, dtype, Dk, Dv=None, variant=2, pad=0, bitwise=True):
    """every phase of a case (the dense one first: its O and lse, computed on every row, feed all phases) -> worst ratios (dQ, dK, dV)"""
    case = abc.CASES[name]
    x = _inputs(name, dtype, Dk, Dv or Dk)
    worst = np.zeros(3)
    stray = 0  # non-zero outputs where no term lands
    fwd = None
    for phase in [None] + case.phases()[:-1]:
        dO = abc.phase_dO(case, x["dO"], phase)
        ref, bnd, f = orc.sel_attention_bwd_bound(x["Q"], x["K"], x["V"], x["ranges"], dO, dtype, _scale(Dk), probe_only=phase is not None)
        fwd = fwd or f
        got = bwd_hip(x, dO, fwd[0], fwd[1], dtype, variant, case.band, pad)
        for i, (g, r, b, what) in enumerate(zip(got, ref, bnd, ("dQ", "dK", "dV"))):
            assert np.isfinite(g).all(), (what, phase)
            err = np.abs(g - r)
            ratio = float((err[b > 0] / b[b > 0]).max(initial=0.0))
            worst[i] = max(worst[i], ratio)
            stray += np.count_nonzero(g[b == 0])
            print(f"{name} {dtype} Dk{Dk} phase {phase} {what}: worst |got - ref| / bound {ratio:.3f}, "
                  f"{np.count_nonzero(g[b == 0])} non-zero elements without a term (largest {np.abs(g[b == 0]).max(initial=0.0):.3g})")
        if bitwise:
            again = bwd_hip(x, dO, fwd[0], fwd[1], dtype, variant, case.band, pad)
            for g, a in zip(got, again):
                assert np.array_equal(g, a)
    assert stray == 0, f"{stray} elements that no (row, head, key) term reaches are not zero"
    assert worst.max() <= 1.0, worst
    return worst


D_DTYPE = [(64, "bf16"), (64, "fp16"), (128, "bf16"), (128, "fp16")]


@pytest.mark.parametrize("D,dtype", D_DTYPE)
@pytest.mark.parametrize("name", ["A", "B", "C", "D5", "D7", "D1", "E", "S3"])
def test_selection_mfma_backward_within_bound(name, D, dtype):
    """variant 2: A one split, two 256-row chunks, partial last key block, rows form of dQ; B two splits + the reduce kernel, full hits and
    the clamped last block; C h = 16, the one-row dQ kernel; D5 / D7 / D1 rows straddling the 16-slot tiles; E 511 of the pending list's
    512 entries; S3 three rows per (b, g), the one-row dQ kernel on its row-linear grid (12 rows, 3 workgroups).  Worst |got - ref| / bound
    seen on the MI355X over the 28 runs of A-E: dQ 0.46 (E, D = 64, bf16), dK 0.71 and dV 0.98 (D1, h = 1:
    a key that one probe row reaches has a single rounded term, whose error can be the whole half ulp the bound allows); dense phases
    alone: 0.46 / 0.55 / 0.89.  S3 (4 runs): dQ 0.31, dK 0.57, dV 0.84, the dense phase alone the same."""
    check_case(name, dtype, D)


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("D,dtype", D_DTYPE)
def test_selection_mfma_backward_long_context_within_bound(D, dtype, rows, tune):
    """F: ranges across key 65536 and in the partial last tile of 70000 keys, with the one-row (SEL_ROWS 0) and the rows dQ kernel.
    Seen on the MI355X: dQ 0.23, dK 0.79, dV 0.92 (the same figures from both dQ kernels)."""
    tune("SEL_ROWS", rows)
    check_case("F", dtype, D)


@pytest.mark.parametrize("D,dtype", D_DTYPE)
def test_selection_mfma_backward_strided_cache_views(D, dtype):
    """G: case A with K and V as [:, :, :S_kv] views of larger buffers (the strides are passed; the rows behind the view hold NaN).
    Seen on the MI355X: the figures of case A on contiguous tensors, dQ 0.45, dK 0.55, dV 0.86."""
    check_case("A", dtype, D, pad=37)


@pytest.mark.parametrize("dtype,Dk,Dv", [("fp32", 32, 32), ("bf16", 128, 96)])
def test_selection_generic_backward_within_bound(dtype, Dk, Dv):
    """variant 1 (one wave per row, fp32 atomics): the same bound, which does not depend on the summation order.  Seen on the MI355X:
    fp32 dQ 0.04, dK 0.04, dV 0.06 (the bound counts worst-case fp32 sums); bf16 dQ 0.25, dK 0.15, dV < 0.001 (this kernel keeps P and
    dS in fp32: only the stored dQ and the rounded O show at the bf16 level)."""
    check_case("A", dtype, Dk, Dv, variant=1, bitwise=False)


@pytest.mark.parametrize("D,dtype", D_DTYPE)
@pytest.mark.parametrize("name", list(abc.BAND_CASES))
def test_band_mfma_backward_within_bound(name, D, dtype):
    """nsa_band_attn_bwd, variant 2: windows 1 / 33 / 100 (the lower window edge inside a tile), the compressed schedule, and the form for
    >= 2048 token groups (48 slots per wave at D = 64) with a window and with the compressed schedule.  Seen on the MI355X over the 24
    runs: dQ 0.55 (long_cmp), dK 0.59 (w100), dV 0.92 (long_w33); w = 1 is exact (p = 1, dS = 0, dV = dO)."""
    check_case(name, dtype, D)


def test_autograd_backward_is_the_c_abi_call():
    """selection_attention_hip(...).backward hands the kernels the forward's own O and lse: bitwise the C-ABI call fed the same"""
    import nsa_vibe_amd as nv

    dtype, D = "bf16", 64
    x = _inputs("A", dtype, D, D)
    rg = torch.from_numpy(x["ranges"]).cuda()
    q, k, v = (_dev(x[n], dtype).requires_grad_(True) for n in ("Q", "K", "V"))
    nv.selection_attention_hip(q, k, v, rg, variant=2, bwd_variant=2).backward(_dev(x["dO"], dtype))
    O, lse = nv.selection_attention_hip(q.detach(), k.detach(), v.detach(), rg, variant=2, return_lse=True)
    dQ, dK, dV = bwd_hip(x, x["dO"], O.double().cpu().numpy(), lse.double().cpu().numpy(), dtype, 2)
    assert np.array_equal(q.grad.double().cpu().numpy(), dQ)
    for grad, want in ((k.grad, dK), (v.grad, dV)):
        assert torch.equal(grad.cpu(), torch.from_numpy(want).float().to(DT[dtype]))
