"""CPU: the float64 attention backward with per-element bounds (oracle.sel_attention_bwd_bound) that the GPU tests of
test_hip_attention_bwd_bound.py hold the kernels to.
  (a) it is the same function as the C oracle's sel_attention_masked_bwd and as the reference's autograd (goldens g16);
  (b) POWER: on every case of attention_bwd_cases.py a kernel that gets one (row, key) term wrong lands outside the bound -- mutants built
      from the float64 terms (a wrong mask leaves lse, O and delta alone: it only adds or removes the terms of its keys);
  (c) the share of the same mutants that the max-norm criterion of the older tests (3e-2 max(1, max|ref|), dense dO) accepts is printed.
"""
import dataclasses

import numpy as np
import pytest

import attention_bwd_cases as abc
from conftest import load_golden


def _ratio(got, ref, bound):
    """max |got - ref| / bound; elements with bound 0 must be equal"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert not err[bound == 0].any()
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "D5", "D1", "w33", "cmp"])
def test_reference_equals_c_oracle(orc, name):
    """against the C oracle (fp64 inner math, every term rounded to fp32 and summed in fp32): within the fp32 part of the bound, which is
    (N + 2) 2^-24 sum|terms| and a few 2^-24 per term"""
    x = abc.inputs(name, "bf16", 32)
    ref, bnd, (O, lse) = orc.sel_attention_bwd_bound(x["Q"], x["K"], x["V"], x["ranges"], x["dO"], "fp32")
    got = orc.sel_attention_masked_bwd(x["Q"], x["K"], x["V"], x["ranges"], x["dO"])
    for g, r, b, what in zip(got, ref, bnd, ("dQ", "dK", "dV")):
        ratio = _ratio(g, r, b)
        print(f"{name} {what}: C oracle vs float64 reference {ratio:.3f} of the fp32 bound")
        assert ratio <= 1.0, what
    Oc, lc = orc.sel_attention_masked(x["Q"], x["K"], x["V"], x["ranges"], return_lse=True)
    assert np.abs(Oc - O).max() <= 1e-5
    fin = np.isfinite(lse)
    assert np.array_equal(np.isfinite(lc), fin) and np.abs(lc[fin] - lse[fin]).max() <= 1e-5


@pytest.mark.parametrize("name", ["ref_test_shape", "a", "b", "c"])
def test_reference_equals_g16_autograd(orc, name):
    """against torch autograd through the reference's grouped_selection_attention_masked in fp32 (goldens g16): within the fp32 bound
    (the reference's softmax and matmuls round in fp32 where the bound counts a kernel's fp32 roundings)"""
    g = load_golden("g16_bwd_" + name)
    ref, bnd, (O, _) = orc.sel_attention_bwd_bound(g["Q"], g["K"], g["V"], g["ranges"], g["dO"], "fp32")
    assert np.abs(O - g["O"]).max() <= 1e-5
    for what, r, b in zip(("dQ", "dK", "dV"), ref, bnd):
        ratio = _ratio(g[what], r, b)
        print(f"g16 {name} {what}: reference autograd vs float64 reference {ratio:.3f} of the fp32 bound")
        assert ratio <= 1.0, what


def test_band_wrapper_is_the_band(orc):
    x = abc.inputs("w33", "bf16", 32)
    kw = abc.CASES["w33"].band
    a = orc.band_attention_bwd_bound(x["Q"], x["K"], x["V"], x["dO"], "bf16", **kw)
    b = orc.sel_attention_bwd_bound(x["Q"], x["K"], x["V"], x["ranges"], x["dO"], "bf16")
    for u, v in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]):
        assert np.array_equal(u, v)
    rq, rk, rv = orc.band_attention_bwd(x["Q"], x["K"], x["V"], x["dO"], **kw)
    assert np.abs(rk - a[0][1]).max() <= 1e-4 and np.abs(rq - a[0][0]).max() <= 1e-4


# ---- (b), (c) ----------------------------------------------------------------------------------------------------------------------------
KINDS = ("block_drop", "block_full", "edge_drop", "edge_add", "twice")
OLD_BAR = 3e-2


def _chunk_detect(c, bQ, bK, bV, old=None):
    """per (active row, column) of one chunk: does switching that (row, key) term on or off leave the bound in dK / dV (vk) or in dQ (q);
    old = (MQ, MK, MV): also whether the change stays inside the older tests' max-norm bar on all three tensors"""
    b, g, cols = c["b"], c["g"], c["cols"]
    rows = c["rows"][c["ar"]]
    tV = np.abs(np.einsum("rhc,rhd->rcd", c["p"], c["dO"]))
    tK = np.abs(np.einsum("rhc,rhd->rcd", c["dS"], c["q"]))
    vk = (tV > bV[b, g, cols][None]).any(axis=2) | (tK > bK[b, g, cols][None]).any(axis=2)
    aK = np.abs(c["Kc"])
    dq = np.zeros(vk.shape, bool)
    mq = np.zeros(vk.shape)
    with np.errstate(divide="ignore"):
        for hh in range(c["dS"].shape[1]):
            thr = (bQ[b, rows, g, hh][:, None, :] / aK[None]).min(axis=2)  # [A,C]: the smallest |dS| that shows in some element of dQ
            dq |= np.abs(c["dS"][:, hh]) > thr
            mq = np.maximum(mq, np.abs(c["dS"][:, hh]) * aK.max(axis=1)[None])
    ok_old = None
    if old is not None:
        ok_old = (mq <= OLD_BAR * old[0]) & (tK.max(axis=2) <= OLD_BAR * old[1]) & (tV.max(axis=2) <= OLD_BAR * old[2])
    return vk, dq, ok_old


def _mutants(case, x, orc, dtype="bf16"):
    """-> found[kind], old[kind]: int8 arrays over (b, g, row, key) -- (b, g, row, 64-key block) for the block kinds --: 0 no such mutant,
    1 a mutant, 2 a mutant that leaves the bound in some phase (found) / that the old bar accepts in the dense phase (old)"""
    nblk = (case.S_kv + 63) // 64
    shape = {k: (case.B, case.G, case.S, nblk if k.startswith("block") else case.S_kv) for k in KINDS}
    found = {k: np.zeros(shape[k], np.int8) for k in KINDS}
    old = {k: np.zeros(shape[k], np.int8) for k in KINDS}

    probed = np.zeros(case.S, bool)  # mutants live on the rows some sparse phase probes (the long bands' phases leave rows out)
    for phase in case.phases()[:-1]:
        probed[case.probe_rows(phase)] = True

    def mark(arr, b, g, rows, keys, flag):
        arr[b, g, rows, keys] = np.maximum(arr[b, g, rows, keys], 1 + flag.astype(np.int8))

    for phase in case.phases():
        dO = abc.phase_dO(case, x["dO"], phase)
        ref, (bQ, bK, bV), _ = orc.sel_attention_bwd_bound(x["Q"], x["K"], x["V"], x["ranges"], dO, dtype, probe_only=True)
        bars = tuple(max(1.0, float(np.abs(r).max())) for r in ref) if phase is None else None
        for c in orc.sel_attention_bwd_terms(x["Q"], x["K"], x["V"], x["ranges"], dO, dtype, extend=True, probe_only=True):
            if "ar" not in c:
                continue
            vk, dq, ok_old = _chunk_detect(c, bQ, bK, bV, bars)
            b, g, cols, cnt = c["b"], c["g"], c["cols"], c["cnt"][c["ar"]]
            rows = c["rows"][c["ar"]]
            cov = cnt > 0
            pr = probed[rows][:, None]
            adj = (np.diff(cols) == 1)[None]
            left = np.concatenate([np.zeros((cov.shape[0], 1), bool), cov[:, :-1] & adj], axis=1)
            right = np.concatenate([cov[:, 1:] & adj, np.zeros((cov.shape[0], 1), bool)], axis=1)
            # first / last key of a range that no other range covers = a covered key with an uncovered neighbour, and the other way round
            sel = {"edge_drop": cov & ~(left & right) & (cnt == 1), "edge_add": ~cov & (left | right), "twice": cnt >= 2}
            for kind, m in sel.items():
                a, k = np.nonzero(m & pr)
                mark(found[kind], b, g, rows[a], cols[k], vk[a, k] | dq[a, k])
                if ok_old is not None:
                    mark(old[kind], b, g, rows[a], cols[k], ok_old[a, k])
            blk = cols // 64
            for j in np.unique(blk):
                c0, c1 = np.searchsorted(blk, j), np.searchsorted(blk, j, side="right")
                covb = cov[:, c0:c1]
                for kind, m in (("block_drop", covb), ("block_full", ~covb)):
                    touched = np.nonzero(covb.any(axis=1) & m.any(axis=1) & pr[:, 0])[0]
                    if not touched.size:
                        continue
                    dqb = np.abs(np.einsum("rhc,cd->rhd", c["dS"][touched][:, :, c0:c1] * m[touched][:, None, :], c["Kc"][c0:c1]))
                    hit = (vk[touched, c0:c1] & m[touched]).any(axis=1) | (dqb > bQ[b, rows[touched], g]).any(axis=(1, 2))
                    mark(found[kind], b, g, rows[touched], int(j), hit)
    return found, old


@pytest.mark.parametrize("name", list(abc.CASES))
def test_every_single_term_mutant_leaves_the_bound(orc, name):
    """Power of the GPU test on this case's inputs (bf16, D = 64).  A dropped (row, 64-key block) contribution and a partly covered block
    taken as fully covered must ALWAYS leave the bound; a dropped first / last key of a range, an added key just outside one and a key
    counted once per covering range must do so for at least 99 % of the mutants.  The older criterion's acceptance of the same mutants
    (dense dO, 3e-2 max-norm) is printed beside it."""
    case = abc.CASES[name]
    x = abc.inputs(name, "bf16", 64)
    if case.B * case.G > 4:  # the long bands: every (b, g) is an independent problem of the same kind; two of the eight keep this test short
        case = dataclasses.replace(case, B=1, G=2)
        x = {k: np.ascontiguousarray(v[:1, :, :2] if k in ("Q", "dO", "ranges") else v[:1, :2]) for k, v in x.items()}
    found, old = _mutants(case, x, orc)
    fails = []
    for kind in KINDS:
        n, hit = int((found[kind] > 0).sum()), int((found[kind] == 2).sum())
        missed = [tuple(int(v) for v in i) for i in np.argwhere(found[kind] == 1)[:20]]
        n_old, acc = int((old[kind] > 0).sum()), int((old[kind] == 2).sum())
        print(f"{name} {kind}: {hit} of {n} mutants leave the bound" + (f"; missed (b, g, row, key or block) {missed}" if missed else "")
              + (f"; the 3e-2 max-norm bar accepts {acc} of {n_old} ({100.0 * acc / n_old:.0f} %)" if n_old else ""))
        need = n if kind.startswith("block") else 0.99 * n
        if hit < need:
            fails.append((kind, hit, n))
    assert not fails, fails
