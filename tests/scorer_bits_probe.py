"""The two fused MFMA selection scorers (sel_scores_mfma.hip: 16x16x32 tiles; sel_scores_mfma32.hip: 32x32x16 tiles), bit for bit: runs a
fixed table of cases on the native library that NSA_HIP_LIB names (default: the product) and writes the raw bit patterns of every output
to an .npz.

    python tests/scorer_bits_probe.py OUT.npz          # run every case, write OUT.npz
    python tests/scorer_bits_probe.py --list           # construct every case's inputs on the CPU and print the table (no device)
    python tests/scorer_bits_probe.py --routes         # one line per case for tools/attn_route_names.cpp (entry point, shape, switches)
    python tests/scorer_bits_probe.py --check-routes F # that program's answer against the kernel named next to each case

tests/golden/scorer_bits.npz was recorded with this script from the library of the commit before the two kernels' K_cmp staging, sweep bounds
and exact sweep-1 update moved into sel_scores_mfma.hpp (built beside the product, loaded through NSA_HIP_LIB); it was recorded twice and an
array is kept only where both recordings agree (the scorers have no atomics: all of them agreed).  tests/test_hip_scorer_bits.py requires the
product to reproduce every stored array exactly.  Inputs come from numpy PCG64 streams rounded to bf16-representable values (the
tests/golden_inputs.py recipe); the stored form is that of tests/projection_bits_probe.py with BIG = 32 (first and last 16 elements +
SHA-256 of all bytes).

Geometry l / d / l' = 32 / 16 / 64, B = 2, G = 2.  Contexts T = 160 (S_cmp = 9: one partial tile), 3264 (203 = 3 64 + 11: the last tile's
second 32-row half is empty), 3776 (235 = 3 64 + 43: partly filled), 4112 (256: no tail); query rows S = 100, 131 (no multiple of any
workgroup's 16 / 32 / 48 / 64 queries: the last workgroup has absent queries) and 192 as the LAST S rows of T (q0 = T - S), and the whole
sequence at T = 160.  Every instance runs the plain softmax and normalize="causal" (with q0 > 0 the workgroup's column bounds nc_wmin <
nc_wgmax fall inside a tile: the masked-tile arm of both sweeps), bf16 and f16, D = 64 and (16x16 form) 128, on a K_cmp that is a [..., :D]
slice of a cache D + 32 wide; group "contig" has contiguous rows.  Group "skip": causal_skip 0 / 1 through selection_scores and 2 through
the C ABI into a p_grp prefilled with the bit pattern FILL, so the fixture also pins which entries stay unwritten.  Group "big": Q and K_cmp
x 4, and one K_cmp column = 40 Q (most probabilities underflow to exact zero): the `sum > 4096` arm of the first sweep on unpadded tiles.
Group "select": the 32x32 form with the top-n selector in its launch (SCORES_SELECT 1), batched over the whole sequence and sequential over
its last 320 rows, n_top = 16; ranges stored with the scores.

The kernel next to each case is the instance its route launches (SCORES_FORM pins the form; variant 2 keeps B S G <= 1024 rows off the
decode-shaped pair).  The names were confirmed without a GPU: tools/attn_route_names.cpp (the host route check of csrc/dispatch_check.cpp
that also prints template instances) calls each case's entry point with its shape and switches against HIP calls it answers itself;
--check-routes found every case as the table names it."""
import contextlib
import itertools
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import projection_bits_probe as pp  # noqa: E402
from golden_inputs import _bf16_round, _rng, randn  # noqa: E402

BIG = 32
PAD = 32  # elements between the rows of a K_cmp view beyond D
B, G, L, DSTRIDE, LSEL, NTOP = 2, 2, 32, 16, 64, 16
FILL = 0x7FC12345  # a NaN payload no kernel produces
T_ = {"bf16": "__bf16", "fp16": "_Float16"}
DTS = ("bf16", "fp16")
# instance -> (h, SCORES_FORM, queries per workgroup, kernel template)
INSTANCES = {
    "nt4_h6": (6, 0, 32, "scores_mfma_kernel<{T}, {D}, 4, 6, {N}>"),
    "flat_h6": (6, 1, 32, "scores_mfma_kernel<{T}, {D}, 3, 6, {N}>"),
    "h4": (4, -1, 64, "scores_mfma_kernel<{T}, {D}, 4, 4, {N}>"),
    "h8": (8, -1, 32, "scores_mfma_kernel<{T}, {D}, 4, 8, {N}>"),
    "h16": (16, -1, 16, "scores_mfma_kernel<{T}, {D}, 4, 0, {N}>"),
    "h5": (5, -1, 48, "scores_mfma_kernel<{T}, {D}, 4, 0, {N}>"),
    "mfma32": (6, 2, 64, "scores_mfma32_kernel<{T}, {SEL}, {N}>"),
}
# (T, S, q0): the last S rows of T, and the whole sequence at T = 160
SHAPES = [(160, 160, 0), (160, 100, 60), (160, 131, 29)] + [(T, S, T - S) for T in (3264, 3776, 4112) for S in (100, 131, 192)]
NORMS = ("all", "causal")
GROUPS = tuple(INSTANCES) + ("skip", "contig", "big", "select")


def tf(x):
    return "true" if x else "false"


def s_cmp(T):
    return (T - L) // DSTRIDE + 1


def case(group, name, inst, **kw):
    h, form = INSTANCES[inst][:2]
    return types.SimpleNamespace(group=group, name=name, inst=inst, h=h, form=form, wide=True, skip=0, kind="plain", sel=None, **kw)


def kernel_of(c):
    return INSTANCES[c.inst][3].format(T=T_[c.dt], D=c.D, N=tf(c.norm == "causal"), SEL=tf(c.sel is not None))


def cases(group):
    out = []
    if group in INSTANCES:
        for dt, D, norm, (T, S, q0) in itertools.product(DTS, (64,) if group == "mfma32" else (64, 128), NORMS, SHAPES):
            out.append(case(group, f"{dt}/D{D}/{norm}/T{T}_S{S}", group, dt=dt, D=D, norm=norm, T=T, S=S, q0=q0))
    elif group == "skip":
        for inst, norm, skip, (T, S, q0) in itertools.product(INSTANCES, NORMS, (1, 2), ((160, 160, 0), (3264, 131, 3133), (4112, 192, 3920))):
            c = case(group, f"{inst}/{norm}/skip{skip}/T{T}_S{S}", inst, dt="bf16", D=64, norm=norm, T=T, S=S, q0=q0)
            c.skip = skip
            out.append(c)
    elif group == "contig":
        for inst, norm in itertools.product(INSTANCES, NORMS):
            c = case(group, f"{inst}/{norm}/T3776_S131", inst, dt="fp16", D=64, norm=norm, T=3776, S=131, q0=3776 - 131)
            c.wide = False
            out.append(c)
    elif group == "big":
        for inst, kind in itertools.product(INSTANCES, ("x4", "col40")):
            c = case(group, f"{inst}/{kind}/T4112_S192", inst, dt="bf16", D=64, norm="all", T=4112, S=192, q0=4112 - 192)
            c.kind = kind
            out.append(c)
    elif group == "select":
        for dt, norm, T, mode in itertools.product(DTS, NORMS, (3264, 4112), ("batched", "sequential")):
            S = T if mode == "batched" else 320
            c = case(group, f"{dt}/{norm}/{mode}/T{T}_S{S}", "mfma32", dt=dt, D=64, norm=norm, T=T, S=S, q0=T - S)
            c.sel = mode
            out.append(c)
    return out


# ---- inputs (CPU) ------------------------------------------------------------------------------------------------------------------------
def vals(*shape, key, scale=1.0):
    return _bf16_round(randn(_rng(51, *key), *shape) * np.float32(scale))


_cache = {}


def inputs(c):
    """Q [B,S,G,h,D] and the K_cmp cache [B,G,S_cmp,D (+ PAD)] of a case (fp32 arrays of bf16-representable values), shared by the cases of one
    shape.  x4: both scaled by 4 (logits far apart); col40: compressed token 5 of every (b,g) = 40 x the first head's query of row 0"""
    key = (c.S, c.h, c.D, c.T, c.wide, c.kind)
    if key not in _cache:
        Q = vals(B, c.S, G, c.h, c.D, key=(1, c.S, c.h, c.D))
        Kc = vals(B, G, s_cmp(c.T), c.D + (PAD if c.wide else 0), key=(2, c.T, c.D, int(c.wide)))
        if c.kind == "x4":
            Q, Kc = Q * np.float32(4), Kc * np.float32(4)
        elif c.kind == "col40":
            Kc = Kc.copy()
            Kc[:, :, 5, :c.D] = _bf16_round(np.float32(40) * Q[:, 0, :, 0, :])
        _cache[key] = (Q, Kc)
    return _cache[key]


# ---- runs (device) -----------------------------------------------------------------------------------------------------------------------
class Out(pp.Out):
    def put(self, key, t):
        super().put(key, t, big=BIG)


@contextlib.contextmanager
def switches(c):
    """SCORES_FORM / SCORES_SELECT of the case, and both back to automatic (-1) afterwards"""
    from nsa_vibe_amd import _lib

    try:
        _lib.set_tuning("SCORES_FORM", c.form)
        _lib.set_tuning("SCORES_SELECT", 1 if c.sel else -1)
        yield
    finally:
        _lib.set_tuning("SCORES_FORM", -1)
        _lib.set_tuning("SCORES_SELECT", -1)


_dev = {}


def dev_inputs(c):
    import torch

    key = (c.S, c.h, c.D, c.T, c.wide, c.kind, c.dt)
    if key not in _dev:
        DT = {"bf16": torch.bfloat16, "fp16": torch.float16}[c.dt]
        Q, Kc = (torch.from_numpy(a).to(DT).cuda() for a in inputs(c))
        Kc = Kc[..., :c.D]
        assert (Kc.stride(2) != c.D) == c.wide and Kc.data_ptr() % 16 == 0
        _dev[key] = (Q, Kc)
    return _dev[key]


def scores_cabi(Q, Kc, meta, c):
    """nsa_sel_scores_rows (variant 2) with the case's causal_skip into a p_grp prefilled with FILL"""
    import torch
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd._native import _DT, _stream

    p = torch.full((B, c.S, G, meta.S_sel), FILL, dtype=torch.int32, device=Q.device)
    cptr, crows, cvals = meta.device_csc(Q.device)
    rc = _lib.lib().nsa_sel_scores_rows(Q.data_ptr(), Kc.data_ptr(), p.data_ptr(), B, c.S, G, c.h, c.D, Kc.shape[2], Kc.stride(0), Kc.stride(1), Kc.stride(2),
                                        cptr.data_ptr(), crows.data_ptr(), cvals.data_ptr(), meta.S_sel, L, DSTRIDE, LSEL, c.skip, 2, _DT[Q.dtype], 0.0,
                                        c.q0, int(c.norm == "causal"), None, 0, _stream(Q.device))
    _lib.check(rc, "nsa_sel_scores_rows")
    return p.view(torch.float32)


def run_group(out, group):
    import torch
    import nsa_vibe_amd as nv

    _cache.clear(), _dev.clear()  # (inputs are shared inside a group)
    for c in cases(group):
        Q, Kc = dev_inputs(c)
        meta = nv.build_block_meta(c.T, L, DSTRIDE, LSEL, NTOP, 512)
        assert Kc.shape[2] == meta.S_cmp
        with switches(c):
            if c.sel:
                p, rg = nv.selection_scores_select(Q, Kc, meta, NTOP, mode=c.sel, t0=c.q0, normalize=c.norm, leave_skipped=False)
                out.put(f"{group}/{c.name}/ranges", rg)
            elif c.skip == 2:
                p = scores_cabi(Q, Kc, meta, c)
            else:
                p = nv.selection_scores(Q, Kc, meta, causal_skip=bool(c.skip), variant=2, q0=c.q0, normalize=c.norm)
            torch.cuda.synchronize()
        out.put(f"{group}/{c.name}/p_grp", p)


RUN = {g: (lambda o, g=g: run_group(o, g)) for g in GROUPS}


def run_cases():
    out = Out()
    for g in RUN:
        RUN[g](out)
    return out


def list_cases():
    """every input builder, on the CPU: the case table with the kernel each case is meant for"""
    n = 0
    for g in GROUPS:
        for c in cases(g):
            Q, Kc = inputs(c)
            assert Q.shape == (B, c.S, G, c.h, c.D) and Kc.shape == (B, G, s_cmp(c.T), c.D + (PAD if c.wide else 0))
            assert c.q0 + c.S == c.T
            print(f"{g}/{c.name}: Q {Q.shape} K_cmp {Kc.shape} q0 {c.q0} causal_skip {c.skip} SCORES_FORM {c.form}\n    -> {kernel_of(c)}")
            n += 1
    print(f"{n} cases constructed")


def route_lines():
    """one line per case for tools/attn_route_names.cpp"""
    out = []
    for g in GROUPS:
        for c in cases(g):
            f = dict(case=f"{g}/{c.name}", entry="scoresel" if c.sel else "scores", dt={"bf16": 1, "fp16": 2}[c.dt], B=B, S=c.S, G=G, h=c.h, D=c.D, S_kv=s_cmp(c.T),
                     pad=PAD if c.wide else 0, S_sel=-(-c.T // LSEL), skip=1 if c.sel else c.skip, t0=c.q0, norm=int(c.norm == "causal"),
                     mode=int(c.sel == "batched"))
            out.append(" ".join(f"{k}={v}" for k, v in f.items()) + f" sw=SCORES_FORM:{c.form},SCORES_SELECT:{1 if c.sel else -1}")
    return out


def check_routes(path):
    got = dict(line.rstrip("\n").split("\t") for line in open(path))
    bad = [(f"{g}/{c.name}", kernel_of(c), got.get(f"{g}/{c.name}")) for g in GROUPS for c in cases(g) if got.get(f"{g}/{c.name}") != kernel_of(c)]
    for b in bad:
        print("MISMATCH", *b, sep="\n    ")
    print(f"{len(got)} routes read, {len(bad)} mismatches")
    return not bad


if __name__ == "__main__":
    if sys.argv[1:] == ["--list"]:
        list_cases()
    elif sys.argv[1:] == ["--routes"]:
        print("\n".join(route_lines()))
    elif sys.argv[1:2] == ["--check-routes"]:
        sys.exit(0 if check_routes(sys.argv[2]) else 1)
    else:
        res = run_cases()
        np.savez_compressed(sys.argv[1], **res)
        print(f"{len(res)} arrays, {os.path.getsize(sys.argv[1])} bytes -> {sys.argv[1]}")
