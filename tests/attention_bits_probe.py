"""The MFMA attention kernels that walk K/V in 32- or 64-key tiles, bit for bit: runs a fixed table of cases on the native library that
NSA_HIP_LIB names (default: the product) and writes the raw bit patterns of every output to an .npz.

    python tests/attention_bits_probe.py OUT.npz          # run every case, write OUT.npz
    python tests/attention_bits_probe.py --list           # construct every case's inputs on the CPU and print the table (no device)
    python tests/attention_bits_probe.py --routes         # one line per case for tools/attn_route_names.cpp (entry point, shape, switches)
    python tests/attention_bits_probe.py --check-routes F # that program's answer against the kernel named next to each case

tests/golden/attention_bits.npz was recorded with this script from the library of the commit before the kernels' K/V tile plumbing moved into
attn_mfma_tiles.hpp (built beside the product, loaded through NSA_HIP_LIB); it was recorded twice and an array is kept only where both
recordings agree.  tests/test_hip_attention_bits.py requires the product to reproduce every stored array exactly.  Inputs come from numpy
PCG64 streams rounded to bf16-representable values (the tests/golden_inputs.py recipe); the stored form is that of
tests/projection_bits_probe.py with BIG = 64 (first and last 32 elements + SHA-256 of all bytes).

What every case has: a K/V whose last tile is partial (S_kv = 203, 600, 1100, ...: no multiple of 32 or 64), h = 6 and h = 16 (unused MFMA
columns and slots), bf16 and f16, D = 64 and 128 where the kernel has both, and K/V that are slices [..., :D] of a cache D + 32 wide (row
stride != row bytes) -- except the block form, whose route takes contiguous rows only (sel_attn_blocks_nt: kss == 64), and the layer decode
step, whose caches are the module's own.  The kernel next to each case is the instance its route launches; where the shape decides
(R = B S G >= 1024 keeps the selection forward off the split-KV form, the band plan's 2048 / 1024 group thresholds) the table says so.
The names were confirmed without a GPU: tools/attn_route_names.cpp calls the case's entry point with its shape and switches against HIP
calls it answers itself and prints the template instance, map_mode and selector instance of every launch; --check-routes found all 183
cases (every group but the layer decode step, whose route tests/test_dispatch_host.py pins) as the table names them.

Backward arrays are kept where two recordings on the parent library agree; they agreed on every one (the dK / dV partial sums of
bwd_dkdv_kernel are reduced in a fixed order), so NOT_REPRODUCIBLE is empty."""
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

BIG = 64
PAD = 32  # elements between the rows of a K/V view beyond D
T = {"bf16": "__bf16", "fp16": "_Float16"}
DTS = ("bf16", "fp16")
SWITCHES = ("SEL_ROWS", "ATTN_MAP", "ATTN_STAGE", "BAND_STAGE", "SEL_BLOCKS", "SEL_ROWSUM", "SEL_FUSE", "SEL_FLAT", "SEL_KSPLIT", "SEL_KSPLIT_T1",
            "SEL_KSPLIT_T2", "DECODE_BAND")
DEFAULTS = {"ATTN_STAGE": 1, "BAND_STAGE": 1, "SEL_ROWSUM": 1, "SEL_FUSE": 0}  # nsa_common.hpp TUNE_TABLE; every other switch: -1
# backward arrays (keys of the fixture) that two recordings on the parent library did not reproduce
NOT_REPRODUCIBLE = ()


def tf(x):
    return "true" if x else "false"


def cand(S_sel):
    """candidates per lane of the fused selector (fused_select_args)"""
    return next(c for c in (1, 2, 4, 8, 16) if (S_sel + 63) // 64 <= c)


def case(group, name, kernel, sw=None, **kw):
    return types.SimpleNamespace(group=group, name=name, kernel=kernel, sw=sw or {}, **kw)


def sel_cases():
    """selection forward: [B,S,G] rows x n = 5 ranges over S_kv keys"""
    out = []
    # the one-row kernel (SEL_ROWS 0): R = 4 128 2 = 1024 rows (>= 1024: no split-KV), B G = 8 so ATTN_MAP 2 is whole pairs per XCD
    for dt, D in itertools.product(DTS, (64, 128)):
        for stage, mp in itertools.product((0, 1), (0, 1, 2)):
            h = 6 if (stage + mp) % 2 == 0 else 16
            out.append(case("one_row", f"{dt}/D{D}/h{h}/stage{stage}_map{mp}", f"sel_attn_fwd_mfma_kernel<{T[dt]}, {D}, false, {stage}> map_mode {mp}",
                            dict(SEL_ROWS=0, ATTN_STAGE=stage, ATTN_MAP=mp), dt=dt, D=D, h=h, B=4, S=128, G=2, S_kv=203, wide=True, lse=True))
    # its split-KV form: R = 6 rows (16 splits) with the log-sum-exp wanted (S = 1 without it is the decode workgroup kernel's)
    for dt, D, h, stage in itertools.product(DTS, (64, 128), (6, 16), (0, 1)):
        out.append(case("split", f"{dt}/D{D}/h{h}/stage{stage}", f"sel_attn_fwd_mfma_kernel<{T[dt]}, {D}, true, {stage}> + sel_attn_combine_kernel<{T[dt]}, {D}>",
                        dict(ATTN_STAGE=stage), dt=dt, D=D, h=h, B=1, S=3, G=2, S_kv=203, wide=True, lse=True))
    # the rows form, forced: SEL_ROWS 1 = pairs of rows (NT 1; h = 16 has one row per tile and stays on the one-row kernel), 3 = 48 / h rows (NT 3)
    for dt, (D, h, mode, B, S, G), rs in itertools.product(DTS, ((64, 6, 1, 4, 131, 2), (64, 6, 3, 1, 347, 3), (64, 16, 3, 4, 131, 2), (128, 6, 1, 1, 347, 3)),
                                                          (0, 1)):
        out.append(case("rows", f"{dt}/D{D}/h{h}/nt{mode}_rs{rs}/B{B}G{G}", f"sel_attn_rows_mfma_kernel<{T[dt]}, {D}, {mode}, {tf(rs)}> map_mode {2 if B * G % 8 == 0 else 1}",
                        dict(SEL_ROWS=mode, SEL_ROWSUM=rs), dt=dt, D=D, h=h, B=B, S=S, G=G, S_kv=203, wide=True, lse=True))
    # the block form (D = 64, contiguous rows): SEL_BLOCKS 1 / 2 / 4, the flat layout (h = 6), the key split (zones at rows 256 and 768 of 1100)
    for dt, h, nt, rs in itertools.product(DTS, (6, 16), (1, 2, 4), (0, 1)):
        out.append(case("blocks", f"{dt}/h{h}/nt{nt}_rs{rs}", f"sel_attn_blocks_mfma_kernel<{T[dt]}, {nt}, {tf(rs)}, false, false>",
                        dict(SEL_BLOCKS=nt, SEL_ROWSUM=rs, SEL_FLAT=0, SEL_KSPLIT=0), dt=dt, D=64, h=h, B=4, S=131, G=2, S_kv=203, wide=False, lse=True))
    for dt, rs in itertools.product(DTS, (0, 1)):
        out.append(case("blocks", f"{dt}/h6/flat_rs{rs}", f"sel_attn_blocks_mfma_kernel<{T[dt]}, 3, {tf(rs)}, true, false>",
                        dict(SEL_ROWSUM=rs, SEL_FLAT=1, SEL_KSPLIT=0), dt=dt, D=64, h=6, B=4, S=131, G=2, S_kv=203, wide=False, lse=True))
    for dt, h, rs in itertools.product(DTS, (6, 16), (0, 1)):
        out.append(case("blocks", f"{dt}/h{h}/ksplit_rs{rs}",
                        f"sel_attn_blocks_mfma_kernel<{T[dt]}, 4, {tf(rs)}, false, true> + sel_attn_ksplit_combine_kernel<{T[dt]}>",
                        dict(SEL_ROWSUM=rs, SEL_FLAT=0, SEL_KSPLIT=1, SEL_KSPLIT_T1=256, SEL_KSPLIT_T2=768), dt=dt, D=64, h=h, B=1, S=1100, G=2, S_kv=1100,
                        wide=False, lse=True))
    return out


def fuse_cases():
    """select + attend with the selector inside the attention kernel (SEL_FUSE 1; SEL_ROWSUM at its default 1), in the three forms that carry it.  p_grp is S_sel wide, and
    the width picks the selector instance (1 / 2 / 4 / 8 / 16 candidates per lane for S_sel <= 64 / 128 / 256 / 512 / 1024); the 600 rows are
    the last ones of a context of 64 S_sel + 7 keys, so the top 6 are picked among (nearly) S_sel candidate blocks.  R = 1 600 2 = 1200 rows;
    SEL_KSPLIT 0 because the key split (automatic from 32k keys on) has no fused selector"""
    out = []
    forms = (("one_row", dict(SEL_ROWS=0, ATTN_STAGE=1), "sel_attn_fwd_mfma_kernel<{T}, {D}, false, 1>", True),
             ("rows", dict(SEL_ROWS=1), "sel_attn_rows_mfma_kernel<{T}, {D}, 1, true>", True),
             ("rows3", dict(SEL_ROWS=3), "sel_attn_rows_mfma_kernel<{T}, {D}, 3, true>", True),
             ("blocks", dict(SEL_FLAT=0, SEL_KSPLIT=0), "sel_attn_blocks_mfma_kernel<{T}, 4, true, false, false>", False),
             ("flat", dict(SEL_FLAT=1, SEL_KSPLIT=0), "sel_attn_blocks_mfma_kernel<{T}, 3, true, true, false>", False))
    for (form, sw, kern, wide), (i, S_sel) in itertools.product(forms, enumerate((10, 100, 200, 400, 1000))):
        dt = DTS[i % 2]
        h = 6 if form in ("rows", "flat") else (6, 16)[(i // 2) % 2]
        D = 128 if form in ("one_row", "rows") and S_sel in (10, 400) else 64
        mode = ("batched", "sequential")[i % 2]
        out.append(case("fuse", f"{form}/{dt}/D{D}/h{h}/S_sel{S_sel}_{mode}", kern.format(T=T[dt], D=D) + f" select_topn_row_regs<{cand(S_sel)}>",
                        dict(SEL_FUSE=1, **sw), dt=dt, D=D, h=h, B=1, S=600, G=2, S_kv=64 * S_sel + 7, S_sel=S_sel, mode=mode, wide=wide))
    return out


def band_cases():
    """band forward (sliding: w = 100 behind t0 + t; compressed: l = 32, d = 16).  band_plan: B G ceil(S / (16 NTW / h)) >= 2048 groups take NTW
    column tiles (3 at D = 64, 2 at D = 128), fewer take 1, and under 1024 groups of 16 / h rows the keys are split"""
    shapes = []  # (D, h, B, S, G, t0, NT, split, stage)
    for D, h in itertools.product((64, 128), (6, 16)):
        ntw = 3 if D == 64 else 2
        tpw3, tpw1 = 16 * ntw // h, 16 // h
        shapes.append((D, h, 4, 256 * tpw3, 2, 37, ntw, False, 1))
        if D == 64:
            shapes.append((D, h, 4, 256 * tpw3, 2, 37, ntw, False, 0))
        shapes.append((D, h, 4, 130 * tpw1 + 1, 2, 37, 1, False, 1))
        shapes.append((D, h, 1, 5, 2, 600, 1, True, 1))
    out = []
    for dt, (D, h, B, S, G, t0, nt, split, stage), kind in itertools.product(DTS, shapes, ("win", "cmp")):
        if kind == "cmp" and h == 16 and not split:
            continue  # (the compressed band differs from the sliding one in its interval only: one h per plain instance)
        band = dict(t0=t0, a=0, dd=1, c=0, w=100) if kind == "win" else dict(t0=t0, a=32, dd=16, c=1, w=2 ** 30)
        S_kv = t0 + S if kind == "win" else (t0 + S - 32) // 16 + 1
        kern = f"band_attn_fwd_kernel<{T[dt]}, {D}, {nt}, {tf(split)}, {stage}>" + (f" + sel_attn_combine_kernel<{T[dt]}, {D}>" if split else "")
        out.append(case("band", f"{kind}/{dt}/D{D}/h{h}/nt{nt}_split{int(split)}_stage{stage}", kern, dict(BAND_STAGE=stage), dt=dt, D=D, h=h, B=B, S=S, G=G,
                        S_kv=S_kv, band=band, wide=True, lse=True))
    return out


def bwd_cases():
    """MFMA backward (bwd_variant 2) of the selection (rows of a wave share the tiles when 16 / h >= 2: bwd_dq_rows_kernel; else, or with
    SEL_ROWS 0, bwd_dq_kernel) and of the band (band_attn_bwd_dq_kernel: 3 column tiles at D = 64 from 2048 groups on, else 1); dK / dV of
    both come from bwd_dkdv_kernel"""
    out = []
    for dt, D, (h, rows, B, S, G) in itertools.product(DTS, (64, 128), ((6, -1, 4, 131, 2), (6, 0, 1, 347, 3), (16, -1, 4, 131, 2))):
        k = "bwd_dq_rows_kernel" if (h == 6 and rows < 0) else "bwd_dq_kernel"
        out.append(case("bwd", f"sel/{dt}/D{D}/h{h}/rows{rows}", f"{k}<{T[dt]}, {D}> map_mode {2 if B * G % 8 == 0 else 1} + bwd_dkdv_kernel<{T[dt]}, {D}>",
                        dict(SEL_ROWS=rows), dt=dt, D=D, h=h, B=B, S=S, G=G, S_kv=203, wide=True))
    for dt, (D, h, B, S, G, nt) in itertools.product(DTS, ((64, 6, 4, 2048, 2, 3), (64, 6, 1, 301, 3, 1), (64, 16, 4, 131, 2, 1), (128, 6, 4, 301, 2, 1))):
        out.append(case("bwd", f"band/{dt}/D{D}/h{h}/nt{nt}", f"band_attn_bwd_dq_kernel<{T[dt]}, {D}, {nt}> map_mode {2 if B * G % 8 == 0 else 1} + bwd_dkdv_kernel<{T[dt]}, {D}>",
                        {}, dt=dt, D=D, h=h, B=B, S=S, G=G, S_kv=37 + S, band=dict(t0=37, a=0, dd=1, c=0, w=100), wide=True))
    return out


def decode_cases():
    """the band inside the layer decode step (DECODE_BAND default: the sliding and the compressed branch ride on the step's launch):
    NSAAttention(768, 12, 2, 64, 64, l 32, d 16, l' 64, n 16, w 512), prefill of 607 tokens, two steps"""
    return [case("decode", f"{dt}/B{B}", f"decode_step_kernel: band_attn_body<{T[dt]}, 64, 1, true, 1>", {}, dt=dt, B=B) for dt, B in (("bf16", 2), ("fp16", 3))]


DECODE_PREFILL, DECODE_STEPS = 607, 2
GROUPS = {"one_row": sel_cases, "split": sel_cases, "rows": sel_cases, "blocks": sel_cases, "fuse": fuse_cases, "band": band_cases, "bwd": bwd_cases,
          "decode": decode_cases}


def cases(group):
    return [c for c in GROUPS[group]() if c.group == group]


# ---- inputs (CPU) ------------------------------------------------------------------------------------------------------------------------
def vals(*shape, key, scale=1.0):
    return _bf16_round(randn(_rng(41, *key), *shape) * np.float32(scale))


def qkv_inputs(c):
    """Q [B,S,G,h,D] and the K / V caches [B,G,S_kv,D (+ PAD)]: shared by the cases of one shape"""
    key = (c.B, c.S, c.G, c.h, c.D, c.S_kv)
    Dw = c.D + (PAD if c.wide else 0)
    return vals(c.B, c.S, c.G, c.h, c.D, key=(1, *key)), vals(c.B, c.G, c.S_kv, Dw, key=(2, *key)), vals(c.B, c.G, c.S_kv, Dw, key=(3, *key))


def range_inputs(c, n=5):
    """n ranges per row: a whole 64-key block, a whole 32-key tile, two unaligned spans (one may reach past S_kv: clamped), and for every third row
    the tail of K/V; every fifth row selects nothing"""
    r = _rng(41, 4, c.B, c.S, c.G, c.S_kv)
    shape = (c.B, c.S, c.G)
    rg = np.zeros(shape + (n, 2), np.int64)
    rg[..., 0, 0] = 64 * r.integers(0, max(1, c.S_kv // 64), shape)
    rg[..., 0, 1] = rg[..., 0, 0] + 64
    rg[..., 1, 0] = 32 * r.integers(0, max(1, c.S_kv // 32), shape)
    rg[..., 1, 1] = rg[..., 1, 0] + 32
    for i in (2, 3):
        rg[..., i, 0] = r.integers(0, c.S_kv, shape)
        rg[..., i, 1] = rg[..., i, 0] + r.integers(1, 90, shape)
    tail = r.integers(0, 3, shape) == 0
    rg[..., 4, 0] = np.where(tail, c.S_kv - r.integers(1, 40, shape), 0)
    rg[..., 4, 1] = np.where(tail, c.S_kv, 0)
    rg[r.integers(0, 5, shape) == 0] = 0
    return rg.astype(np.int32)


def pgrp_inputs(c):
    return _rng(41, 5, c.B, c.S, c.G, c.S_sel).random((c.B, c.S, c.G, c.S_sel), dtype=np.float32)


def dO_inputs(c):
    return vals(c.B, c.S, c.G, c.h, c.D, key=(6, c.B, c.S, c.G, c.h, c.D))


# ---- runs (device) -----------------------------------------------------------------------------------------------------------------------
class Out(pp.Out):
    def put(self, key, t):
        big, pp.BIG = pp.BIG, BIG
        try:
            super().put(key, t)
        finally:
            pp.BIG = big


@contextlib.contextmanager
def switches(sw):
    """the case's switches set, and every switch back to automatic afterwards: -1, except for ATTN_STAGE, BAND_STAGE, SEL_ROWSUM (default 1) and
    SEL_FUSE (default 0), where -1 would itself force a form.  Every switch is set before the case too, so that nothing an earlier test of the
    process left behind reaches it"""
    from nsa_vibe_amd import _lib

    def reset():
        for k in SWITCHES:
            _lib.set_tuning(k, DEFAULTS.get(k, -1))

    try:
        reset()
        for k, v in sw.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        reset()


def dev_qkv(c):
    import torch

    DT = {"bf16": torch.bfloat16, "fp16": torch.float16}[c.dt]
    Q, K, V = (torch.from_numpy(a).to(DT).cuda() for a in qkv_inputs(c))
    K, V = K[..., :c.D], V[..., :c.D]
    assert (K.stride(2) != c.D) == c.wide and K.data_ptr() % 16 == 0
    return Q, K, V


def run_sel(out, group):
    import torch
    import nsa_vibe_amd as nv

    for c in cases(group):
        Q, K, V = dev_qkv(c)
        rg = torch.from_numpy(range_inputs(c)).cuda()
        with switches(c.sw):
            O, lse = nv.selection_attention_hip(Q, K, V, rg, variant=2, return_lse=True)
            torch.cuda.synchronize()
        out.put(f"{group}/{c.name}/O", O)
        out.put(f"{group}/{c.name}/lse", lse)


def run_fuse(out):
    import torch
    import nsa_vibe_amd as nv

    for c in cases("fuse"):
        Q, K, V = dev_qkv(c)
        p = torch.from_numpy(pgrp_inputs(c)).cuda()
        with switches(c.sw):
            rg, O, lse = nv.select_and_attend(p, Q, K, V, types.SimpleNamespace(l_sel=64), 6, mode=c.mode, t0=c.S_kv - c.S, return_lse=True)
            torch.cuda.synchronize()
        for k, v in (("ranges", rg), ("O", O), ("lse", lse)):
            out.put(f"fuse/{c.name}/{k}", v)


def run_band(out):
    import torch
    import nsa_vibe_amd as nv

    for c in cases("band"):
        Q, K, V = dev_qkv(c)
        with switches(c.sw):
            O, lse = nv.band_attention_hip(Q, K, V, variant=2, return_lse=True, **c.band)
            torch.cuda.synchronize()
        out.put(f"band/{c.name}/O", O)
        out.put(f"band/{c.name}/lse", lse)


def run_bwd(out):
    import torch
    import nsa_vibe_amd as nv

    for c in cases("bwd"):
        Q, K, V = (t.detach().requires_grad_() for t in dev_qkv(c))
        dO = torch.from_numpy(dO_inputs(c)).to(Q.dtype).cuda()
        with switches(c.sw):
            if hasattr(c, "band"):
                O = nv.band_attention_hip(Q, K, V, variant=2, bwd_variant=2, **c.band)
            else:
                O = nv.selection_attention_hip(Q, K, V, torch.from_numpy(range_inputs(c)).cuda(), variant=2, bwd_variant=2)
            O.backward(dO)
            torch.cuda.synchronize()
        for k, v in (("dQ", Q.grad), ("dK", K.grad), ("dV", V.grad)):
            if f"bwd/{c.name}/{k}" not in NOT_REPRODUCIBLE:
                out.put(f"bwd/{c.name}/{k}", v)


def decode_module():
    from nsa_vibe_amd.nsa_attention import NSAAttention

    return NSAAttention(768, 12, 2, 64, 64, l=32, d=16, l_sel=64, n_sel=16, w=512)


def run_decode(out):
    import torch

    for c in cases("decode"):
        DT = {"bf16": torch.bfloat16, "fp16": torch.float16}[c.dt]
        m = pp.load_state(decode_module(), 768, DT)
        x = torch.from_numpy(vals(c.B, DECODE_PREFILL + DECODE_STEPS, 768, key=(7, c.B))).to(DT).cuda()
        with switches({}), torch.no_grad():
            kv = m.new_kv(c.B, DECODE_PREFILL + DECODE_STEPS + 1, "cuda", DT)
            _, kv = m(x[:, :DECODE_PREFILL], kv, prefill=True)
            for s in range(DECODE_STEPS):
                t = DECODE_PREFILL + s
                y, kv = m(x[:, t: t + 1], kv, prefill=False)
                torch.cuda.synchronize()
                out.put(f"decode/{c.name}/step{s}/y", y)
                out.put(f"decode/{c.name}/step{s}/gates", m._last_gates)
        assert m._fallback_counters["total_fallbacks"] == 0


RUN = {"one_row": lambda o: run_sel(o, "one_row"), "split": lambda o: run_sel(o, "split"), "rows": lambda o: run_sel(o, "rows"),
       "blocks": lambda o: run_sel(o, "blocks"), "fuse": run_fuse, "band": run_band, "bwd": run_bwd, "decode": run_decode}


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
            if g == "decode":
                m = decode_module()
                m.load_state_dict({k: __import__("torch").from_numpy(v) for k, v in pp.module_state(m, 768).items()})
                shapes = f"x {vals(c.B, DECODE_PREFILL + DECODE_STEPS, 768, key=(7, c.B)).shape}"
            else:
                Q, K, V = qkv_inputs(c)
                assert Q.shape == (c.B, c.S, c.G, c.h, c.D) and K.shape == V.shape == (c.B, c.G, c.S_kv, c.D + (PAD if c.wide else 0))
                assert c.S_kv % 32 and c.S_kv % 64
                shapes = f"Q {Q.shape} K {K.shape}"
                if g == "fuse":
                    shapes += f" p_grp {pgrp_inputs(c).shape}"
                elif not hasattr(c, "band"):
                    rg = range_inputs(c)
                    assert rg.shape == (c.B, c.S, c.G, 5, 2) and (c.S < 100 or (rg.max() > c.S_kv and (rg[..., 4, 1] == c.S_kv).any()))
                if g == "bwd":
                    assert dO_inputs(c).shape == Q.shape
            print(f"{g}/{c.name}: {shapes} {c.sw}\n    -> {c.kernel}")
            n += 1
    print(f"{n} cases constructed")


def route_lines():
    """one line per case for tools/attn_route_names.cpp: the entry point, the shape and the switches (the decode group goes through the module;
    its route is pinned by the layer_decode_step cases of tests/test_dispatch_host.py)"""
    out = []
    for g in GROUPS:
        for c in cases(g) if g != "decode" else []:
            f = dict(case=f"{g}/{c.name}", dt={"bf16": 1, "fp16": 2}[c.dt], B=c.B, S=c.S, G=c.G, h=c.h, D=c.D, S_kv=c.S_kv, pad=PAD if c.wide else 0, n=5, lse=1)
            if g == "fuse":
                f.update(entry="fuse", S_sel=c.S_sel, mode=int(c.mode == "batched"), t0=c.S_kv - c.S)
            elif hasattr(c, "band"):
                f.update(entry="bandbwd" if g == "bwd" else "band", **{k: min(v, 2 ** 30) for k, v in c.band.items()})
            else:
                f.update(entry="selbwd" if g == "bwd" else "sel")
            sw = {**DEFAULTS, **c.sw}
            out.append(" ".join(f"{k}={v}" for k, v in f.items()) + " sw=" + ",".join(f"{k}:{v}" for k, v in sw.items()))
    return out


def check_routes(path):
    """the output of tools/attn_route_names.cpp against the table: every kernel a case names is launched, with the map_mode and the selector
    instance it names"""
    got = dict(line.rstrip("\n").split("\t") for line in open(path))
    bad = []
    for g in GROUPS:
        for c in cases(g) if g != "decode" else []:
            launched = got.get(f"{g}/{c.name}", "")
            for part in c.kernel.split(" + "):
                name = part[:part.index(">") + 1]
                hit = [k for k in launched.split(" | ") if k.startswith(name)]
                ok = bool(hit)
                if ok and " map_mode " in part:
                    ok = f"map_mode={part.split(' map_mode ')[1].split()[0]}" in hit[0]
                if ok and "select_topn_row_regs<" in part:
                    ok = f"cand={part.split('select_topn_row_regs<')[1].split('>')[0]}" in hit[0]
                if not ok:
                    bad.append((f"{g}/{c.name}", part, launched))
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
