"""Case table of the attention-backward bound tests (test_attention_bwd_bound_host.py on the CPU, test_hip_attention_bwd_bound.py on the GPU).

Inputs come from numpy PCG64 streams on the host (the recipe of golden_inputs.py): N(0,1) values rounded to the activation dtype.  A case
names its shape, its ranges (or band), a probe stride and its phases: in phase r the upstream gradient dO is zero except on the query rows
t = r (mod stride), and every case has one dense phase (None).  Sparse probes are what makes a single wrong (row, key) term visible: dK and dV
of a key then sum the few probe rows that reach it instead of every row of the sequence.
"""
from dataclasses import dataclass, field

import numpy as np

from oracle import nsa_oracle as orc


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    S: int
    G: int
    h: int
    S_kv: int
    n: int = 1
    stride: int = 8
    residues: tuple = None          # probe phases (None: every residue of the stride); the dense phase is added to all
    band: dict = field(default=None)  # band_ranges arguments (a, dd, c, w) of a band case, None for a selection case
    maker: str = "unaligned"        # how the ranges of a selection case are drawn (see _ranges)
    width: int = 90

    def phases(self):
        res = range(self.stride) if self.residues is None else self.residues
        return [int(r) for r in res] + [None]

    def probe_rows(self, phase):
        return np.arange(self.S) if phase is None else np.arange(phase, self.S, self.stride)


# ---- selection: the smallest shapes at which the MFMA backward takes another path (sel_attn_bwd_mfma.hip) --------------------------------
SEL_CASES = {c.name: c for c in [
    # one split, two 256-row chunks, a partial last key block (44 keys) and hit-map word, the rows form of dQ (16 / h = 2 rows per wave)
    Case("A", 2, 300, 2, 6, 300, 6),
    # dkdv_splits = 2, the second split holds rows 512-519: the reduce kernel and its flags; every hit full but the clamped 8-key last block
    Case("B", 1, 520, 2, 4, 520, 16, maker="aligned"),
    # h = 16: the one-row dQ kernel
    Case("C", 1, 130, 2, 16, 700, 4, stride=16, width=150),
    # rows straddling the 16-slot tiles, rows_per_round = SLOTS / h leaves slots unused
    Case("D5", 2, 100, 2, 5, 200, 4),
    Case("D7", 2, 100, 2, 7, 200, 4),
    Case("D1", 2, 40, 2, 1, 130, 3),
    # the pending list of the dK / dV kernel: 255 pending hits of key block 1 followed by 256 new ones (511 of its 512 entries)
    Case("E", 1, 768, 1, 6, 128, 2, maker="pending"),
    # across key 65536 (second schedule register of the rows dQ kernel) and the partial last tile
    Case("F", 1, 21, 2, 6, 70000, 8, stride=4, maker="long", width=150),
]}

# ---- band (sliding window a = 0, dd = 1, c = 0; compressed a = l, dd = d, c = 1), h = 6 ---------------------------------------------------
_CMP = dict(a=32, dd=16, c=1, w=2 ** 30)
# the long bands probe the residues that hold t = l - 2 (no key), t = l - 1 (first key), the rows with (t + 1 - l) mod d in {0, d - 1}
# (t = 15, 14 mod 16) and the last row (2049 = 1 mod 16)
BAND_CASES = {c.name: c for c in [
    Case("w1", 2, 300, 2, 6, 300, band=dict(a=0, dd=1, c=0, w=1)),
    Case("w33", 2, 300, 2, 6, 300, band=dict(a=0, dd=1, c=0, w=33)),
    Case("w100", 2, 300, 2, 6, 300, band=dict(a=0, dd=1, c=0, w=100)),
    Case("cmp", 2, 600, 2, 6, 36, band=_CMP),
    Case("long_w33", 2, 2050, 4, 6, 2050, stride=16, residues=(1, 14, 15), band=dict(a=0, dd=1, c=0, w=33)),
    Case("long_cmp", 2, 2050, 4, 6, 127, stride=16, residues=(1, 14, 15), band=_CMP),
]}
# ---- selection cases added later: they go behind the bands, because inputs() seeds from a case's position in CASES ------------------------
LATE_CASES = {c.name: c for c in [
    # S < 2 * (16 / h): the one-row dQ kernel on its row-linear grid (12 rows, 3 workgroups of 4 waves, no (b,g)-major map)
    Case("S3", B=2, S=3, G=2, h=6, S_kv=100, n=3, stride=3),
]}
CASES = {**SEL_CASES, **BAND_CASES, **LATE_CASES}


def _rng(*key):
    return np.random.default_rng([23, *key])


def _ranges(case: Case, r) -> np.ndarray:
    B, S, G, n, S_kv = case.B, case.S, case.G, case.n, case.S_kv
    if case.band is not None:
        return orc.band_ranges_rows(B, S, G, S_kv, **case.band)
    rg = np.zeros((B, S, G, n, 2), np.int64)
    if case.maker == "pending":
        rg[:, :, :, 0] = (0, 64)                      # key block 0: every row
        rg[:, :512:2, :, 1] = (64, 128)               # key block 1: rows 0-254 and 256-511, alternately full ...
        rg[:, 1:512:2, :, 1] = (70, 120)              # ... and partial
        rg[:, 255, :, 1] = 0
        return rg.astype(np.int32)
    if case.maker == "long":  # the ranges of test_backward_query_tile_dq_long_context_and_kernel_switch
        st = r.integers(0, S_kv - 200, size=(B, S, G, n))
        rg = np.stack([st, st + r.integers(0, case.width, size=st.shape)], axis=-1)
        rg[0, :, :, 0] = (0, 64)
        rg[0, :, :, 1] = (65500, 65610)  # straddles tile 2047 | 2048
        rg[0, 2, 0] = 0                  # empty row
        rg[0, 5, 1, 2] = (69990, 70000)  # the partial last tile
        return rg.astype(np.int32)
    used = r.integers(0, n + 1, size=(B, S, G))
    if case.maker == "aligned":
        s = r.integers(0, (S_kv + 63) // 64, size=(B, S, G, n)) * 64
        e = np.minimum(S_kv, s + 64 * r.integers(1, 3, size=s.shape))
    else:
        s = r.integers(0, S_kv, size=(B, S, G, n))
        e = np.minimum(S_kv, s + r.integers(0, case.width, size=s.shape))
    rg = np.stack([s, e], axis=-1)
    rg[np.arange(n)[None, None, None, :] >= used[..., None]] = 0
    rg[0, 0, 0] = 0            # an empty row
    rg[0, 1, 0] = 0
    rg[0, 1, 0, 0] = (0, S_kv)  # everything
    return rg.astype(np.int32)


def inputs(name: str, dtype: str = "bf16", Dk: int = 64, Dv: int = None) -> dict:
    """-> dict Q [B,S,G,h,Dk], K [B,G,S_kv,Dk], V [B,G,S_kv,Dv], dO [B,S,G,h,Dv] (float64 values representable in dtype: the dense
    phase's dO), ranges [B,S,G,n,2] int32"""
    c = CASES[name]
    Dv = Dk if Dv is None else Dv
    r = _rng(list(CASES).index(name), Dk, Dv)
    f = lambda *sh: orc.round_to(r.standard_normal(sh, dtype=np.float32), dtype)  # noqa: E731
    out = dict(Q=f(c.B, c.S, c.G, c.h, Dk), K=f(c.B, c.G, c.S_kv, Dk), V=f(c.B, c.G, c.S_kv, Dv), dO=f(c.B, c.S, c.G, c.h, Dv))
    out["ranges"] = _ranges(c, r)
    return out


def phase_dO(case: Case, dO: np.ndarray, phase) -> np.ndarray:
    """dO of one phase: the dense dO on the probe rows, zero elsewhere"""
    if phase is None:
        return dO
    out = np.zeros_like(dO)
    out[:, phase::case.stride] = dO[:, phase::case.stride]
    return out
