"""The one-launch decode step of the selected branch (sel_decode_fused.hip: decode_step_kernel in every form, decode_step_onepass_kernel and
the band workgroups behind them), bit for bit: runs a fixed table of cases on the native library that NSA_HIP_LIB names (default: the
product) and writes the raw bit patterns of O and ranges to an .npz.

    python tests/decode_bits_probe.py OUT.npz          # run every case, write OUT.npz
    python tests/decode_bits_probe.py --list           # construct every case's inputs on the CPU and print the table (no device)

tests/golden/decode_step_bits.npz was recorded with this script from the library of the commit before the two kernel templates' shared phases
(LDS map, forced-block prefetch, per-head log-sum-exp, stencil taps, head sum, selector call, chunk MFMA loop) and the launchers' kernel
table were written once (built beside the product, loaded through NSA_HIP_LIB); it was recorded twice and an array is kept only where both
recordings agree.  All of them agreed, the team form included: its tickets decide who finishes a row, never what is summed in which order.
tests/test_hip_decode_bits.py requires the product to reproduce every stored array exactly.  Inputs come from numpy PCG64 streams rounded to
bf16-representable values (the tests/golden_inputs.py recipe); the stored form is that of tests/projection_bits_probe.py with BIG = 64
(first and last 32 elements + SHA-256 of all bytes).

Geometry l / d / l' = 32 / 16 / 64, G = 2, n_top = 16, B G <= 4 except the mixed-position batches taken from the parity tests.  Every case
asks the library's plan first and requires one launch in the form named here, so a case cannot drift onto another kernel unnoticed.
  step     form 0 unsplit, selection_decode_step at t = 200 (S_cmp = 11: the tail mask of a partial chunk) in bf16 / f16, D = 64 / 128,
           h = 6 (HC = 6) / h = 4 (HC = 0), and at t = 1039 (S_cmp = 64: a full chunk, no tail).  The row with t < 31 (no compressed row)
           is the slot at t = 9 of the ragged cases.
  team     form 0 as a team: DECODE_SPLIT = 2 at t = 2047 (S_cmp = 127: two chunks, one per workgroup), D = 64 / 128, and the same with
           DECODE_TEAM_SPIN = 0 (a workgroup that does not find its team complete at its single look forms the missing records itself).
  wide     form 1 (DECODE_WIDE = 1): 16 waves at 33 chunks (t = 32799, S_cmp = 2049) -- the way tests/test_hip_decode_rows.py and
           test_hip_decode_ragged.py reach it -- and, with DECODE_WAVES = 8, 8 waves at 17 chunks (t = 16415, S_cmp = 1025).
  onepass  form 2 (DECODE_WIDE = 2) at t = 2047 on 16 waves and (DECODE_WAVES = 8) on 8, h = 6 / 4.
  rows     selection_decode_rows: t0 = 1052, S = 8 (rows of one and of two chunks; tests/test_hip_decode_rows.py SHAPES[0] at B = 2) at
           D = 64 / 128, and t0 = 32796, S = 8, B = 1 (form 1).
  ragged   selection_decode_ragged: t_pos = [1055, 40, 9, 4100, -1], S = 1 (tests/test_hip_decode_ragged.py "S1_mixed": two chunks, few
           blocks, no compressed token, an empty slot) in bf16 h = 6, f16 h = 6 and bf16 h = 4; [1052, 40, 9000, -1], S = 4 at D = 128;
           [32796, 100, -1], S = 8 (form 1).  Caches poisoned (+-3e4) beyond every sequence's own rows, as in that test.
  paged    selection_decode_paged on the ragged cases' caches scattered into pool pages in a seeded random order (the method of
           tests/test_hip_decode_paged.py).
  long     the long-row form (DECODE_LONG = 1, plan form 3), ragged and paged: D = 128 at [16414, 16415, 40, 9, -1], S = 1 (17 chunks:
           the smallest of tests/test_hip_decode_long.py without its 20-chunk slot); D = 64 at [65567, 40, -1] on 16 waves and at
           [32799, 40] with DECODE_WAVES = 8.
  band     NSAAttention(256, 12 heads, G = 2, d_k = d_v = 64, n_sel = 16, w = 512), B = 2: prefill of 300 tokens, then 3 decode steps
           (S = 1) with the sliding and compressed branches on the step's launch (decode_band_workgroup): DECODE_BAND = 1 (BP.mg.on off:
           splits merged by the finish kernel) and DECODE_BAND = 2 (BP.mg.on: merged by the workgroup that holds them); y, the gates and
           the ranges of the last step are stored."""
import contextlib
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import projection_bits_probe as pp  # noqa: E402
from golden_inputs import _bf16_round, _rng, randn  # noqa: E402

BIG = 64
G, N_TOP, L, DSTRIDE, LSEL, W = 2, 16, 32, 16, 64, 512
PAGE = 1024
POISON = 3.0e4
SWITCHES = ("DECODE_SPLIT", "DECODE_TEAM_SPIN", "DECODE_WIDE", "DECODE_WAVES", "DECODE_LONG", "DECODE_BAND")
BAND_CFG, BAND_B, BAND_PREFILL, BAND_STEPS = (256, 12, 2, 64, 64), 2, 300, 3


def ncmp(t):
    return 0 if t + 1 < L else (t + 1 - L) // DSTRIDE + 1


def case(group, name, kind, form, sw=None, nsplit=None, **kw):
    kw = dict(dict(D=64, h=6, dt="bf16", S=1), **kw)
    return types.SimpleNamespace(group=group, name=name, kind=kind, form=form, nsplit=nsplit, sw=sw or {}, **kw)


def _step(group, t, form, sw=None, nsplit=1, **kw):
    c = case(group, "", "step", form, sw, nsplit, t_pos=[t, t], **kw)
    c.name = f"{c.dt}/D{c.D}/h{c.h}/t{t}" + "".join(f"/{k[7:].lower()}{v}" for k, v in c.sw.items())
    return c


def _ragged(group, t_pos, S, form, sw=None, **kw):
    c = case(group, "", "ragged", form, sw, t_pos=list(t_pos), S=S, **kw)
    c.name = f"{c.dt}/D{c.D}/h{c.h}/S{S}_t{max(t_pos)}" + "".join(f"/{k[7:].lower()}{v}" for k, v in c.sw.items() if k != "DECODE_LONG")
    return c


MIXED = [1055, 40, 9, 4100, -1]
RAGGED = [_ragged("ragged", MIXED, 1, 0), _ragged("ragged", MIXED, 1, 0, dt="fp16"), _ragged("ragged", MIXED, 1, 0, h=4),
          _ragged("ragged", [1052, 40, 9000, -1], 4, 0, D=128), _ragged("ragged", [32796, 100, -1], 8, 1)]
LONG = [_ragged("long", [16414, 16415, 40, 9, -1], 1, 3, {"DECODE_LONG": 1}, D=128), _ragged("long", [65567, 40, -1], 1, 3, {"DECODE_LONG": 1}),
        _ragged("long", [32799, 40], 1, 3, {"DECODE_LONG": 1, "DECODE_WAVES": 8})]


def cases(group):
    if group == "step":
        return [_step(group, 200, 0, dt=dt, D=D, h=h) for dt in ("bf16", "fp16") for D in (64, 128) for h in (6, 4)] + [_step(group, 1039, 0)]
    if group == "team":
        return [_step(group, 2047, 0, dict({"DECODE_SPLIT": 2}, **spin), 2, D=D) for D in (64, 128) for spin in ({}, {"DECODE_TEAM_SPIN": 0})]
    if group == "wide":
        return [_step(group, 32799, 1, {"DECODE_WIDE": 1}), _step(group, 16415, 1, {"DECODE_WIDE": 1, "DECODE_WAVES": 8}),
                _step(group, 16415, 1, {"DECODE_WIDE": 1, "DECODE_WAVES": 8}, h=4)]
    if group == "onepass":
        return [_step(group, 2047, 2, dict({"DECODE_WIDE": 2}, **wv), h=h) for wv in ({}, {"DECODE_WAVES": 8}) for h in (6, 4)]
    if group == "rows":
        mk = lambda t0, S, B, form, **kw: case(group, f"D{kw.get('D', 64)}/t{t0}_S{S}_B{B}", "rows", form, t_pos=[t0] * B, S=S, **kw)  # noqa: E731
        return [mk(1052, 8, 2, 0), mk(1052, 8, 2, 0, D=128), mk(32796, 8, 1, 1)]
    if group == "ragged":
        return RAGGED
    if group == "paged":
        return [types.SimpleNamespace(**dict(vars(c), group=group, kind="paged")) for c in RAGGED]
    if group == "long":
        return LONG + [types.SimpleNamespace(**dict(vars(c), name=c.name + "/paged", kind="paged")) for c in LONG]
    raise KeyError(group)


GROUPS = ("step", "team", "wide", "onepass", "rows", "ragged", "paged", "long", "band")


# ---- inputs (CPU) ------------------------------------------------------------------------------------------------------------------------
def vals(*shape, key):
    return _bf16_round(randn(_rng(61, *key), *shape))


_cache = {}


def inputs(c):
    """Q [B,S,G,h,D], K_cmp [B,G,n_cmp(t_max),D], K / V [B,G,t_max + 1 + 37,D] of a case (fp32 arrays of bf16-representable values; the
    callers pass the K/V views of t_max + 1 rows), shared by the cases of one shape; sequence b's K/V rows beyond its own tokens and its K_cmp
    rows beyond its n_cmp are poisoned (all of them for an empty slot) -> dict with t_max and S_cmp"""
    key = (tuple(c.t_pos), c.S, c.D, c.h)
    if key not in _cache:
        B, t_max = len(c.t_pos), max(c.t_pos) + c.S - 1
        n, cap = ncmp(t_max), t_max + 1 + 37
        tag = (B, c.S, c.D, c.h, t_max)
        Q, Kc = vals(B, c.S, G, c.h, c.D, key=(1, *tag)), vals(B, G, max(n, 1), c.D, key=(2, *tag))
        K, V = vals(B, G, cap, c.D, key=(3, *tag)), vals(B, G, cap, c.D, key=(4, *tag))
        for b, t0 in enumerate(c.t_pos):
            own = t0 + c.S if t0 >= 0 else 0
            K[b, :, own:], V[b, :, own:] = POISON, -POISON
            Kc[b, :, ncmp(own - 1) if own else 0:] = POISON
        _cache[key] = dict(Q=Q, Kc=Kc, K=K, V=V, t_max=t_max, S_cmp=n)
    return _cache[key]


def pools(c):
    """the caches of inputs(c) cut into pages of 1024 tokens that a seeded permutation places in pools of (pages needed + 3) pages; pages
    nobody owns and the table entries nobody needs (they name a spare page) are poisoned -> dict(Kc, K, V, table, max_pages)"""
    g = inputs(c)
    if "pools" not in g:
        own = [t0 + c.S if t0 >= 0 else 0 for t0 in c.t_pos]
        need = [(o + PAGE - 1) // PAGE for o in own]
        max_pages, n_pages = max(need) + 1, sum(need) + 3
        perm = [int(p) for p in _rng(61, 5, len(c.t_pos), c.S, g["t_max"]).permutation(n_pages)]
        Kc = np.full((n_pages, G, PAGE // 16, c.D), POISON, np.float32)
        K, V = np.full((n_pages, G, PAGE, c.D), POISON, np.float32), np.full((n_pages, G, PAGE, c.D), -POISON, np.float32)
        table, k = [[perm[-1]] * max_pages for _ in own], 0
        for b, o in enumerate(own):
            nc = ncmp(o - 1) if o else 0
            for j in range(need[b]):
                p = table[b][j] = perm[k]
                k += 1
                r, rc = min(PAGE, o - PAGE * j), min(PAGE // 16, nc - 64 * j)
                K[p, :, :r], V[p, :, :r] = g["K"][b, :, PAGE * j:PAGE * j + r], g["V"][b, :, PAGE * j:PAGE * j + r]
                if rc > 0:
                    Kc[p, :, :rc] = g["Kc"][b, :, 64 * j:64 * j + rc]
        g["pools"] = dict(Kc=Kc, K=K, V=V, table=np.asarray(table, np.int32), max_pages=max_pages)
    return g["pools"]


def band_module():
    from nsa_vibe_amd.nsa_attention import NSAAttention

    return NSAAttention(*BAND_CFG, l=L, d=DSTRIDE, l_sel=LSEL, n_sel=N_TOP, w=W)


def band_inputs():
    return vals(BAND_B, BAND_PREFILL + BAND_STEPS, BAND_CFG[0], key=(6,))


# ---- runs (device) -----------------------------------------------------------------------------------------------------------------------
class Out(pp.Out):
    def put(self, key, t):
        super().put(key, t, big=BIG)


@contextlib.contextmanager
def switches(sw):
    """the case's tuning switches, and every decode switch back to automatic (-1) afterwards"""
    from nsa_vibe_amd import _lib

    try:
        for k, v in sw.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k in SWITCHES:
            _lib.set_tuning(k, -1)


def _dt(c):
    import torch

    return {"bf16": torch.bfloat16, "fp16": torch.float16}[c.dt]


def run_case(c):
    """-> (O, ranges) of one case, after the library's plan confirmed one launch in the case's form"""
    import torch
    import nsa_vibe_amd as nv

    g, DT = inputs(c), _dt(c)
    B, t_max, n = len(c.t_pos), g["t_max"], g["S_cmp"]
    up = lambda a: torch.from_numpy(a).to(DT).cuda()  # noqa: E731
    meta = nv.build_block_meta(t_max + 1, L, DSTRIDE, LSEL, N_TOP, W)
    assert meta.S_cmp == n
    Q = up(g["Q"])
    shape = (G, c.h, c.D, c.D, n, meta.S_sel)
    if c.kind == "paged":
        pl = pools(c)
        want = {"launches": 1, "form": c.form}
        got = nv.selection_decode_paged_plan(B, c.S, *shape, pl["max_pages"], N_TOP, t_max, DT)
        assert got == want, (c.name, got)
        pos = torch.tensor(c.t_pos, dtype=torch.int32, device="cuda")
        return nv.selection_decode_paged(Q, up(pl["Kc"]), up(pl["K"]), up(pl["V"]), torch.from_numpy(pl["table"]).cuda(), meta, N_TOP, pos, t_max=t_max)
    Kc, K, V = up(g["Kc"])[:, :, :n], up(g["K"])[:, :, :t_max + 1], up(g["V"])[:, :, :t_max + 1]
    if c.kind == "step":
        got = nv.selection_decode_step_plan(B, *shape, t_max + 1, N_TOP, DT)
        assert got == {"launches": 1, "form": c.form, "nsplit": c.nsplit}, (c.name, got)
        return nv.selection_decode_step(Q, Kc, K, V, meta, N_TOP, t_max)
    if c.kind == "rows":
        got = nv.selection_decode_rows_plan(B, c.S, *shape, t_max + 1, N_TOP, DT)
        assert got == {"launches": 1, "form": c.form}, (c.name, got)
        return nv.selection_decode_rows(Q, Kc, K, V, meta, N_TOP, c.t_pos[0])
    got = nv.selection_decode_ragged_plan(B, c.S, *shape, t_max + 1, N_TOP, t_max, DT)
    assert got == {"launches": 1, "form": c.form}, (c.name, got)
    pos = torch.tensor(c.t_pos, dtype=torch.int32, device="cuda")
    return nv.selection_decode_ragged(Q, Kc, K, V, meta, N_TOP, pos, t_max=t_max)


def run_group(out, group):
    import torch

    _cache.clear()  # (inputs are shared inside a group)
    for c in cases(group):
        with switches(c.sw):
            O, rg = run_case(c)
            torch.cuda.synchronize()
        out.put(f"{group}/{c.name}/O", O)
        out.put(f"{group}/{c.name}/ranges", rg)


def run_band(out):
    import torch

    m = pp.load_state(band_module(), 61, torch.bfloat16)
    x = torch.from_numpy(band_inputs()).bfloat16().cuda()
    for band in (1, 2):
        with switches({"DECODE_BAND": band}), torch.no_grad():
            kv = m.new_kv(BAND_B, BAND_PREFILL + BAND_STEPS + 1, "cuda", torch.bfloat16)
            _, kv = m(x[:, :BAND_PREFILL], kv, prefill=True)
            ys = []
            for t in range(BAND_PREFILL, BAND_PREFILL + BAND_STEPS):
                y, kv = m(x[:, t:t + 1], kv, prefill=False)
                ys.append(y)
            torch.cuda.synchronize()
        assert m._fallback_counters["total_fallbacks"] == 0
        out.put(f"band/band{band}/y", torch.cat(ys, dim=1))
        out.put(f"band/band{band}/gates", m._last_gates)
        out.put(f"band/band{band}/ranges", m._last_ranges)


RUN = {g: (lambda o, g=g: run_group(o, g)) for g in GROUPS if g != "band"}
RUN["band"] = run_band


def run_cases():
    out = Out()
    for g in RUN:
        RUN[g](out)
    return out


def list_cases():
    """every input builder, on the CPU: the case table with the form each case is meant for"""
    n = 0
    for grp in GROUPS[:-1]:
        _cache.clear()
        for c in cases(grp):
            g = inputs(c)
            B = len(c.t_pos)
            assert g["Q"].shape == (B, c.S, G, c.h, c.D) and g["Kc"].shape == (B, G, max(g["S_cmp"], 1), c.D) and g["K"].shape == g["V"].shape
            extra = ""
            if c.kind == "paged":
                pl = pools(c)
                assert pl["table"].shape == (B, pl["max_pages"]) and pl["table"].max() < pl["K"].shape[0] and pl["table"].min() >= 0
                extra = f" pools {pl['K'].shape} table {pl['table'].shape}"
            print(f"{grp}/{c.name}: {c.kind} form {c.form} t_pos {c.t_pos} S {c.S} S_cmp {g['S_cmp']} chunks {(g['S_cmp'] + 63) // 64} Q {g['Q'].shape} "
                  f"K {g['K'].shape}{extra} switches {c.sw}")
            n += 1
    m = band_module()
    m.load_state_dict({k: __import__("torch").from_numpy(v) for k, v in pp.module_state(m, 61).items()})
    print(f"band: NSAAttention{BAND_CFG} x {band_inputs().shape}, prefill {BAND_PREFILL}, {BAND_STEPS} steps, DECODE_BAND 1 and 2")
    print(f"{n + 2} cases constructed")


if __name__ == "__main__":
    if sys.argv[1:] == ["--list"]:
        list_cases()
    else:
        res = run_cases()
        np.savez_compressed(sys.argv[1], **res)
        print(f"{len(res)} arrays, {os.path.getsize(sys.argv[1])} bytes -> {sys.argv[1]}")
