#!/usr/bin/env python3
"""The ragged-batch decode calls (nsa_sel_decode_ragged, nsa_band_attn_fwd_ragged) against what a caller runs without them,
timed IN THE SAME RUN, alternating, on the m7c shape (G = 2, h = 6, D = 64, bf16, n = 16, w = 512):

  (a) equal positions: one ragged call against nsa_sel_decode_step (unchanged code), B in {16, 64, 256} x contexts {4k, 16k}; beside them
      the rows form without a position array (nsa_sel_decode_rows, S = 1, DECODE_ROWS = 1): what separates it from the ragged call is the
      position load alone;
  (b) a mixed batch, positions drawn uniformly from [1k, 16k], B in {16, 64}: one ragged call against one nsa_sel_decode_step per group of
      equal length (with drawn positions: one per sequence, on that sequence's views);
  (c) the sliding + compressed branch of the same mixed batches: two nsa_band_attn_fwd_ragged calls against two nsa_band_attn_fwd calls per
      sequence.

Everything goes through the C ABI with prepared arguments (no Python wrapper work inside the timed window).  COLD, as bench.py's decode
figures: the steps rotate over independent cache sets, so many that the others load >= 512 MiB between two uses of one set (at most 32
sets).  Device events around batches of NB steps; every cell is measured REPS times and the spread (max - min of the repeated medians) is
printed beside the median of medians: a difference below the spread is no difference.

    python tools/bench_sel_decode_ragged.py [OUT.json]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nsa_vibe_amd as nv  # noqa: E402
from nsa_vibe_amd import _lib  # noqa: E402
from nsa_vibe_amd.selection_scorer import _DT, _stream  # noqa: E402

G, H, D, N = 2, 6, 64, 16
L_, D_, LS, W = 32, 16, 64, 512
NB, NBATCH, REPS = 10, 5, 3
COLD_BYTES = 512 * 2 ** 20
dt = torch.bfloat16
dev = torch.device("cuda")
L = _lib.lib()
DT = _DT[dt]


def ncmp(t):
    return 0 if t + 1 < L_ else (t + 1 - L_) // D_ + 1


def strides(*ts):
    return [x.stride(i) for x in ts for i in range(3)]


def wsp(nbytes):
    w = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return w, (w.data_ptr() + 255) & ~255, nbytes


def make_sets(B, cap, n_sets, seed):
    """n_sets independent (Q, K_cmp, V_cmp, K, V) of B sequences with room for cap tokens"""
    sets = []
    for i in range(n_sets):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + 1009 * i)
        mk = lambda *sh: torch.randn(*sh, device=dev, generator=g, dtype=dt)  # noqa: E731
        sets.append((mk(B, 1, G, H, D), mk(B, G, ncmp(cap - 1), D), mk(B, G, ncmp(cap - 1), D), mk(B, G, cap, D), mk(B, G, cap, D)))
    return sets


def n_sets_for(B, ctx_mean):
    step = B * G * (min(N * LS, ctx_mean) * 2 * D * 2 + ncmp(ctx_mean - 1) * D * 2)
    return min(32, -(-COLD_BYTES // step) + 1)


def measure(routes, n_sets):
    """routes: {name: f(set index)} -> {name: (median of medians us per step, spread us)}"""
    pos = {k: 0 for k in routes}
    for k, f in routes.items():
        for i in range(n_sets):
            f(i)
    torch.cuda.synchronize()
    med = {k: [] for k in routes}
    for _ in range(REPS):
        ts = {k: [] for k in routes}
        for _ in range(NBATCH):
            for k, f in routes.items():  # alternating: drift of the machine hits every route alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(NB):
                    f(pos[k] % n_sets)
                    pos[k] += 1
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / NB)
        for k in routes:
            med[k].append(statistics.median(ts[k]))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in med.items()}


def sel_routes(B, positions, sets, st, keep):
    """the ragged call on every set, and per set one nsa_sel_decode_step per group of equal position (on the group's batch slice)"""
    t_max = max(positions)
    meta = nv.build_block_meta(t_max + 1, L_, D_, LS, N, W)
    csc = meta.device_csc(dev)
    pos_dev = torch.tensor(positions, dtype=torch.int32, device=dev)
    O = torch.empty(B, 1, G, H, D, device=dev, dtype=dt)
    rg = torch.empty(B, 1, G, N, 2, device=dev, dtype=torch.int32)
    groups = {}
    for b, t in enumerate(positions):
        groups.setdefault(t, []).append(b)
    assert all(bs == list(range(bs[0], bs[0] + len(bs))) for bs in groups.values())  # (groups are batch slices here)
    ragged_args, step_args = [], []
    for Q, Kc, Vc, K, V in sets:
        ragged_args.append([Q.data_ptr(), Kc.data_ptr(), K.data_ptr(), V.data_ptr(), csc[0].data_ptr(), csc[1].data_ptr(), csc[2].data_ptr(), rg.data_ptr(),
                            O.data_ptr(), pos_dev.data_ptr(), t_max, B, 1, G, H, D, D, meta.S_cmp, meta.S_sel, K.shape[2], L_, D_, LS, N, *strides(Kc, K, V), DT,
                            0.0, None, 0, st])
        per = []
        for t, bs in groups.items():
            b0, nb = bs[0], len(bs)
            m = nv.build_block_meta(t + 1, L_, D_, LS, N, W)
            c = m.device_csc(dev)
            w, wp, wn = wsp(L.nsa_sel_decode_step_workspace(nb, G, H, D, D, ncmp(t), m.S_sel, N, DT))
            keep += [m, c, w]
            per.append([Q[b0:].data_ptr(), Kc[b0:].data_ptr(), K[b0:].data_ptr(), V[b0:].data_ptr(), c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(),
                        rg[b0:].data_ptr(), O[b0:].data_ptr(), nb, G, H, D, D, ncmp(t), m.S_sel, t + 1, L_, D_, LS, N, t, *strides(Kc, K, V), DT, 0.0, wp, wn, st])
        step_args.append(per)
    keep += [meta, csc, pos_dev, O, rg]
    routes = {}
    if len(groups) == 1:  # equal positions: the rows form at t0 = the position, same buffers
        w, wp, wn = wsp(L.nsa_sel_decode_rows_workspace(B, 1, G, H, D, D, meta.S_cmp, meta.S_sel, N, DT))
        keep.append(w)
        rows_args = [a[:9] + a[11:24] + [t_max] + a[24:34] + [0.0, wp, wn, st] for a in ragged_args]

        def rows(i):
            _lib.check(L.nsa_sel_decode_rows(*rows_args[i]), "rows")

        routes["rows"] = rows

    def ragged(i):
        _lib.check(L.nsa_sel_decode_ragged(*ragged_args[i]), "ragged")

    def steps(i):
        for a in step_args[i]:
            _lib.check(L.nsa_sel_decode_step(*a), "step")

    routes.update({"ragged": ragged, "steps": steps})
    return routes, len(groups)


def band_routes(B, positions, sets, st, keep):
    """sliding (w = 512) + compressed branch: two ragged calls per step against two scalar calls per sequence"""
    t_max = max(positions)
    pos_dev = torch.tensor(positions, dtype=torch.int32, device=dev)
    Ow, Oc = torch.empty(B, 1, G, H, D, device=dev, dtype=dt), torch.empty(B, 1, G, H, D, device=dev, dtype=dt)
    w, wp, wn = wsp(L.nsa_band_attn_fwd_ragged_workspace(B, 1, G, H, D, D, DT))
    w1, wp1, wn1 = wsp(L.nsa_band_attn_fwd_workspace(1, 1, G, H, D, D, DT))
    keep += [pos_dev, Ow, Oc, w, w1]
    rag, per = [], []
    for Q, Kc, Vc, K, V in sets:
        rag.append([[Q.data_ptr(), K.data_ptr(), V.data_ptr(), Ow.data_ptr(), None, pos_dev.data_ptr(), t_max, B, 1, G, H, D, D, K.shape[2], *strides(K, V), 0, 1, 0, W,
                     DT, 0.0, 0, wp, wn, st],
                    [Q.data_ptr(), Kc.data_ptr(), Vc.data_ptr(), Oc.data_ptr(), None, pos_dev.data_ptr(), t_max, B, 1, G, H, D, D, Kc.shape[2], *strides(Kc, Vc), L_, D_,
                     1, 1 << 30, DT, 0.0, 0, wp, wn, st]])
        calls = []
        for b, t in enumerate(positions):
            calls.append([Q[b:].data_ptr(), K[b:].data_ptr(), V[b:].data_ptr(), Ow[b:].data_ptr(), None, 1, 1, G, H, D, D, t + 1, *strides(K, V), t, 0, 1, 0, W, DT, 0.0,
                          0, wp1, wn1, st])
            calls.append([Q[b:].data_ptr(), Kc[b:].data_ptr(), Vc[b:].data_ptr(), Oc[b:].data_ptr(), None, 1, 1, G, H, D, D, ncmp(t), *strides(Kc, Vc), t, L_, D_, 1,
                          1 << 30, DT, 0.0, 0, wp1, wn1, st])
        per.append(calls)

    def ragged(i):
        for a in rag[i]:
            _lib.check(L.nsa_band_attn_fwd_ragged(*a), "band ragged")

    def scalar(i):
        for a in per[i]:
            _lib.check(L.nsa_band_attn_fwd(*a), "band")

    return {"ragged": ragged, "per_sequence": scalar}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    st = _stream(dev)
    res = {"library": _lib.loaded_library(), "shape": {"G": G, "h": H, "D": D, "n_top": N, "w": W, "dtype": "bf16"}, "steps_per_batch": NB, "batches": NBATCH,
           "reps": REPS, "equal": [], "mixed": [], "band": []}
    for ctx in (4096, 16384):
        for B in (16, 64, 256):
            n_sets = n_sets_for(B, ctx)
            sets, keep = make_sets(B, ctx, n_sets, 7), []
            routes, _ = sel_routes(B, [ctx - 1] * B, sets, st, keep)
            plan = nv.selection_decode_step_plan(B, G, H, D, D, ncmp(ctx - 1), -(-ctx // LS), ctx, N, dt)
            _lib.set_tuning("DECODE_ROWS", 1)
            r = measure(routes, n_sets)
            _lib.set_tuning("DECODE_ROWS", -1)
            cell = {"ctx": ctx, "B": B, "cache_sets": n_sets, "step_form": plan["form"], "step_nsplit": plan["nsplit"], "ragged_us": r["ragged"][0],
                    "ragged_spread_us": r["ragged"][1], "step_us": r["steps"][0], "step_spread_us": r["steps"][1], "rows_us": r["rows"][0],
                    "rows_spread_us": r["rows"][1]}
            print(json.dumps(cell), flush=True)
            res["equal"].append(cell)
            del sets, keep, routes
            torch.cuda.empty_cache()
    for B in (16, 64):
        gen = torch.Generator()
        gen.manual_seed(100 + B)
        positions = sorted(int(v) for v in torch.randint(1024, 16385, (B,), generator=gen))
        mean = sum(positions) // B
        n_sets = n_sets_for(B, mean)
        sets, keep = make_sets(B, max(positions) + 1, n_sets, 11), []
        routes, ngroups = sel_routes(B, positions, sets, st, keep)
        r = measure(routes, n_sets)
        cell = {"B": B, "positions_min": positions[0], "positions_max": positions[-1], "groups": ngroups, "cache_sets": n_sets, "ragged_us": r["ragged"][0],
                "ragged_spread_us": r["ragged"][1], "steps_us": r["steps"][0], "steps_spread_us": r["steps"][1]}
        print(json.dumps(cell), flush=True)
        res["mixed"].append(cell)
        r = measure(band_routes(B, positions, sets, st, keep), n_sets)
        cell = {"B": B, "cache_sets": n_sets, "ragged_us": r["ragged"][0], "ragged_spread_us": r["ragged"][1], "per_sequence_us": r["per_sequence"][0],
                "per_sequence_spread_us": r["per_sequence"][1]}
        print(json.dumps(cell), flush=True)
        res["band"].append(cell)
        del sets, keep, routes
        torch.cuda.empty_cache()
    print("\n(a) equal positions\n| context | B | sets | single step form / workgroups per row | ragged us | single step us | rows form us | spread us |\n|---|---|---|---|---|---|---|---|")
    for c in res["equal"]:
        print(f"| {c['ctx']} | {c['B']} | {c['cache_sets']} | {c['step_form']} / {c['step_nsplit']} | {c['ragged_us']:.1f} | {c['step_us']:.1f} | "
              f"{c['rows_us']:.1f} | {max(c['ragged_spread_us'], c['step_spread_us'], c['rows_spread_us']):.1f} |")
    print("\n(b) mixed batch, selected branch\n| B | groups | sets | one ragged call us | one single step per group us | spread us |\n|---|---|---|---|---|---|")
    for c in res["mixed"]:
        print(f"| {c['B']} | {c['groups']} | {c['cache_sets']} | {c['ragged_us']:.1f} | {c['steps_us']:.1f} | {max(c['ragged_spread_us'], c['steps_spread_us']):.1f} |")
    print("\n(c) mixed batch, sliding + compressed branch\n| B | sets | two ragged calls us | two calls per sequence us | spread us |\n|---|---|---|---|---|")
    for c in res["band"]:
        print(f"| {c['B']} | {c['cache_sets']} | {c['ragged_us']:.1f} | {c['per_sequence_us']:.1f} | {max(c['ragged_spread_us'], c['per_sequence_spread_us']):.1f} |")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
