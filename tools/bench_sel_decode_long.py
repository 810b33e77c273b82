#!/usr/bin/env python3
"""The long-row form of the ragged decode step (DECODE_LONG = 1, plan form 3) against what the library offers at the same shape
with EQUAL positions today -- one nsa_sel_decode_step on the same data, whose plan (team of workgroups, one-pass form or two launches) is
printed beside its time -- timed in the same run, alternating, m7c head geometry (G = 2, h = 6, n = 16, bf16):

    D = 64:  96k and 128k x B in {16, 64}; 48k x B = 160 (320 rows: 8 waves per row)
    D = 128: 32k and 64k x B in {16, 64}
    mixed:   D = 64, B = 16, positions drawn from [1k, 128k): one long call against one nsa_sel_decode_step per sequence

The protocol is tools/bench_sel_decode_ragged.py's: C ABI with prepared arguments, COLD (the steps rotate over independent cache sets so
that >= 512 MiB pass between two uses of one set), device events around batches of steps, the median of repeated medians and the spread.
Per cell the algorithmic bytes of the long form -- K_cmp once, the chunks beyond a wave's first two once more, the gathered blocks -- and
the fraction of the 8 TB/s peak they make at the measured time.

    python tools/bench_sel_decode_long.py [OUT.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_sel_decode_long.py --cell D CONTEXT B
        (one cell alone, both routes 100 steps each cold, no event timing: the kernel times come from the trace)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_sel_decode_ragged as R  # noqa: E402  (measure, wsp, strides, ncmp and the constants of the protocol)
import nsa_vibe_amd as nv  # noqa: E402
from nsa_vibe_amd import _lib  # noqa: E402

G, H, N, L_, D_, LS, W = R.G, R.H, R.N, R.L_, R.D_, R.LS, R.W
dt, dev, L, DT = R.dt, R.dev, R.L, R.DT
PEAK = 8.0e12  # bytes / s
ncmp = R.ncmp


def make_sets(B, cap, D, n_sets, seed):
    sets = []
    for i in range(n_sets):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + 1009 * i)
        mk = lambda *sh: torch.randn(*sh, device=dev, generator=g, dtype=dt)  # noqa: E731
        sets.append((mk(B, 1, G, H, D), mk(B, G, ncmp(cap - 1), D), mk(B, G, cap, D), mk(B, G, cap, D)))
    return sets


def long_bytes(positions, D, nw):
    """algorithmic bytes of one long call: per row K_cmp once, the chunks beyond 2 nw again, the gathered blocks' K and V"""
    total = 0
    for t in positions:
        n = ncmp(t)
        again = max(0, n - 2 * nw * 64)
        total += G * ((n + again) * D * 2 + min(N * LS, t + 1) * 2 * D * 2)
    return total


def routes_for(B, positions, D, sets, st, keep):
    t_max = max(positions)
    meta = nv.build_block_meta(t_max + 1, L_, D_, LS, N, W)
    csc = meta.device_csc(dev)
    pos_dev = torch.tensor(positions, dtype=torch.int32, device=dev)
    O = torch.empty(B, 1, G, H, D, device=dev, dtype=dt)
    rg = torch.empty(B, 1, G, N, 2, device=dev, dtype=torch.int32)
    groups = {}
    for b, t in enumerate(positions):
        groups.setdefault(t, []).append(b)
    assert all(bs == list(range(bs[0], bs[0] + len(bs))) for bs in groups.values())
    long_args, step_args = [], []
    for Q, Kc, K, V in sets:
        long_args.append([Q.data_ptr(), Kc.data_ptr(), K.data_ptr(), V.data_ptr(), csc[0].data_ptr(), csc[1].data_ptr(), csc[2].data_ptr(), rg.data_ptr(),
                          O.data_ptr(), pos_dev.data_ptr(), t_max, B, 1, G, H, D, D, meta.S_cmp, meta.S_sel, K.shape[2], L_, D_, LS, N, *R.strides(Kc, K, V), DT,
                          0.0, None, 0, st])
        per = []
        for t, bs in groups.items():
            b0, nb = bs[0], len(bs)
            m = nv.build_block_meta(t + 1, L_, D_, LS, N, W)
            c = m.device_csc(dev)
            w, wp, wn = R.wsp(L.nsa_sel_decode_step_workspace(nb, G, H, D, D, ncmp(t), m.S_sel, N, DT))
            keep += [m, c, w]
            per.append([Q[b0:].data_ptr(), Kc[b0:].data_ptr(), K[b0:].data_ptr(), V[b0:].data_ptr(), c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(),
                        rg[b0:].data_ptr(), O[b0:].data_ptr(), nb, G, H, D, D, ncmp(t), m.S_sel, t + 1, L_, D_, LS, N, t, *R.strides(Kc, K, V), DT, 0.0, wp, wn, st])
        step_args.append(per)
    keep += [meta, csc, pos_dev, O, rg]

    def long(i):
        _lib.check(L.nsa_sel_decode_ragged(*long_args[i]), "long")

    def steps(i):
        for a in step_args[i]:
            _lib.check(L.nsa_sel_decode_step(*a), "step")

    plan = nv.selection_decode_ragged_plan(B, 1, G, H, D, D, meta.S_cmp, meta.S_sel, sets[0][2].shape[2], N, t_max, dt)
    assert plan == {"launches": 1, "form": 3}, plan
    return {"long": long, "steps": steps}, len(groups)


def cell_of(B, positions, D, st, seed):
    t_max = max(positions)
    mean = sum(positions) // B
    step = B * G * (min(N * LS, mean) * 2 * D * 2 + ncmp(mean) * D * 2)
    n_sets = min(32, -(-R.COLD_BYTES // step) + 1)
    sets, keep = make_sets(B, t_max + 1, D, n_sets, seed), []
    routes, ngroups = routes_for(B, positions, D, sets, st, keep)
    r = R.measure(routes, n_sets)
    nw = 8 if D == 128 or B * G > 256 else 16
    nbytes = long_bytes(positions, D, nw)
    cell = {"D": D, "B": B, "t_min": min(positions), "t_max": t_max, "groups": ngroups, "cache_sets": n_sets, "waves": nw, "long_us": r["long"][0],
            "long_spread_us": r["long"][1], "steps_us": r["steps"][0], "steps_spread_us": r["steps"][1], "long_bytes": nbytes,
            "long_peak_fraction": nbytes / (r["long"][0] * 1e-6) / PEAK}
    if ngroups == 1:
        cell["step_plan"] = nv.selection_decode_step_plan(B, G, H, D, D, ncmp(t_max), -(-(t_max + 1) // LS), t_max + 1, N, dt)
    del sets, keep, routes
    torch.cuda.empty_cache()
    return cell


def trace_cell(D, ctx, B):
    st = R._stream(dev)
    positions = [ctx - 1] * B
    step = B * G * (min(N * LS, ctx) * 2 * D * 2 + ncmp(ctx - 1) * D * 2)
    n_sets = min(32, -(-R.COLD_BYTES // step) + 1)
    sets, keep = make_sets(B, ctx, D, n_sets, 7), []
    routes, _ = routes_for(B, positions, D, sets, st, keep)
    for f in routes.values():
        for i in range(100):
            f(i % n_sets)
        torch.cuda.synchronize()


def main():
    _lib.set_tuning("DECODE_LONG", 1)
    if len(sys.argv) > 1 and sys.argv[1] == "--cell":
        return trace_cell(*(int(v) for v in sys.argv[2:5]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    st = R._stream(dev)
    res = {"library": _lib.loaded_library(), "shape": {"G": G, "h": H, "n_top": N, "dtype": "bf16"}, "steps_per_batch": R.NB, "batches": R.NBATCH, "reps": R.REPS,
           "equal": [], "mixed": []}
    K = 1024
    for D, ctx, B in ((64, 96 * K, 16), (64, 96 * K, 64), (64, 128 * K, 16), (64, 128 * K, 64), (64, 48 * K, 160), (128, 32 * K, 16), (128, 32 * K, 64),
                      (128, 64 * K, 16), (128, 64 * K, 64)):
        cell = cell_of(B, [ctx - 1] * B, D, st, 7)
        print(json.dumps(cell), flush=True)
        res["equal"].append(cell)
    gen = torch.Generator()
    gen.manual_seed(116)
    positions = sorted(int(v) for v in torch.randint(1024, 128 * K, (16,), generator=gen))
    positions[-1] = max(positions[-1], 70000)  # (at least one row beyond the unsplit forms)
    cell = cell_of(16, positions, 64, st, 11)
    print(json.dumps(cell), flush=True)
    res["mixed"].append(cell)
    print("\n(a) equal positions: one long call against one single step\n| D | context | B | waves | sets | single step launches / form / workgroups per row | long us | "
          "single step us | spread us | long MB | of 8 TB/s |\n|---|---|---|---|---|---|---|---|---|---|---|")
    for c in res["equal"]:
        p = c["step_plan"]
        print(f"| {c['D']} | {c['t_max'] + 1} | {c['B']} | {c['waves']} | {c['cache_sets']} | {p['launches']} / {p['form']} / {p['nsplit']} | {c['long_us']:.1f} | "
              f"{c['steps_us']:.1f} | {max(c['long_spread_us'], c['steps_spread_us']):.1f} | {c['long_bytes'] / 1e6:.1f} | {c['long_peak_fraction']:.3f} |")
    print("\n(b) positions drawn from [1k, 128k): one long call against one single step per sequence\n| D | B | positions | sets | long us | steps us | spread us | "
          "long MB | of 8 TB/s |\n|---|---|---|---|---|---|---|---|---|")
    for c in res["mixed"]:
        print(f"| {c['D']} | {c['B']} | {c['t_min']} .. {c['t_max']} | {c['cache_sets']} | {c['long_us']:.1f} | {c['steps_us']:.1f} | "
              f"{max(c['long_spread_us'], c['steps_spread_us']):.1f} | {c['long_bytes'] / 1e6:.1f} | {c['long_peak_fraction']:.3f} |")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
