#!/usr/bin/env python3
"""The decode step of the selected branch for S consecutive tokens (nsa_sel_decode_rows): three routes timed IN THE SAME RUN,
alternating, on the m7c shape (G = 2, h = 6, D = 64, bf16, n = 16), S in {1, 2, 4, 8} x contexts {4k, 16k, 32k} x B in {1, 16}:

  (a) one nsa_sel_decode_rows call in its one-launch form (DECODE_ROWS = 1),
  (b) S calls of nsa_sel_decode_step on the truncated views of the same cache,
  (c) the separate launches nsa_sel_decode_rows falls back to (DECODE_ROWS = 0).

All three go through the C ABI with prepared arguments (no Python wrapper work inside the timed window).  Device-event medians after
warm-up; every cell is measured REPS times and the spread (max - min of the repeated medians, per route) is printed beside the median of
medians: a difference below the spread is no difference.  The caches are the same for all routes and stay warm at these sizes.
(tools/bench_decode_rows.py is an older tool of another purpose: the decode rows of `bench.py --full`.)

    python tools/bench_sel_decode_rows.py [OUT.json]
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
WARM, ITERS, REPS = 10, 30, 3
dt = torch.bfloat16
dev = torch.device("cuda")
L = _lib.lib()


def ncmp(t):
    return 0 if t + 1 < L_ else (t + 1 - L_) // D_ + 1


def strides(*ts):
    return [x.stride(i) for x in ts for i in range(3)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    res = {"library": _lib.loaded_library(), "shape": {"G": G, "h": H, "D": D, "n_top": N, "dtype": "bf16"}, "iters": ITERS, "reps": REPS, "cells": []}
    st = _stream(dev)
    for ctx in (4096, 16384, 32768):
        for B in (1, 16):
            for S in (1, 2, 4, 8):
                t0 = ctx - S
                meta = nv.build_block_meta(ctx, L_, D_, LS, N, W)
                mk = lambda *sh: torch.randn(*sh, device=dev, generator=g, dtype=dt)  # noqa: E731
                Q, Kc, K, V = mk(B, S, G, H, D), mk(B, G, meta.S_cmp, D), mk(B, G, ctx, D), mk(B, G, ctx, D)
                O = torch.empty(B, S, G, H, D, device=dev, dtype=dt)
                rg = torch.empty(B, S, G, N, 2, device=dev, dtype=torch.int32)
                ws = torch.empty(L.nsa_sel_decode_rows_workspace(B, S, G, H, D, D, meta.S_cmp, meta.S_sel, N, _DT[dt]) + 16, dtype=torch.uint8, device=dev)
                csc = meta.device_csc(dev)
                rows_args = [Q.data_ptr(), Kc.data_ptr(), K.data_ptr(), V.data_ptr(), csc[0].data_ptr(), csc[1].data_ptr(), csc[2].data_ptr(),
                             rg.data_ptr(), O.data_ptr(), B, S, G, H, D, D, meta.S_cmp, meta.S_sel, ctx, L_, D_, LS, N, t0, *strides(Kc, K, V), _DT[dt],
                             0.0, (ws.data_ptr() + 15) & ~15, ws.numel() - 16, st]
                singles, keep = [], []
                for s in range(S):
                    t = t0 + s
                    m = nv.build_block_meta(t + 1, L_, D_, LS, N, W)
                    c = m.device_csc(dev)
                    Qs, Os, rs = Q[:, s:s + 1].contiguous(), torch.empty(B, 1, G, H, D, device=dev, dtype=dt), torch.empty(B, G, N, 2, device=dev, dtype=torch.int32)
                    w1 = torch.empty(L.nsa_sel_decode_step_workspace(B, G, H, D, D, ncmp(t), m.S_sel, N, _DT[dt]) + 16, dtype=torch.uint8, device=dev)
                    keep += [m, c, Qs, Os, rs, w1]
                    singles.append([Qs.data_ptr(), Kc.data_ptr(), K.data_ptr(), V.data_ptr(), c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(), rs.data_ptr(),
                                    Os.data_ptr(), B, G, H, D, D, ncmp(t), m.S_sel, t + 1, L_, D_, LS, N, t, *strides(Kc, K, V), _DT[dt], 0.0,
                                    (w1.data_ptr() + 15) & ~15, w1.numel() - 16, st])

                def route_a():
                    _lib.set_tuning("DECODE_ROWS", 1)
                    _lib.check(L.nsa_sel_decode_rows(*rows_args), "rows")

                def route_b():
                    for a in singles:
                        _lib.check(L.nsa_sel_decode_step(*a), "step")

                def route_c():
                    _lib.set_tuning("DECODE_ROWS", 0)
                    _lib.check(L.nsa_sel_decode_rows(*rows_args), "rows (separate launches)")

                _lib.set_tuning("DECODE_ROWS", 1)
                plan = nv.selection_decode_rows_plan(B, S, G, H, D, D, meta.S_cmp, meta.S_sel, ctx, N, dt)
                assert plan["launches"] == 1, plan
                routes = {"a": route_a, "b": route_b, "c": route_c}
                for _ in range(WARM):
                    for f in routes.values():
                        f()
                torch.cuda.synchronize()
                med = {k: [] for k in routes}
                for _ in range(REPS):
                    ts = {k: [] for k in routes}
                    for _ in range(ITERS):
                        for k, f in routes.items():  # alternating: drift of the machine hits all three alike
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            f()
                            e1.record()
                            e1.synchronize()
                            ts[k].append(e0.elapsed_time(e1) * 1e3)
                    for k in routes:
                        med[k].append(statistics.median(ts[k]))
                _lib.set_tuning("DECODE_ROWS", -1)
                cell = {"ctx": ctx, "B": B, "S": S, "form": plan["form"]}
                for k in routes:
                    cell[f"{k}_us"] = statistics.median(med[k])
                    cell[f"{k}_spread_us"] = max(med[k]) - min(med[k])
                spread = max(cell["a_spread_us"], cell["b_spread_us"], cell["c_spread_us"])
                cell["a_not_slower"] = bool(cell["a_us"] <= min(cell["b_us"], cell["c_us"]) + spread)
                print(json.dumps(cell), flush=True)
                res["cells"].append(cell)
                del keep, singles
    print("\n| context | B | S | (a) one launch us | (b) S single steps us | (c) separate launches us | spread us | (a) not slower |")
    print("|---|---|---|---|---|---|---|---|")
    for c in res["cells"]:
        sp = max(c["a_spread_us"], c["b_spread_us"], c["c_spread_us"])
        print(f"| {c['ctx']} | {c['B']} | {c['S']} | {c['a_us']:.1f} | {c['b_us']:.1f} | {c['c_us']:.1f} | {sp:.1f} | {'yes' if c['a_not_slower'] else 'no'} |")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
