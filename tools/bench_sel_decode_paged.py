#!/usr/bin/env python3
"""The ragged decode step over paged caches (nsa_sel_decode_paged) against nsa_sel_decode_ragged on contiguous caches, timed IN
THE SAME RUN, alternating, on the m7c shape (G = 2, h = 6, D = 64, bf16, n = 16), S = 1, every sequence at the last token of its context:

  (a) an identity table (sequence b's page j is pool page b P + j, P = context / 1024): what the table lookups themselves cost;
  (b) a randomly permuted table over the same pools: what losing page-to-page adjacency costs on top.

Contexts 4k / 16k x B in {16, 64, 256}.  Everything goes through the C ABI with prepared arguments (no Python wrapper work inside the timed
window).  COLD, as bench.py's decode figures and tools/bench_sel_decode_ragged.py: the steps rotate over independent cache sets -- each a
set of contiguous caches and a set of pools of the same size --, so many that the others load >= 512 MiB between two uses of one set (at
most 32 sets).  Device events around batches of NB steps; every cell is measured REPS times and the spread (max - min of the repeated
medians) is printed beside the median of medians: a difference below the spread is no difference.  A record, not a gate: no default
depends on it.

    python tools/bench_sel_decode_paged.py [OUT.json [CONTEXTS [BATCHES]]]     (comma-separated; default 4096,16384 and 16,64,256)
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
PAGE = 1024
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


def n_sets_for(B, ctx):
    step = B * G * (min(N * LS, ctx) * 2 * D * 2 + ncmp(ctx - 1) * D * 2)
    return min(32, -(-COLD_BYTES // step) + 1)


def make_sets(B, ctx, n_sets, seed):
    """n_sets independent (Q, contiguous K_cmp / K / V, pools Kc / K / V of B ctx / 1024 pages)"""
    sets, n_pages = [], B * ctx // PAGE
    for i in range(n_sets):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed + 1009 * i)
        mk = lambda *sh: torch.randn(*sh, device=dev, generator=g, dtype=dt)  # noqa: E731
        sets.append((mk(B, 1, G, H, D), mk(B, G, ncmp(ctx - 1), D), mk(B, G, ctx, D), mk(B, G, ctx, D), mk(n_pages, G, PAGE // 16, D), mk(n_pages, G, PAGE, D),
                     mk(n_pages, G, PAGE, D)))
    return sets


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


def routes_for(B, ctx, sets, st, keep):
    t = ctx - 1
    P = ctx // PAGE
    meta = nv.build_block_meta(ctx, L_, D_, LS, N, W)
    csc = meta.device_csc(dev)
    pos_dev = torch.full((B,), t, dtype=torch.int32, device=dev)
    O = torch.empty(B, 1, G, H, D, device=dev, dtype=dt)
    rg = torch.empty(B, 1, G, N, 2, device=dev, dtype=torch.int32)
    gen = torch.Generator()
    gen.manual_seed(1000 * B + P)
    ident = torch.arange(B * P, dtype=torch.int32).view(B, P)
    tables = {"paged_identity": ident.to(dev), "paged_permuted": torch.randperm(B * P, generator=gen).to(torch.int32).view(B, P).to(dev)}
    keep += [meta, csc, pos_dev, O, rg, tables]
    common = [csc[0].data_ptr(), csc[1].data_ptr(), csc[2].data_ptr(), rg.data_ptr(), O.data_ptr(), pos_dev.data_ptr(), t, B, 1, G, H, D, D, meta.S_cmp, meta.S_sel]
    ragged_args, paged_args = [], {k: [] for k in tables}
    for Q, Kc, K, V, Kcp, Kp, Vp in sets:
        ragged_args.append([Q.data_ptr(), Kc.data_ptr(), K.data_ptr(), V.data_ptr(), *common, ctx, L_, D_, LS, N, *strides(Kc, K, V), DT, 0.0, None, 0, st])
        for k, tb in tables.items():
            paged_args[k].append([Q.data_ptr(), Kcp.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), tb.data_ptr(), tb.stride(0), B * P, P, PAGE, *common, L_, D_, LS, N,
                                  *strides(Kcp, Kp, Vp), DT, 0.0, None, 0, st])

    def ragged(i):
        _lib.check(L.nsa_sel_decode_ragged(*ragged_args[i]), "ragged")

    def paged(k):
        return lambda i: _lib.check(L.nsa_sel_decode_paged(*paged_args[k][i]), k)

    return {"ragged": ragged, "paged_identity": paged("paged_identity"), "paged_permuted": paged("paged_permuted")}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    st = _stream(dev)
    res = {"library": _lib.loaded_library(), "shape": {"G": G, "h": H, "D": D, "n_top": N, "dtype": "bf16", "S": 1, "page_tokens": PAGE}, "steps_per_batch": NB,
           "batches": NBATCH, "reps": REPS, "cells": []}
    contexts = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4096, 16384]
    batches = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [16, 64, 256]
    assert all(c % PAGE == 0 for c in contexts), "contexts must be multiples of the page size"
    for ctx in contexts:
        for B in batches:
            n_sets = n_sets_for(B, ctx)
            sets, keep = make_sets(B, ctx, n_sets, 7), []
            routes = routes_for(B, ctx, sets, st, keep)
            plan = nv.selection_decode_paged_plan(B, 1, G, H, D, D, ncmp(ctx - 1), -(-ctx // LS), ctx // PAGE, N, ctx - 1, dt)
            r = measure(routes, n_sets)
            cell = {"ctx": ctx, "B": B, "cache_sets": n_sets, "form": plan["form"]}
            for k, (us, spread) in r.items():
                cell[k + "_us"], cell[k + "_spread_us"] = us, spread
            print(json.dumps(cell), flush=True)
            res["cells"].append(cell)
            del sets, keep, routes
            torch.cuda.empty_cache()
    print("\n| context | B | sets | ragged, contiguous us | paged, identity table us | paged, permuted table us | spread us |\n|---|---|---|---|---|---|---|")
    for c in res["cells"]:
        print(f"| {c['ctx']} | {c['B']} | {c['cache_sets']} | {c['ragged_us']:.1f} | {c['paged_identity_us']:.1f} | {c['paged_permuted_us']:.1f} | "
              f"{max(c['ragged_spread_us'], c['paged_identity_spread_us'], c['paged_permuted_spread_us']):.1f} |")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
