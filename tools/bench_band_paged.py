#!/usr/bin/env python3
"""The sliding and the compressed branch of a ragged decode step over paged caches (nsa_band_attn_fwd_paged) against
nsa_band_attn_fwd_ragged on contiguous caches, timed IN THE SAME RUN, alternating, on the m7c shape (G = 2, h = 6, D = 64, bf16), S = 1,
every sequence at the last token of its context.  Sliding: w = 512 on pages of 1024 rows; compressed (l = 32, d = 16): pages of 64 rows.

  (a) an identity table (sequence b's page j is pool page b P + j): what the table entries and the per-page descriptors themselves cost;
  (b) a randomly permuted table over the same pools: what losing page-to-page adjacency costs on top.

Contexts 4k / 16k x B in {16, 64, 256}.  Everything goes through the C ABI with prepared arguments (no Python wrapper work inside the timed
window).  COLD, the protocol of tools/bench_sel_decode_paged.py: the steps rotate over independent cache sets -- each a pair of contiguous
caches and a pair of pools of the same size --, so many that the others load >= 512 MiB between two uses of one set (at most 32 sets).
Device events around batches of NB steps; every cell is measured REPS times and the spread (max - min of the repeated medians) is printed
beside the median of medians: a difference below the spread is no difference.  A record, not a gate: no default depends on it.

    python tools/bench_band_paged.py [OUT.json [CONTEXTS [BATCHES]]]     (comma-separated; default 4096,16384 and 16,64,256)
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsa_vibe_amd import _lib  # noqa: E402
from nsa_vibe_amd.selection_scorer import _DT, _stream  # noqa: E402

G, H, D = 2, 6, 64
L_, D_, W = 32, 16, 512
NB, NBATCH, REPS = 10, 5, 3
COLD_BYTES = 512 * 2 ** 20
dt = torch.bfloat16
dev = torch.device("cuda")
L = _lib.lib()
DT = _DT[dt]
# branch -> (a, dd, c, w), page rows, key rows a sequence of ctx tokens holds, key rows one step reads
BRANCHES = {
    "sliding": ((0, 1, 0, W), 1024, lambda ctx: ctx, lambda ctx: min(W, ctx)),
    "compressed": ((L_, D_, 1, 1 << 30), 64, lambda ctx: (ctx - L_) // D_ + 1, lambda ctx: (ctx - L_) // D_ + 1),
}


def strides(*ts):
    return [x.stride(i) for x in ts for i in range(3)]


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


def cell_routes(branch, B, ctx, st, keep):
    band, rows, held, read = BRANCHES[branch]
    P = -(-held(ctx) // rows)  # pages per sequence
    cap = P * rows
    n_sets = min(32, -(-COLD_BYTES // (B * G * read(ctx) * 2 * D * 2)) + 1)
    t = ctx - 1
    pos = torch.full((B,), t, dtype=torch.int32, device=dev)
    O = torch.empty(B, 1, G, H, D, device=dev, dtype=dt)
    ws_bytes = L.nsa_band_attn_fwd_paged_workspace(B, 1, G, H, D, D, DT)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    gen = torch.Generator()
    gen.manual_seed(1000 * B + P)
    tables = {"paged_identity": torch.arange(B * P, dtype=torch.int32).view(B, P).to(dev),
              "paged_permuted": torch.randperm(B * P, generator=gen).to(torch.int32).view(B, P).to(dev)}
    keep += [pos, O, ws, tables]
    ragged_args, paged_args = [], {k: [] for k in tables}
    for i in range(n_sets):
        g = torch.Generator(device="cuda")
        g.manual_seed(7 + 1009 * i)
        mk = lambda *sh: torch.randn(*sh, device=dev, generator=g, dtype=dt)  # noqa: E731
        Q, K, V, Kp, Vp = mk(B, 1, G, H, D), mk(B, G, cap, D), mk(B, G, cap, D), mk(B * P, G, rows, D), mk(B * P, G, rows, D)
        keep += [Q, K, V, Kp, Vp]
        ragged_args.append([Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), None, pos.data_ptr(), t, B, 1, G, H, D, D, cap, *strides(K, V), *band, DT, 0.0, 0,
                            ws.data_ptr(), ws_bytes, st])
        for k, tb in tables.items():
            paged_args[k].append([Q.data_ptr(), Kp.data_ptr(), Vp.data_ptr(), tb.data_ptr(), tb.stride(0), B * P, P, rows, O.data_ptr(), None, pos.data_ptr(), t, B, 1,
                                  G, H, D, D, *strides(Kp, Vp), *band, DT, 0.0, ws.data_ptr(), ws_bytes, st])

    def ragged(i):
        _lib.check(L.nsa_band_attn_fwd_ragged(*ragged_args[i]), "ragged")

    def paged(k):
        return lambda i: _lib.check(L.nsa_band_attn_fwd_paged(*paged_args[k][i]), k)

    return {"ragged": ragged, "paged_identity": paged("paged_identity"), "paged_permuted": paged("paged_permuted")}, n_sets, P, ws_bytes > 0


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    st = _stream(dev)
    res = {"library": _lib.loaded_library(), "shape": {"G": G, "h": H, "D": D, "dtype": "bf16", "S": 1, "w": W, "page_rows": {k: v[1] for k, v in BRANCHES.items()}},
           "steps_per_batch": NB, "batches": NBATCH, "reps": REPS, "cells": []}
    contexts = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4096, 16384]
    batches = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [16, 64, 256]
    for branch in BRANCHES:
        for ctx in contexts:
            for B in batches:
                keep = []
                routes, n_sets, P, split = cell_routes(branch, B, ctx, st, keep)
                r = measure(routes, n_sets)
                cell = {"branch": branch, "ctx": ctx, "B": B, "cache_sets": n_sets, "pages_per_sequence": P, "split": split}
                for k, (us, spread) in r.items():
                    cell[k + "_us"], cell[k + "_spread_us"] = us, spread
                print(json.dumps(cell), flush=True)
                res["cells"].append(cell)
                del keep, routes
                torch.cuda.empty_cache()
    print("\n| branch | context | B | sets | form | ragged, contiguous us | paged, identity table us | paged, permuted table us | spread us |\n|---|---|---|---|---|---|---|---|---|")
    for c in res["cells"]:
        print(f"| {c['branch']} | {c['ctx']} | {c['B']} | {c['cache_sets']} | {'split' if c['split'] else 'unsplit'} | {c['ragged_us']:.1f} | "
              f"{c['paged_identity_us']:.1f} | {c['paged_permuted_us']:.1f} | "
              f"{max(c['ragged_spread_us'], c['paged_identity_spread_us'], c['paged_permuted_spread_us']):.1f} |")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
