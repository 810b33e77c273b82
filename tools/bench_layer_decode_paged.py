#!/usr/bin/env python3
"""The layer's paged decode call (nsa_layer_decode_paged) against the ragged call on contiguous slabs, timed IN THE SAME RUN,
alternating, on the m7c layer (dim 768, 12 heads, G = 2, D = 64, bf16), contexts {4k, 16k} x B in {16, 64} x S in {1, 4}, every sequence
at position context - S.  Three routes:

  ragged      nsa_layer_decode_ragged on slabs of capacity = the context (the parent's code: the baseline);
  identity    nsa_layer_decode_paged on pools of B context / 1024 pages, sequence b in pages b P .. b P + P - 1 in order;
  permuted    the same call, the same pools, a seeded permutation of all page ids in the table.

Everything goes through the C ABI with prepared arguments.  COLD, as tools/bench_sel_decode_paged.py and tools/bench_layer_decode_ragged.py:
the steps of a route rotate over independent cache sets, so many that the others load >= 512 MiB between two uses of one set (at most 32).
The two paged routes share their sets' storage (they differ in the table alone).  Device events around batches of NB steps; every cell is
measured REPS times and the spread (max - min of the repeated medians) is printed beside the median of medians: a difference below the
spread is no difference.  Not measured: D = 128, warm caches, B > 64, mixed positions, pages shared between sequences.

    python tools/bench_layer_decode_paged.py [OUT.json]     (default OUT: profiles/layer_decode_paged/bench.json)
"""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nsa_vibe_amd as nv  # noqa: E402
from nsa_vibe_amd import _lib  # noqa: E402
from nsa_vibe_amd.selection_scorer import _stream  # noqa: E402

DIM, HEADS, G, D, N = 768, 12, 2, 64, 16
L_, D_, LS, W = 32, 16, 64, 512
NB, NBATCH, REPS = 10, 5, 3
COLD_BYTES = 512 * 2 ** 20
CACHES = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp")
dt = torch.bfloat16
dev = torch.device("cuda")
L = _lib.lib()


def ncmp(n_tok):
    return 0 if n_tok < L_ else (n_tok - L_) // D_ + 1


def aligned(nbytes):
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return buf, (buf.data_ptr() + 255) & ~255


def n_sets_for(B, ctx):
    step = B * G * ((min(N * LS, ctx) + min(W, ctx)) * 2 * D * 2 + ncmp(ctx) * 2 * D * 2)
    return min(32, -(-COLD_BYTES // step) + 1)


def measure(routes, n_sets):
    """routes: {name: f(set index)} -> {name: (median of medians us per step, spread us)}"""
    pos = {k: 0 for k in routes}
    for f in routes.values():
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


def paged_desc(pkv, table):
    """nsa_paged_kv_desc of the pools of pkv with another table (the descriptor NSA_PagedKV builds names its own)"""
    d = _lib.NsaPagedKvDesc()
    for name in CACHES:
        setattr(d, name[1:], getattr(pkv, name).data_ptr())
    d.block_table, d.table_stride = table.data_ptr(), table.stride(0)
    d.n_pages, d.B, d.max_pages = pkv.n_pages, pkv.B, pkv.max_pages
    return d


def cell_routes(m, B, S, ctx, slabs, paged, tables, keep):
    desc, _ = m._layer_desc()
    dref, st = ctypes.byref(desc), _stream(dev)
    P = ctx // 1024
    t_max = ctx - 1
    meta = nv.build_block_meta(t_max + 1, L_, D_, LS, N, W)
    csc = [c.data_ptr() for c in meta.device_csc(dev)]
    x = torch.randn(B, S, DIM, device=dev, dtype=dt)
    y = torch.empty(B, S, DIM, device=dev, dtype=dt)
    rg = torch.empty(B, S, G, N, 2, device=dev, dtype=torch.int32)
    gt = torch.empty(B, S, G, 3, device=dev, dtype=torch.float32)
    pos_dev = torch.full((B,), ctx - S, dtype=torch.int32, device=dev)
    wr, pr = aligned(L.nsa_layer_decode_ragged_workspace(dref, B, S, ctx))
    wp, pp = aligned(L.nsa_layer_decode_paged_workspace(dref, B, S, P))
    keep += [meta, x, y, rg, gt, pos_dev, wr, wp]
    tail = [*csc, int(meta.S_sel), rg.data_ptr(), gt.data_ptr()]
    sd = [kv.native_desc() for kv in slabs]
    ragged_args = [[dref, ctypes.byref(kd), x.data_ptr(), y.data_ptr(), pos_dev.data_ptr(), t_max, S, *tail, pr, wr.numel() - 256, st] for kd in sd]
    keep.append(sd)
    routes = {"ragged": lambda i: _lib.check(L.nsa_layer_decode_ragged(*ragged_args[i]), "ragged")}
    for name, table in tables.items():
        pd = [paged_desc(pkv, table) for pkv in paged]
        args = [[dref, ctypes.byref(kd), x.data_ptr(), y.data_ptr(), pos_dev.data_ptr(), t_max, S, *tail, pp, wp.numel() - 256, st] for kd in pd]
        keep += [pd, args]
        routes[name] = (lambda a: lambda i: _lib.check(L.nsa_layer_decode_paged(*a[i]), "paged"))(args)
    plans = {"ragged": m.decode_ragged_plan(B, S, ctx, t_max, int(meta.S_sel))["launches"], "paged": m.decode_paged_plan(B, S, P, t_max, int(meta.S_sel))["launches"]}
    return routes, plans


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "layer_decode_paged", "bench.json")
    torch.manual_seed(1)
    m = nv.NSAAttention(DIM, HEADS, G, D, D, l=L_, d=D_, l_sel=LS, n_sel=N, w=W, selector="sequential").cuda().to(dt).eval()
    res = {"library": _lib.loaded_library(), "shape": {"dim": DIM, "heads": HEADS, "G": G, "D": D, "n_sel": N, "dtype": "bf16"},
           "steps_per_batch": NB, "batches": NBATCH, "reps": REPS, "cells": []}
    print(json.dumps({"library": res["library"]}), flush=True)
    with torch.no_grad():
        for ctx in (4096, 16384):
            P = ctx // 1024
            for B in (16, 64):
                n_sets = n_sets_for(B, ctx)
                slabs, paged = [], []
                for _ in range(n_sets):
                    kv = m.new_kv(B, ctx, dev, dt)
                    pkv = m.new_paged_kv(B * P, B, P, dev, dt)
                    for name in CACHES:
                        getattr(kv, name).normal_()
                        getattr(pkv, name).normal_()
                    slabs.append(kv)
                    paged.append(pkv)
                gen = torch.Generator()
                gen.manual_seed(100 + B + ctx)
                tables = {"identity": torch.arange(B * P, dtype=torch.int32).view(B, P).to(dev),
                          "permuted": torch.randperm(B * P, generator=gen).to(torch.int32).view(B, P).to(dev)}
                for S in (1, 4):
                    keep = []
                    routes, plans = cell_routes(m, B, S, ctx, slabs, paged, tables, keep)
                    r = measure(routes, n_sets)
                    cell = {"ctx": ctx, "B": B, "S": S, "sets": n_sets, "launches": plans}
                    for k, (us, sp) in r.items():
                        cell[k + "_us"], cell[k + "_spread_us"] = us, sp
                    spread = max(sp for _, sp in r.values())
                    cell["spread_us"] = spread
                    cell["identity_behind_us"] = r["identity"][0] - r["ragged"][0]
                    cell["permuted_behind_us"] = r["permuted"][0] - r["ragged"][0]
                    cell["identity_inside_spread"] = abs(cell["identity_behind_us"]) <= spread
                    cell["permuted_inside_spread"] = abs(cell["permuted_behind_us"]) <= spread
                    cell["table_order_inside_spread"] = abs(r["permuted"][0] - r["identity"][0]) <= spread
                    print(json.dumps(cell), flush=True)
                    res["cells"].append(cell)
                    del routes, keep
                del slabs, paged, tables
                torch.cuda.empty_cache()
    lines = ["| context | B | S | sets | launches ragged / paged | ragged us | paged identity us | paged permuted us | spread us | identity behind by | "
             "permuted behind by | inside the spread |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        inside = ", ".join(k for k in ("identity", "permuted") if c[k + "_inside_spread"]) or "neither"
        lines.append(f"| {c['ctx']} | {c['B']} | {c['S']} | {c['sets']} | {c['launches']['ragged']} / {c['launches']['paged']} | {c['ragged_us']:.1f} | "
                     f"{c['identity_us']:.1f} | {c['permuted_us']:.1f} | {c['spread_us']:.1f} | {c['identity_behind_us']:+.1f} us "
                     f"({100 * c['identity_behind_us'] / c['ragged_us']:+.0f}%) | {c['permuted_behind_us']:+.1f} us ({100 * c['permuted_behind_us'] / c['ragged_us']:+.0f}%) | "
                     f"{inside} |")
    table = "\n".join(lines)
    print("\n" + table)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(out_path)[0] + ".txt", "w") as f:
        f.write(f"library {res['library']}\n\n{table}\n")


if __name__ == "__main__":
    main()
