#!/usr/bin/env python3
"""The ragged layer decode with FP8 mirrors (nsa_layer_decode_ragged_fp8) against the bf16 ragged call of the SAME library and,
for reference, the paged FP8 call (nsa_layer_decode_paged_fp8, identity table), timed in the same run on the m7c layer (dim 768, 12 heads,
G = 2, D = 64, bf16): contexts {4k, 16k} x B in {16, 64, 256} x S in {1, 4}, every sequence at position context - S.  One cell per process
(the driver below starts them, each under its own timeout, and stops at the first that fails).  COLD as
tools/bench_layer_decode_paged_fp8.py: the steps of a route rotate over independent cache sets, so many that the others load >= 512 MiB
between two uses of one set (at most 32).  The routes alternate in an order that changes from batch to batch; every cell is measured REPS
times and the spread (max - min of the repeated medians) stands beside the median of medians: a difference below the spread is no
difference.  No default depends on these numbers.

    python tools/bench_layer_decode_ragged_fp8.py [OUT.json]          (default OUT: profiles/layer_decode_ragged_fp8/bench.json)
    python tools/bench_layer_decode_ragged_fp8.py --cell CTX B S      (one cell: prints its JSON line)
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, HEADS, G, D, N = 768, 12, 2, 64, 16
L_, D_, LS, W = 32, 16, 64, 512
NB, NBATCH, REPS = 10, 6, 3
COLD_BYTES = 512 * 2 ** 20
CELL_TIMEOUT = 170
ROUTES = ("bf16", "fp8", "paged_fp8")


def cell(ctx, B, S):
    import torch

    import nsa_vibe_amd as nv
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.kv_cache import _MIRRORED, _POOLS
    from nsa_vibe_amd.selection_scorer import _stream

    dev, dt, L = torch.device("cuda"), torch.bfloat16, _lib.lib()
    torch.manual_seed(1)
    m = nv.NSAAttention(DIM, HEADS, G, D, D, l=L_, d=D_, l_sel=LS, n_sel=N, w=W, selector="sequential").cuda().to(dt).eval()
    P, t_max = ctx // 1024, ctx - 1
    n_cmp = (ctx - L_) // D_ + 1
    step_bytes = B * G * ((min(N * LS, ctx) + min(W, ctx)) * 2 * D + n_cmp * 2 * D)  # what a step of an FP8 route reads: the smallest of the three
    n_sets = min(32, -(-COLD_BYTES // step_bytes) + 1)
    desc, _ = m._layer_desc()
    dref, st = ctypes.byref(desc), _stream(dev)
    meta = nv.build_block_meta(t_max + 1, L_, D_, LS, N, W)
    csc = [c.data_ptr() for c in meta.device_csc(dev)]
    x = torch.randn(B, S, DIM, device=dev, dtype=dt)
    y = torch.empty(B, S, DIM, device=dev, dtype=dt)
    rg = torch.empty(B, S, G, N, 2, device=dev, dtype=torch.int32)
    gt = torch.empty(B, S, G, 3, device=dev, dtype=torch.float32)
    pos = torch.full((B,), ctx - S, dtype=torch.int32, device=dev)
    nb = max(L.nsa_layer_decode_ragged_workspace(dref, B, S, ctx), L.nsa_layer_decode_paged_fp8_workspace(dref, B, S, P))
    assert L.nsa_layer_decode_ragged_workspace(dref, B, S, ctx) == L.nsa_layer_decode_ragged_fp8_workspace(dref, B, S, ctx)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
    wptr = (ws.data_ptr() + 255) & ~255
    sets, args = [], {k: [] for k in ROUTES}

    def mirrors(kv):  # finite bytes, scales near those of N(0, 1) rows
        for name in _MIRRORED:
            getattr(kv, name + "8").view(torch.uint8).random_(0, 0x78)
            getattr(kv, name + "_scale").fill_(0.008)

    with torch.no_grad():
        for _ in range(n_sets):
            kv = m.new_kv(B, ctx, dev, dt, kv_dtype=torch.float8_e4m3fn)
            pkv = m.new_paged_kv(B * P, B, P, dev, dt, kv_dtype=torch.float8_e4m3fn)
            for name in _POOLS:
                getattr(kv, name).normal_()
                getattr(pkv, name).normal_()
            mirrors(kv)
            mirrors(pkv)
            pkv.block_table.copy_(torch.arange(B * P, dtype=torch.int32).view(B, P))
            sets.append((kv, pkv))
            head = [x.data_ptr(), y.data_ptr(), pos.data_ptr(), t_max, S, *csc, int(meta.S_sel), rg.data_ptr(), gt.data_ptr(), wptr, nb, st]
            args["bf16"].append([dref, ctypes.byref(kv.native_desc()), *head])
            args["fp8"].append([dref, ctypes.byref(kv.native_desc()), ctypes.byref(kv.native_fp8_desc()), *head])
            args["paged_fp8"].append([dref, ctypes.byref(pkv.native_desc()), ctypes.byref(pkv.native_fp8_desc()), *head])
        fns = {"bf16": L.nsa_layer_decode_ragged, "fp8": L.nsa_layer_decode_ragged_fp8, "paged_fp8": L.nsa_layer_decode_paged_fp8}
        run = lambda k, i: _lib.check(fns[k](*args[k][i]), k)  # noqa: E731
        at = {k: 0 for k in fns}
        for k in fns:
            for i in range(n_sets):
                run(k, i)
        torch.cuda.synchronize()
        med = {k: [] for k in fns}
        for rep in range(REPS):
            ts = {k: [] for k in fns}
            for bt in range(NBATCH):
                order = ROUTES[(rep + bt) % 3:] + ROUTES[:(rep + bt) % 3]  # alternating, in changing order
                for k in (order if (rep + bt) % 2 == 0 else order[::-1]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(NB):
                        run(k, at[k] % n_sets)
                        at[k] += 1
                    e1.record()
                    e1.synchronize()
                    ts[k].append(e0.elapsed_time(e1) * 1e3 / NB)
            for k in fns:
                med[k].append(statistics.median(ts[k]))
    S_sel = int(meta.S_sel)
    c = {"ctx": ctx, "B": B, "S": S, "sets": n_sets, "library": _lib.loaded_library(),
         "launches": {"bf16": m.decode_ragged_plan(B, S, ctx, t_max, S_sel)["launches"], "fp8": m.decode_ragged_plan(B, S, ctx, t_max, S_sel, fp8=True)["launches"],
                      "paged_fp8": m.decode_paged_plan(B, S, P, t_max, S_sel, fp8=True)["launches"]}}
    for k in fns:
        c[k + "_us"], c[k + "_spread_us"] = statistics.median(med[k]), max(med[k]) - min(med[k])
    c["spread_us"] = max(c["bf16_spread_us"], c["fp8_spread_us"])
    c["fp8_minus_bf16_us"] = c["fp8_us"] - c["bf16_us"]
    c["inside_spread"] = abs(c["fp8_minus_bf16_us"]) <= c["spread_us"]
    print(json.dumps(c), flush=True)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "layer_decode_ragged_fp8", "bench.json")
    cells = []
    for ctx in (4096, 16384):
        for B in (16, 64, 256):
            for S in (1, 4):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cell", str(ctx), str(B), str(S)], capture_output=True, text=True,
                                   timeout=CELL_TIMEOUT)
                if r.returncode != 0:  # nothing more is started on the device behind a cell that failed
                    sys.exit(f"cell ctx={ctx} B={B} S={S} ended with status {r.returncode}:\n{r.stderr[-2000:]}")
                cells.append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(json.dumps(cells[-1]), flush=True)
    lines = ["| context | B | S | sets | launches bf16 / fp8 / paged fp8 | bf16 us | fp8 us | spread us | fp8 - bf16 | inside the spread | paged fp8 us |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in cells:
        n = c["launches"]
        lines.append(f"| {c['ctx']} | {c['B']} | {c['S']} | {c['sets']} | {n['bf16']} / {n['fp8']} / {n['paged_fp8']} | {c['bf16_us']:.1f} | {c['fp8_us']:.1f} | "
                     f"{c['spread_us']:.1f} | {c['fp8_minus_bf16_us']:+.1f} us ({100 * c['fp8_minus_bf16_us'] / c['bf16_us']:+.0f}%) | "
                     f"{'yes' if c['inside_spread'] else 'no'} | {c['paged_fp8_us']:.1f} |")
    table = "\n".join(lines)
    print("\n" + table)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"shape": {"dim": DIM, "heads": HEADS, "G": G, "D": D, "n_sel": N, "dtype": "bf16"}, "steps_per_batch": NB, "batches": NBATCH, "reps": REPS,
                   "cells": cells}, f, indent=1)
    with open(os.path.splitext(out_path)[0] + ".txt", "w") as f:
        f.write(f"library {cells[0]['library']}\n\n{table}\n")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--cell":
        cell(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
