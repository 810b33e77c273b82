#!/usr/bin/env python3
"""nsa_kv_quantize_fp8 timed at the cache shapes of tools/bench_sel_decode_fp8.py (G = 2, D = 64, contexts 4k / 16k / 32k x B in {16, 64, 256}),
in its two uses: the one-row append (rows [t, t + 1) of every plane, one launch: what keeps a mirror current) and the whole cache at once.
With --other LIB the same calls of a second build of the library are timed IN THE SAME RUN, alternating (an A/B of two commits).

Through the C ABI with prepared arguments.  Cold: an append touches rows no earlier call of the run touched (t steps through the cache), a
whole-cache call rotates over so many cache sets that the others move >= 512 MiB between two uses of one.  Device events around batches of NB
calls; every cell is measured REPS times and the spread (max - min of the repeated medians) stands beside the median of medians: a
difference below the spread is no difference.  Bytes: 3 D + 4 per row (bf16 in, e4m3 and the scale out); the fraction is of 8 TB/s.

    python tools/bench_kv_quantize_fp8.py [--other OTHER.so] [OUT.json]     (the table goes to OUT.txt beside it)
"""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsa_vibe_amd import _lib  # noqa: E402
from nsa_vibe_amd.selection_scorer import _stream  # noqa: E402

G, D = 2, 64
NB, NBATCH, REPS = 10, 5, 3
COLD_BYTES = 512 * 2 ** 20
PEAK = 8.0e12
dev = torch.device("cuda")
FP8 = torch.float8_e4m3fn


def bind(path):
    fn = ctypes.CDLL(path).nsa_kv_quantize_fp8
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_int64] * 8 + [ctypes.c_void_p]
    return fn


def measure(routes):
    """routes: {name: f(call index)} -> {name: (median of medians us per call, spread us)}"""
    pos = {k: 0 for k in routes}
    for k, f in routes.items():
        for _ in range(3):
            f(pos[k])
            pos[k] += 1
    torch.cuda.synchronize()
    med = {k: [] for k in routes}
    for rep in range(REPS):
        ts = {k: [] for k in routes}
        for nb in range(NBATCH):
            order = list(routes.items())
            if (rep + nb) & 1:  # alternating orders: no route always runs behind the same other one
                order.reverse()
            for k, f in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(NB):
                    f(pos[k])
                    pos[k] += 1
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / NB)
        for k in routes:
            med[k].append(statistics.median(ts[k]))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in med.items()}


def main():
    argv = sys.argv[1:]
    other = None
    if "--other" in argv:
        i = argv.index("--other")
        other = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    out_path = argv[0] if argv else None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libs = {"this": bind(os.path.join(root, _lib.loaded_library()["path"]))}
    if other:
        libs["other"] = bind(other)
    st = _stream(dev)
    res = {"library": _lib.loaded_library(), "other": other, "shape": {"G": G, "D": D}, "calls_per_batch": NB, "batches": NBATCH, "reps": REPS, "cells": []}
    for ctx in (4096, 16384, 32768):
        for B in (16, 64, 256):
            whole = B * G * ctx * (3 * D + 4)
            n_sets = max(2, min(24, -(-COLD_BYTES // whole) + 1))
            sets = []
            for i in range(n_sets):
                X = torch.randn((B, G, ctx, D), device=dev, dtype=torch.bfloat16, generator=torch.Generator(device="cuda").manual_seed(7 + i))
                sets.append((X, torch.empty(X.shape, device=dev, dtype=FP8), torch.empty(X.shape[:3], device=dev)))

            def call(fn, s, t0, t1):
                X, X8, z = s
                rc = fn(X.data_ptr(), X8.data_ptr(), z.data_ptr(), B, G, ctx, D, t0, t1, *X.stride()[:3], *X8.stride()[:3], *z.stride()[:2], st)
                assert rc == 0, rc

            # (append: call i of library j takes row 2 (i // n_sets) + j of set i % n_sets -- the two libraries walk disjoint rows)
            for kind in ("append", "whole"):
                routes = {}
                for j, (name, fn) in enumerate(libs.items()):
                    if kind == "append":
                        routes[name] = lambda i, fn=fn, j=j: call(fn, sets[i % n_sets], (2 * (i // n_sets) + j) % ctx, (2 * (i // n_sets) + j) % ctx + 1)
                    else:
                        routes[name] = lambda i, fn=fn: call(fn, sets[i % n_sets], 0, ctx)
                r = measure(routes)
                by = whole if kind == "whole" else B * G * (3 * D + 4)
                cell = {"ctx": ctx, "B": B, "use": kind, "cache_sets": n_sets, "bytes": by}
                for k, (us, spread) in r.items():
                    cell[k] = {"us": us, "spread_us": spread, "hbm_fraction": by / (us * 1e-6) / PEAK}
                print(json.dumps(cell), flush=True)
                res["cells"].append(cell)
            del sets
            torch.cuda.empty_cache()
    names = list(libs)
    lines = ["| context | B | use | sets | MiB | " + " | ".join(f"{n} us (HBM) | {n} spread us" for n in names) + " |", "|---" * (5 + 2 * len(names)) + "|"]
    for c in res["cells"]:
        lines.append(f"| {c['ctx']} | {c['B']} | {c['use']} | {c['cache_sets']} | {c['bytes'] / 2 ** 20:.2f} | " +
                     " | ".join(f"{c[n]['us']:.2f} ({c[n]['hbm_fraction']:.2f}) | {c[n]['spread_us']:.2f}" for n in names) + " |")
    print("\n" + "\n".join(lines))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.splitext(out_path)[0] + ".txt", "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
