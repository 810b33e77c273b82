#!/usr/bin/env python3
"""Time the paged caches' admission copies on the GPU: NSA_PagedKV.load_sequence, gather_sequence and fork (one native launch each) against
the torch-indexing path they replaced -- one index copy per (pool, page), restated below as `indexed_load` / `indexed_gather` -- in the same
process, alternating, on cold pools (a 512 MiB write between timed calls pushes the pools out of the 256 MiB Infinity Cache).

m7c cache shape (G = 2, d_k = d_v = 64, bf16), t in {4k, 16k, 64k}.  For fork the comparison is what a caller had to do without sharing: a
full load of the prefix into a fresh slot.  Times are host clock around work that ends in a device synchronise (the indexed path is bound
by its launches, so kernel time alone would flatter it); each cell is the median of --repeats calls, with the spread (max - min) / median
of those repeats next to it.  Bytes per second: bytes read + bytes written by the copy over the median, next to the 8 TB/s HBM peak.

    python tools/bench_paged_admission.py [--repeats 9] [--out profiles/paged_admission]

Writes bench.json and bench.txt.  No default and no test depends on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nsa_vibe_amd.kv_cache import NSA_KV, NSA_PagedKV, PAGE_CMP, PAGE_TOKENS, _POOLS, n_cmp_at  # noqa: E402

G, D, DTYPE, PEAK = 2, 64, torch.bfloat16, 8.0e12
GEOM = (32, 16, 64, 16, 512)  # l, d, l_sel, n_sel, w


def indexed_load(pkv, b, kv1, t):
    """the copy NSA_PagedKV.load_sequence made before nsa_paged_kv_store: torch indexing, one copy per (pool, page)"""
    pkv.ensure(b, t)
    n_cmp = n_cmp_at(t, pkv.l, pkv.d)
    for name in _POOLS:
        rows, n = (PAGE_CMP, n_cmp) if name in ("_K_cmp", "_V_cmp") else (PAGE_TOKENS, t)
        pool, src = getattr(pkv, name), getattr(kv1, name)
        for j in range((n + rows - 1) // rows):
            k = min(rows, n - j * rows)
            pool[pkv.pages[b][j], :, :k] = src[0, :, j * rows:j * rows + k]


def indexed_gather(pkv, b, t):
    """... and NSA_PagedKV.gather_sequence before nsa_paged_kv_load"""
    cap = max(1, len(pkv.pages[b])) * PAGE_TOKENS
    kv1 = NSA_KV(1, pkv.G, pkv.d_k, pkv.d_v, cap, pkv.l, pkv.d, pkv.l_sel, pkv.n_sel, pkv.w, pkv._K_sel.device, pkv._K_sel.dtype, auto_grow=False)
    n_cmp = n_cmp_at(t, pkv.l, pkv.d)
    for name in _POOLS:
        rows, n = (PAGE_CMP, n_cmp) if name in ("_K_cmp", "_V_cmp") else (PAGE_TOKENS, t)
        pool, dst = getattr(pkv, name), getattr(kv1, name)
        dst.zero_()
        for j in range((n + rows - 1) // rows):
            k = min(rows, n - j * rows)
            dst[0, :, j * rows:j * rows + k] = pool[pkv.pages[b][j], :, :k]
    kv1.t, kv1.n_cmp = t, n_cmp
    return kv1


def copy_bytes(t, t0=0):
    """bytes read + written by a copy of token rows [t0, t) and their compressed rows"""
    return 2 * 2 * G * D * (6 * (t - t0) + 2 * (n_cmp_at(t, 32, 16) - n_cmp_at(t0, 32, 16)))


def fork_bytes(t):
    """... by the private copies of a fork at t: the open pages' rows below t"""
    total = 0
    for j in range((t + PAGE_TOKENS - 1) // PAGE_TOKENS):
        if t < PAGE_TOKENS * (j + 1) + 16:
            total += 2 * 2 * G * D * (6 * min(PAGE_TOKENS, t - PAGE_TOKENS * j) + 2 * max(0, min(PAGE_CMP, n_cmp_at(t, 32, 16) - PAGE_CMP * j)))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--lengths", type=int, nargs="*", default=[4096, 16384, 65536])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_admission"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_paged_admission: needs the GPU (no timing is taken anywhere else)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    def timed(fn, prepare=None):
        if prepare:
            prepare()
        flush.fill_(1)  # cold pools: nothing of them is left in the Infinity Cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    cells, lines = [], []
    for t in args.lengths:
        pages = (t + PAGE_TOKENS - 1) // PAGE_TOKENS
        pkv = NSA_PagedKV(2 * pages + 2, 2, pages, G, D, D, *GEOM, dev, DTYPE)
        kv1 = NSA_KV(1, G, D, D, pages * PAGE_TOKENS, *GEOM, dev, DTYPE, auto_grow=False)
        for name in _POOLS:
            getattr(kv1, name).normal_()
            getattr(pkv, name).zero_()
        pkv.ensure(0, t)
        free1 = lambda: pkv.free(1)  # noqa: E731
        ops = {
            "load_sequence": (lambda: pkv.load_sequence(0, kv1, t), lambda: indexed_load(pkv, 0, kv1, t), None, copy_bytes(t), copy_bytes(t)),
            "gather_sequence": (lambda: pkv.gather_sequence(0, t), lambda: indexed_gather(pkv, 0, t), None, copy_bytes(t), copy_bytes(t)),
            "fork": (lambda: pkv.fork(0, 1, t), lambda: indexed_load(pkv, 1, kv1, t), free1, fork_bytes(t), copy_bytes(t)),
        }
        for op, (native, parent, prepare, nbytes_native, nbytes_parent) in ops.items():
            for _ in range(2):  # warm-up: code objects, allocator
                timed(native, prepare)
                timed(parent, prepare)
            tn, tp = [], []
            for _ in range(args.repeats):  # alternating
                tn.append(timed(native, prepare)[0])
                tp.append(timed(parent, prepare)[0])
            if op == "load_sequence":  # the two paths leave the same bits
                pkv.load_sequence(0, kv1, t)
                a = {n: getattr(pkv, n).clone() for n in _POOLS}
                indexed_load(pkv, 0, kv1, t)
                assert all(torch.equal(a[n].view(torch.int16), getattr(pkv, n).view(torch.int16)) for n in _POOLS), "native and indexed load differ"
            if op == "gather_sequence":
                a, b = pkv.gather_sequence(0, t), indexed_gather(pkv, 0, t)
                assert all(torch.equal(getattr(a, n).view(torch.int16), getattr(b, n).view(torch.int16)) for n in _POOLS), "native and indexed gather differ"
            mn, mp = statistics.median(tn), statistics.median(tp)
            sn, sp = (max(tn) - min(tn)) / mn, (max(tp) - min(tp)) / mp
            spread = max(sn, sp)
            cell = {"op": op, "t": t, "native_ms": mn * 1e3, "parent_ms": mp * 1e3, "native_spread": sn, "parent_spread": sp, "speedup": mp / mn,
                    "native_bytes": nbytes_native, "native_TBps": nbytes_native / mn / 1e12, "native_share_of_peak": nbytes_native / mn / PEAK,
                    "parent_bytes": nbytes_parent, "parent_TBps": nbytes_parent / mp / 1e12, "meets_bar": bool(mn <= mp * (1 + spread)),
                    "repeats": args.repeats}
            cells.append(cell)
            lines.append(f"{op:16s} t={t:6d}  native {mn * 1e3:9.3f} ms (spread {sn:5.1%}, {cell['native_TBps']:6.3f} TB/s = {cell['native_share_of_peak']:5.1%} of "
                         f"8 TB/s)  parent path {mp * 1e3:9.3f} ms (spread {sp:5.1%}, {cell['parent_TBps']:6.3f} TB/s)  x{mp / mn:7.1f}  "
                         f"{'ok' if cell['meets_bar'] else 'MISSES THE BAR'}")
            print(lines[-1], flush=True)
        del pkv, kv1
        torch.cuda.empty_cache()
    os.makedirs(args.out, exist_ok=True)
    head = (f"paged admission copies, {torch.cuda.get_device_name(0)}, G = {G}, d_k = d_v = {D}, bf16, cold pools, host clock to synchronise, median of "
            f"{args.repeats} alternating repeats; bar: native <= parent path (1 + spread)")
    with open(os.path.join(args.out, "bench.json"), "w") as f:
        json.dump({"what": head, "peak_bytes_per_s": PEAK, "cells": cells}, f, indent=1)
    with open(os.path.join(args.out, "bench.txt"), "w") as f:
        f.write(head + "\n" + "\n".join(lines) + "\n")
    print(f"wrote {args.out}/bench.json and bench.txt")


if __name__ == "__main__":
    main()
