#!/usr/bin/env python3
"""The FP8 K/V decode calls (nsa_sel_decode_ragged_fp8, nsa_sel_decode_paged_fp8) against the bf16 calls of the same library
(nsa_sel_decode_ragged, nsa_sel_decode_paged), timed IN THE SAME RUN, alternating, on the m7c shape (G = 2, h = 6, D = 64, bf16 Q, n = 16):
contexts 4k / 16k / 32k x B in {16, 64, 256}, S = 1, with equal positions (ctx - 1) and with positions drawn uniformly from
[ctx / 4, ctx), ragged (contiguous caches) and paged (identity table over pools that hold the same rows).  The FP8 caches are the bf16
ones through nsa_kv_quantize_fp8; K_cmp is shared, so all four routes select the same blocks.

Everything goes through the C ABI with prepared arguments.  COLD, in the method of tools/bench_sel_decode_ragged.py: the steps rotate over
independent cache sets, so many that the others load >= 512 MiB (counted in FP8 bytes, the smaller figure) between two uses of one set.
Device events around batches of NB steps; every cell is measured REPS times and the spread (max - min of the repeated medians) stands
beside the median of medians: a difference below the spread is no difference.  Bytes are the algorithmic ones of a step -- per (b, g) the
K_cmp sweep n_cmp(t) D 2 and the gathered rows min(n 64, t + 1) of K and V at 2 D 2 (bf16) or 2 D + 8 (FP8 with its two scales) -- and
the fraction is of 8 TB/s.

    python tools/bench_sel_decode_fp8.py [OUT.json]     (the table goes to OUT.txt beside it)
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
PAGE = 1024
PEAK = 8.0e12
dt = torch.bfloat16
dev = torch.device("cuda")
L = _lib.lib()
DT = _DT[dt]


def ncmp(t):
    return 0 if t + 1 < L_ else (t + 1 - L_) // D_ + 1


def strides(*ts):
    return [x.stride(i) for x in ts for i in range(3)]


def step_bytes(positions, fp8):
    row = 2 * D + 8 if fp8 else 2 * D * 2
    return sum(G * (ncmp(t) * D * 2 + min(N * LS, t + 1) * row) for t in positions)


def as_pool(X, rows):
    """[B, G, J rows, ...] -> the pool [B J, G, rows, ...] whose page b J + j holds rows [rows j, rows j + rows) of sequence b (a copy)"""
    B, J = X.shape[0], X.shape[2] // rows
    return X.view(B, G, J, rows, *X.shape[3:]).transpose(1, 2).reshape(B * J, G, rows, *X.shape[3:]).contiguous()


def make_set(B, J, seed):
    """one cache set of B sequences with room for J pages: contiguous bf16 and FP8 caches and the same rows as pools"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mk = lambda *sh: torch.randn(*sh, device=dev, generator=g, dtype=dt)  # noqa: E731
    s = dict(Q=mk(B, 1, G, H, D), Kc=mk(B, G, J * (PAGE // 16), D), K=mk(B, G, J * PAGE, D), V=mk(B, G, J * PAGE, D))
    (s["K8"], s["kz"]), (s["V8"], s["vz"]) = nv.quantize_kv_fp8(s["K"]), nv.quantize_kv_fp8(s["V"])
    for k, rows in (("Kc", PAGE // 16), ("K", PAGE), ("V", PAGE), ("K8", PAGE), ("V8", PAGE), ("kz", PAGE), ("vz", PAGE)):
        s["p" + k] = as_pool(s[k], rows)
    return s


def measure(routes, n_sets):
    """routes: {name: f(set index)} -> {name: (median of medians us per step, spread us)}"""
    pos = {k: 0 for k in routes}
    for f in routes.values():
        for i in range(n_sets):
            f(i)
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
                    f(pos[k] % n_sets)
                    pos[k] += 1
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / NB)
        for k in routes:
            med[k].append(statistics.median(ts[k]))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in med.items()}


def routes_of(B, J, positions, sets, st, keep):
    t_max = max(positions)
    meta = nv.build_block_meta(t_max + 1, L_, D_, LS, N, W)
    csc = [c.data_ptr() for c in meta.device_csc(dev)]
    pos_dev = torch.tensor(positions, dtype=torch.int32, device=dev)
    table = torch.arange(B * J, dtype=torch.int32, device=dev).view(B, J)
    O = torch.empty(B, 1, G, H, D, device=dev, dtype=dt)
    rg = torch.empty(B, 1, G, N, 2, device=dev, dtype=torch.int32)
    keep += [meta, pos_dev, table, O, rg]
    shape = [B, 1, G, H, D, D, meta.S_cmp, meta.S_sel]
    geo = [L_, D_, LS, N]
    tail = [DT, 0.0, None, 0, st]
    args = {"ragged_bf16": [], "ragged_fp8": [], "paged_bf16": [], "paged_fp8": []}
    for s in sets:
        p = lambda k: s[k].data_ptr()  # noqa: E731
        out = [rg.data_ptr(), O.data_ptr(), pos_dev.data_ptr(), t_max]
        args["ragged_bf16"].append([p("Q"), p("Kc"), p("K"), p("V"), *csc, *out, *shape, J * PAGE, *geo, *strides(s["Kc"], s["K"], s["V"]), *tail])
        args["ragged_fp8"].append([p("Q"), p("Kc"), p("K8"), p("V8"), p("kz"), p("vz"), *csc, *out, *shape, J * PAGE, *geo,
                                   *strides(s["Kc"], s["K8"], s["V8"]), *strides(s["kz"])[:2], *strides(s["vz"])[:2], *tail])
        tb = [table.data_ptr(), table.stride(0), B * J, J, PAGE]
        args["paged_bf16"].append([p("Q"), p("pKc"), p("pK"), p("pV"), *tb, *csc, *out, *shape, *geo, *strides(s["pKc"], s["pK"], s["pV"]), *tail])
        args["paged_fp8"].append([p("Q"), p("pKc"), p("pK8"), p("pV8"), p("pkz"), p("pvz"), *tb, *csc, *out, *shape, *geo,
                                  *strides(s["pKc"], s["pK8"], s["pV8"]), *strides(s["pkz"])[:2], *strides(s["pvz"])[:2], *tail])
    fns = {"ragged_bf16": L.nsa_sel_decode_ragged, "ragged_fp8": L.nsa_sel_decode_ragged_fp8, "paged_bf16": L.nsa_sel_decode_paged,
           "paged_fp8": L.nsa_sel_decode_paged_fp8}

    def route(k):
        return lambda i: _lib.check(fns[k](*args[k][i]), k)

    return {k: route(k) for k in fns}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    st = _stream(dev)
    res = {"library": _lib.loaded_library(), "shape": {"G": G, "h": H, "D": D, "n_top": N, "S": 1, "q_dtype": "bf16"}, "steps_per_batch": NB,
           "batches": NBATCH, "reps": REPS, "peak_bytes_per_s": PEAK, "cells": []}
    for ctx in (4096, 16384, 32768):
        J = ctx // PAGE
        for B in (16, 64, 256):
            gen = torch.Generator()
            gen.manual_seed(ctx + B)
            drawn = sorted(int(v) for v in torch.randint(ctx // 4, ctx, (B,), generator=gen))
            n_sets = min(32, -(-COLD_BYTES // step_bytes(drawn, True)) + 1)
            sets = [make_set(B, J, 7 + 1009 * i) for i in range(n_sets)]
            for kind, positions in (("equal", [ctx - 1] * B), ("drawn", drawn)):
                keep = []
                r = measure(routes_of(B, J, positions, sets, st, keep), n_sets)
                cell = {"ctx": ctx, "B": B, "positions": kind, "cache_sets": n_sets, "bytes_bf16": step_bytes(positions, False),
                        "bytes_fp8": step_bytes(positions, True)}
                for k, (us, spread) in r.items():
                    by = cell["bytes_fp8" if k.endswith("fp8") else "bytes_bf16"]
                    cell[k] = {"us": us, "spread_us": spread, "hbm_fraction": by / (us * 1e-6) / PEAK}
                print(json.dumps(cell), flush=True)
                res["cells"].append(cell)
                del keep
            del sets
            torch.cuda.empty_cache()
    lines = ["| context | B | positions | sets | MiB bf16 / fp8 | ragged bf16 us (HBM) | ragged fp8 us (HBM) | paged bf16 us (HBM) | paged fp8 us (HBM) | spread us | fp8 faster |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        f = lambda k: f"{c[k]['us']:.1f} ({c[k]['hbm_fraction']:.2f})"  # noqa: E731
        spread = max(c[k]["spread_us"] for k in ("ragged_bf16", "ragged_fp8", "paged_bf16", "paged_fp8"))
        won = [m for m in ("ragged", "paged") if c[m + "_bf16"]["us"] - c[m + "_fp8"]["us"] > spread]
        lines.append(f"| {c['ctx']} | {c['B']} | {c['positions']} | {c['cache_sets']} | {c['bytes_bf16'] / 2 ** 20:.1f} / {c['bytes_fp8'] / 2 ** 20:.1f} | "
                     f"{f('ragged_bf16')} | {f('ragged_fp8')} | {f('paged_bf16')} | {f('paged_fp8')} | {spread:.1f} | {' + '.join(won) or 'no'} |")
    print("\n" + "\n".join(lines))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.splitext(out_path)[0] + ".txt", "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
