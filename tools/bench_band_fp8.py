#!/usr/bin/env python3
"""The FP8 K/V band calls (nsa_band_attn_fwd_ragged_fp8, nsa_band_attn_fwd_paged_fp8) against the bf16 calls of the same library
(nsa_band_attn_fwd_ragged, nsa_band_attn_fwd_paged), timed IN THE SAME RUN, alternating, on the m7c shape (G = 2, h = 6, D = 64, bf16 Q):
the sliding (w = 512) and the compressed (l = 32, d = 16) branch of a decode step, S = 1, every sequence at position ctx - 1, contexts
4k / 16k / 64k x B in {16, 64, 256}, ragged (contiguous caches) and paged (identity table over pools that hold the same rows; pages of 1024 /
64 rows).  The FP8 caches are the bf16 ones through nsa_kv_quantize_fp8.

Everything goes through the C ABI with prepared arguments.  COLD, in the method of tools/bench_sel_decode_fp8.py: the steps rotate over
independent cache sets, so many that the others load >= 512 MiB (counted in FP8 bytes) between two uses of one set.  The sliding branch reads
the last w rows only, so its caches hold the sequence's last page (the table's other entries point at it too; the ragged call gets positions
inside that page): a set stays small at 64k.  Device events around batches of NB steps; every cell is measured REPS times and the spread (max -
min of the repeated medians) stands beside the median of medians: a difference below the spread is no difference.  Bytes are the algorithmic
ones of a step -- per (b, g) the rows of the interval at 2 D 2 (bf16) or 2 D + 8 (FP8 with its two scales) -- and the fraction is of 8 TB/s.

    python tools/bench_band_fp8.py [OUT.json]     (the table goes to OUT.txt beside it)
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

G, H, D = 2, 6, 64
L_, D_, W = 32, 16, 512
NB, NBATCH, REPS = 10, 5, 3
COLD_BYTES = 512 * 2 ** 20
PEAK = 8.0e12
dt = torch.bfloat16
dev = torch.device("cuda")
L = _lib.lib()
DT = _DT[dt]


def strides(*ts):
    return [x.stride(i) for x in ts for i in range(3)]


def as_pool(X, rows):
    """[B, G, J rows, ...] -> the pool [B J, G, rows, ...] whose page b J + j holds rows [rows j, rows j + rows) of sequence b (a copy)"""
    B, J = X.shape[0], X.shape[2] // rows
    return X.view(B, G, J, rows, *X.shape[3:]).transpose(1, 2).reshape(B * J, G, rows, *X.shape[3:]).contiguous()


def make_set(B, n_rows, page, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mk = lambda *sh: torch.randn(*sh, device=dev, generator=g, dtype=dt)  # noqa: E731
    s = dict(Q=mk(B, 1, G, H, D), K=mk(B, G, n_rows, D), V=mk(B, G, n_rows, D))
    (s["K8"], s["kz"]), (s["V8"], s["vz"]) = nv.quantize_kv_fp8(s["K"]), nv.quantize_kv_fp8(s["V"])
    for k in ("K", "V", "K8", "V8", "kz", "vz"):
        s["p" + k] = as_pool(s[k], page)
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


def routes_of(B, band, t_ragged, t_paged, n_rows, page, max_pages, table, sets, st, keep):
    """ragged: positions t_ragged over caches of n_rows rows; paged: positions t_paged through `table` [B, max_pages]"""
    pr = torch.full((B,), t_ragged, dtype=torch.int32, device=dev)
    pp = torch.full((B,), t_paged, dtype=torch.int32, device=dev)
    O = torch.empty(B, 1, G, H, D, device=dev, dtype=dt)
    need = L.nsa_band_attn_fwd_ragged_workspace(B, 1, G, H, D, D, DT)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    keep += [pr, pp, O, ws, table]
    wsa = [ws.data_ptr() if need else None, need, st]
    shape = [B, 1, G, H, D, D]
    args = {"ragged_bf16": [], "ragged_fp8": [], "paged_bf16": [], "paged_fp8": []}
    for s in sets:
        p = lambda k: s[k].data_ptr()  # noqa: E731
        tb = [table.data_ptr(), table.stride(0), s["pK"].shape[0], max_pages, page]
        args["ragged_bf16"].append([p("Q"), p("K"), p("V"), O.data_ptr(), None, pr.data_ptr(), t_ragged, *shape, n_rows, *strides(s["K"], s["V"]), *band, DT, 0.0, 0, *wsa])
        args["ragged_fp8"].append([p("Q"), p("K8"), p("V8"), p("kz"), p("vz"), O.data_ptr(), None, pr.data_ptr(), t_ragged, *shape, n_rows, *strides(s["K8"], s["V8"]),
                                   *strides(s["kz"])[:2], *strides(s["vz"])[:2], *band, DT, 0.0, *wsa])
        args["paged_bf16"].append([p("Q"), p("pK"), p("pV"), *tb, O.data_ptr(), None, pp.data_ptr(), t_paged, *shape, *strides(s["pK"], s["pV"]), *band, DT, 0.0, *wsa])
        args["paged_fp8"].append([p("Q"), p("pK8"), p("pV8"), p("pkz"), p("pvz"), *tb, O.data_ptr(), None, pp.data_ptr(), t_paged, *shape, *strides(s["pK8"], s["pV8"]),
                                  *strides(s["pkz"])[:2], *strides(s["pvz"])[:2], *band, DT, 0.0, *wsa])
    fns = {"ragged_bf16": L.nsa_band_attn_fwd_ragged, "ragged_fp8": L.nsa_band_attn_fwd_ragged_fp8, "paged_bf16": L.nsa_band_attn_fwd_paged,
           "paged_fp8": L.nsa_band_attn_fwd_paged_fp8}

    def route(k):
        return lambda i: _lib.check(fns[k](*args[k][i]), k)

    return {k: route(k) for k in fns}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    st = _stream(dev)
    res = {"library": _lib.loaded_library(), "shape": {"G": G, "h": H, "D": D, "w": W, "l": L_, "d": D_, "S": 1, "q_dtype": "bf16"}, "steps_per_batch": NB,
           "batches": NBATCH, "reps": REPS, "peak_bytes_per_s": PEAK, "cells": []}
    for ctx in (4096, 16384, 65536):
        for B in (16, 64, 256):
            for branch in ("sliding", "compressed"):
                t = ctx - 1
                if branch == "sliding":
                    # the last page alone: the ragged call sits at row 1023 of it, the paged one at ctx - 1 with every entry of sequence b -> page b
                    band, page, n_rows, rows_read, t_ragged = [0, 1, 0, W], 1024, 1024, W, 1023
                    max_pages = ctx // page
                    table = torch.arange(B, dtype=torch.int32, device=dev).view(B, 1).expand(B, max_pages).contiguous()
                else:
                    rows_read = (t + 1 - L_) // D_ + 1
                    band, page, t_ragged = [L_, D_, 1, 1 << 30], 64, t
                    n_rows = -(-rows_read // page) * page
                    max_pages = n_rows // page
                    table = torch.arange(B * max_pages, dtype=torch.int32, device=dev).view(B, max_pages)
                by = {"bf16": B * G * rows_read * 2 * D * 2, "fp8": B * G * rows_read * (2 * D + 8)}
                n_sets = min(32, -(-COLD_BYTES // by["fp8"]) + 1)
                sets = [make_set(B, n_rows, page, 7 + 1009 * i) for i in range(n_sets)]
                keep = []
                r = measure(routes_of(B, band, t_ragged, t, n_rows, page, max_pages, table, sets, st, keep), n_sets)
                cell = {"ctx": ctx, "B": B, "branch": branch, "rows": rows_read, "cache_sets": n_sets, "bytes_bf16": by["bf16"], "bytes_fp8": by["fp8"]}
                for k, (us, spread) in r.items():
                    cell[k] = {"us": us, "spread_us": spread, "hbm_fraction": by["fp8" if k.endswith("fp8") else "bf16"] / (us * 1e-6) / PEAK}
                print(json.dumps(cell), flush=True)
                res["cells"].append(cell)
                del keep, sets
                torch.cuda.empty_cache()
    lines = ["| context | B | branch | sets | MiB bf16 / fp8 | ragged bf16 us (HBM) | ragged fp8 us (HBM) | paged bf16 us (HBM) | paged fp8 us (HBM) | spread us | fp8 faster | fp8 slower |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in res["cells"]:
        f = lambda k: f"{c[k]['us']:.1f} ({c[k]['hbm_fraction']:.2f})"  # noqa: E731
        spread = max(c[k]["spread_us"] for k in ("ragged_bf16", "ragged_fp8", "paged_bf16", "paged_fp8"))
        won = [m for m in ("ragged", "paged") if c[m + "_bf16"]["us"] - c[m + "_fp8"]["us"] > spread]
        lost = [m for m in ("ragged", "paged") if c[m + "_fp8"]["us"] - c[m + "_bf16"]["us"] > spread]
        lines.append(f"| {c['ctx']} | {c['B']} | {c['branch']} | {c['cache_sets']} | {c['bytes_bf16'] / 2 ** 20:.1f} / {c['bytes_fp8'] / 2 ** 20:.1f} | "
                     f"{f('ragged_bf16')} | {f('ragged_fp8')} | {f('paged_bf16')} | {f('paged_fp8')} | {spread:.1f} | {' + '.join(won) or 'no'} | {' + '.join(lost) or 'no'} |")
    print("\n" + "\n".join(lines))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.splitext(out_path)[0] + ".txt", "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
