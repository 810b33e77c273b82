#!/usr/bin/env python3
"""The decode step of the whole layer for S consecutive tokens (nsa_layer_decode_rows): three routes timed IN THE SAME RUN,
alternating call by call, on the m7c layer (dim 768, 12 heads, G = 2, D = 64, bf16), S in {1, 2, 4, 8, 16} x contexts {4k, 16k, 32k} x B in {1, 16}:

  (a) one nsa_layer_decode_rows call,
  (b) S calls of nsa_layer_decode_step at t0 .. t0 + S - 1 (the yardstick: these kernels are the parent commit's),
  (c) the extend route: F.linear(x, W_qkv) + nsa_layer_extend + F.linear(O_mix, W_out) (what forward(prefill=True) runs on a filled cache).

(a) and (b) go through the C ABI with prepared arguments; (c) adds its two torch GEMMs, as the module does.  All three write the same rows
t0 .. t0 + S - 1 of the same caches (random contents of ctx - S tokens), which stay warm at these sizes.  Device-event medians of ITERS calls
after warm-up; every cell is measured REPS times and the spread (max - min of the repeated medians, per route) is printed beside the median
of medians: a difference below the spread is no difference.  Not measured: cold caches, D = 128, B > 16.

    timeout 600 python tools/bench_layer_decode_rows.py [OUT.json] [context ...]
"""
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nsa_vibe_amd as nv  # noqa: E402
from nsa_vibe_amd import _lib  # noqa: E402
from nsa_vibe_amd.selection_scorer import _stream  # noqa: E402

DIM, HEADS, G, D, N = 768, 12, 2, 64, 16
L_, D_, LS, W = 32, 16, 64, 512
WARM, ITERS, REPS = 10, 30, 3
dt = torch.bfloat16
dev = torch.device("cuda")
L = _lib.lib()


def aligned(nbytes):
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return buf, (buf.data_ptr() + 255) & ~255


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    contexts = [int(a) for a in sys.argv[2:]] or [4096, 16384, 32768]
    torch.manual_seed(1)
    m = nv.NSAAttention(DIM, HEADS, G, D, D, l=L_, d=D_, l_sel=LS, n_sel=N, w=W, selector="sequential").cuda().to(dt).eval()
    desc, W_qkv = m._layer_desc()
    W_out = m.out.weight.detach()
    dref = ctypes.byref(desc)
    st = _stream(dev)
    res = {"library": _lib.loaded_library(), "shape": {"dim": DIM, "heads": HEADS, "G": G, "D": D, "n_sel": N, "dtype": "bf16"}, "iters": ITERS,
           "reps": REPS, "cells": []}
    for ctx in contexts:
        meta = nv.build_block_meta(ctx, L_, D_, LS, N, W)
        csc = [c.data_ptr() for c in meta.device_csc(dev)]
        S_sel = int(meta.S_sel)
        for B in (1, 16):
            kv = m.new_kv(B, ctx, dev, dt)
            for name in ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp"):
                getattr(kv, name).normal_()
            kd = kv.native_desc()
            kref = ctypes.byref(kd)
            for S in (1, 2, 4, 8, 16):  # (S = 1: the cell behind the default rule's one decline)
                t0 = ctx - S
                x = torch.randn(B, S, DIM, device=dev, dtype=dt)
                xs = [x[:, s].contiguous() for s in range(S)]
                y = torch.empty(B, S, DIM, device=dev, dtype=dt)
                ys = [torch.empty(B, DIM, device=dev, dtype=dt) for _ in range(S)]
                rg = torch.empty(B, S, G, N, 2, device=dev, dtype=torch.int32)
                gt = torch.empty(B, S, G, 3, device=dev, dtype=torch.float32)
                O = torch.empty(B, S, HEADS * D, device=dev, dtype=dt)
                wa, pa = aligned(L.nsa_layer_decode_rows_workspace(dref, B, S, kd.S_max))
                wb, pb = aligned(L.nsa_layer_decode_step_workspace(dref, B, kd.S_max))
                wc, pc = aligned(L.nsa_layer_extend_workspace(dref, B, S, t0, S_sel))
                rows_args = [dref, kref, x.data_ptr(), y.data_ptr(), t0, S, *csc, S_sel, rg.data_ptr(), gt.data_ptr(), pa, wa.numel() - 256, st]
                steps = [[dref, kref, xs[s].data_ptr(), ys[s].data_ptr(), t0 + s, *csc, S_sel, rg.data_ptr(), gt.data_ptr(), pb, wb.numel() - 256, st]
                         for s in range(S)]

                def route_a():
                    _lib.check(L.nsa_layer_decode_rows(*rows_args), "rows")

                def route_b():
                    for a in steps:
                        _lib.check(L.nsa_layer_decode_step(*a), "step")

                def route_c():
                    proj = F.linear(x, W_qkv)
                    _lib.check(L.nsa_layer_extend(dref, kref, proj.data_ptr(), t0, S, *csc, S_sel, rg.data_ptr(), O.data_ptr(), gt.data_ptr(), pc,
                                                  wc.numel() - 256, st), "extend")
                    F.linear(O, W_out)

                _lib.set_tuning("LAYER_DECODE_ROWS", 1)
                plan = m.decode_rows_plan(B, S, kd.S_max, t0, S_sel)
                _lib.set_tuning("LAYER_DECODE_ROWS", -1)
                routes = {"a": route_a, "b": route_b, "c": route_c}
                with torch.no_grad():
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
                cell = {"ctx": ctx, "B": B, "S": S, "launches": plan["launches"], "route": plan["route"]}
                for k in routes:
                    cell[f"{k}_us"] = statistics.median(med[k])
                    cell[f"{k}_spread_us"] = max(med[k]) - min(med[k])
                spread = max(cell["a_spread_us"], cell["b_spread_us"], cell["c_spread_us"])
                cell["a_not_slower_than_b"] = bool(cell["a_us"] <= cell["b_us"] + spread)
                cell["a_beats_both"] = bool(cell["a_us"] + spread < min(cell["b_us"], cell["c_us"]))
                print(json.dumps(cell), flush=True)
                res["cells"].append(cell)
            del kv, kd
    print("\n| context | B | S | launches | (a) one call us | (b) S single steps us | (c) extend route us | spread us | (a) beats both |")
    print("|---|---|---|---|---|---|---|---|---|")
    for c in res["cells"]:
        sp = max(c["a_spread_us"], c["b_spread_us"], c["c_spread_us"])
        print(f"| {c['ctx']} | {c['B']} | {c['S']} | {c['launches']} | {c['a_us']:.1f} | {c['b_us']:.1f} | {c['c_us']:.1f} | {sp:.1f} | "
              f"{'yes' if c['a_beats_both'] else 'no'} |")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
