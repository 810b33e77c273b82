#!/usr/bin/env python3
"""The layer's ragged decode call (nsa_layer_decode_ragged) against what a caller runs without it, timed IN THE SAME RUN,
alternating, on the m7c layer (dim 768, 12 heads, G = 2, D = 64, bf16), B in {16, 64} x S in {1, 4}:

  (a) equal positions at contexts {4k, 16k}: one ragged call against one nsa_layer_decode_rows call at the same t0 -- the price of the
      position array and of the pooling launch that is always made;
  (b) positions drawn uniformly from [1k, 16k]: one ragged call against the only route without it, one B = 1 layer call per sequence on
      that sequence's slab (nsa_layer_decode_step for S = 1, nsa_layer_decode_rows for S = 4).  With `--parent LIB` (or NSA_HIP_LIB_PARENT)
      that route is ALSO timed on another build of the library -- the parent commit's -- loaded beside the product with ctypes.CDLL.
      (Not through NSA_HIP_LIB: _lib.lib() checks every declared symbol and the parent's library lacks nsa_layer_decode_ragged*.)

Everything goes through the C ABI with prepared arguments.  COLD, as tools/bench_sel_decode_ragged.py: the steps rotate over independent
pools, so many that the others load >= 512 MiB between two uses of one pool (at most 32).  Device events around batches of NB steps; every
cell is measured REPS times and the spread (max - min of the repeated medians) is printed beside the median of medians: a difference below
the spread is no difference.  Not measured: D = 128, warm caches, B > 64.

    python tools/bench_layer_decode_ragged.py [--parent LIB] [OUT.json]     (default OUT: profiles/layer_decode_ragged/bench.json)
"""
import ctypes
import hashlib
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


def load_parent(path):
    """another build of the library beside the product: the three entry points the per-sequence route calls, with the product's signatures"""
    P = ctypes.CDLL(path)
    for name in ("nsa_layer_decode_step", "nsa_layer_decode_rows", "nsa_hip_last_error"):
        fn = getattr(P, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    with open(path, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()[:16]
    return P, {"path": os.path.relpath(os.path.abspath(path), ROOT), "sha16": sha}


def aligned(nbytes):
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return buf, (buf.data_ptr() + 255) & ~255


def n_sets_for(B, ctx):
    step = B * G * ((min(N * LS, ctx) + min(W, ctx)) * 2 * D * 2 + ncmp(ctx) * 2 * D * 2)
    return min(32, -(-COLD_BYTES // step) + 1)


def make_pools(m, B, cap, n_sets):
    pools = []
    for _ in range(n_sets):
        kv = m.new_kv(B, cap, dev, dt)
        for name in CACHES:
            getattr(kv, name).normal_()
        pools.append(kv)
    return pools


def slab_desc(kv, b):
    """nsa_kv_desc of slab b alone (B = 1)"""
    d = _lib.NsaKvDesc()
    for f, name in zip(("K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw", "K_cmp", "V_cmp"), CACHES):
        setattr(d, f, getattr(kv, name)[b].data_ptr())
    d.B, d.S_max, d.n_cmp_max = 1, kv._K_sel.shape[2], kv._K_cmp.shape[2]
    return d


def measure(routes, n_sets):
    """routes: {name: f(pool index)} -> {name: (median of medians us per step, spread us)}"""
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


def cell_routes(m, B, S, positions, pools, parent, keep):
    """the ragged call on every pool; the rows call (equal positions) or one B = 1 call per sequence (mixed), on the product and on `parent`"""
    desc, _ = m._layer_desc()
    dref, st = ctypes.byref(desc), _stream(dev)
    cap = pools[0]._K_sel.shape[2]
    t_max = max(positions) + S - 1
    meta = nv.build_block_meta(t_max + 1, L_, D_, LS, N, W)
    csc = [c.data_ptr() for c in meta.device_csc(dev)]
    x = torch.randn(B, S, DIM, device=dev, dtype=dt)
    y = torch.empty(B, S, DIM, device=dev, dtype=dt)
    rg = torch.empty(B, S, G, N, 2, device=dev, dtype=torch.int32)
    gt = torch.empty(B, S, G, 3, device=dev, dtype=torch.float32)
    pos_dev = torch.tensor(positions, dtype=torch.int32, device=dev)
    wr, pr = aligned(L.nsa_layer_decode_ragged_workspace(dref, B, S, cap))
    keep += [meta, x, y, rg, gt, pos_dev, wr]
    descs = [p.native_desc() for p in pools]
    ragged_args = [[dref, ctypes.byref(kd), x.data_ptr(), y.data_ptr(), pos_dev.data_ptr(), t_max, S, *csc, int(meta.S_sel), rg.data_ptr(), gt.data_ptr(), pr,
                    wr.numel() - 256, st] for kd in descs]
    keep.append(descs)

    def ragged(i):
        _lib.check(L.nsa_layer_decode_ragged(*ragged_args[i]), "ragged")

    routes = {"ragged": ragged}
    plan = m.decode_ragged_plan(B, S, cap, t_max, int(meta.S_sel))
    if len(set(positions)) == 1:
        t0 = positions[0]
        wa, pa = aligned(L.nsa_layer_decode_rows_workspace(dref, B, S, cap))
        keep.append(wa)
        rows_args = [[dref, ctypes.byref(kd), x.data_ptr(), y.data_ptr(), t0, S, *csc, int(meta.S_sel), rg.data_ptr(), gt.data_ptr(), pa, wa.numel() - 256, st]
                     for kd in descs]

        def rows(i):
            _lib.check(L.nsa_layer_decode_rows(*rows_args[i]), "rows")

        routes["rows"] = rows
        return routes, plan
    # one B = 1 call per sequence on its slab, with that sequence's own block metadata
    w1, p1 = aligned(max(L.nsa_layer_decode_step_workspace(dref, 1, cap), L.nsa_layer_decode_rows_workspace(dref, 1, S, cap)))
    keep.append(w1)
    per = []
    for kv in pools:
        calls = []
        for b, t in enumerate(positions):
            mb = nv.build_block_meta(t + S, L_, D_, LS, N, W)
            cb = [c.data_ptr() for c in mb.device_csc(dev)]
            kd = slab_desc(kv, b)
            keep += [mb, kd]
            head = [dref, ctypes.byref(kd), x[b].data_ptr(), y[b].data_ptr(), t] + ([S] if S > 1 else [])
            calls.append(head + [*cb, int(mb.S_sel), rg[b].data_ptr(), gt[b].data_ptr(), p1, w1.numel() - 256, st])
        per.append(calls)
    name = "nsa_layer_decode_rows" if S > 1 else "nsa_layer_decode_step"

    def per_sequence_on(lib):
        fn = getattr(lib, name)

        def run(i):
            for a in per[i]:
                if fn(*a) != 0:
                    raise RuntimeError(f"{name}: {(lib.nsa_hip_last_error() or b'').decode()}")
        return run

    routes["per_sequence"] = per_sequence_on(L)
    if parent is not None:
        routes["per_sequence_parent"] = per_sequence_on(parent)
        try:  # a status return of the other build is reported and its route left out; the product's routes are measured all the same
            routes["per_sequence_parent"](0)
            torch.cuda.synchronize()
        except RuntimeError as e:
            print(json.dumps({"parent_route_left_out": str(e)}), flush=True)
            del routes["per_sequence_parent"]
    return routes, plan


def main():
    args = sys.argv[1:]
    parent_path = os.environ.get("NSA_HIP_LIB_PARENT")
    if "--parent" in args:
        i = args.index("--parent")
        parent_path = args[i + 1]
        del args[i:i + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "layer_decode_ragged", "bench.json")
    parent, parent_info = load_parent(parent_path) if parent_path else (None, None)
    torch.manual_seed(1)
    m = nv.NSAAttention(DIM, HEADS, G, D, D, l=L_, d=D_, l_sel=LS, n_sel=N, w=W, selector="sequential").cuda().to(dt).eval()
    res = {"library": _lib.loaded_library(), "parent_library": parent_info, "shape": {"dim": DIM, "heads": HEADS, "G": G, "D": D, "n_sel": N, "dtype": "bf16"},
           "steps_per_batch": NB, "batches": NBATCH, "reps": REPS, "equal": [], "mixed": []}
    print(json.dumps({"library": res["library"], "parent_library": parent_info}), flush=True)
    with torch.no_grad():
        for ctx in (4096, 16384):
            for B in (16, 64):
                n_sets = n_sets_for(B, ctx)
                pools = make_pools(m, B, ctx, n_sets)
                for S in (1, 4):
                    keep = []
                    routes, plan = cell_routes(m, B, S, [ctx - S] * B, pools, None, keep)
                    r = measure(routes, n_sets)
                    cell = {"ctx": ctx, "B": B, "S": S, "pools": n_sets, "launches": plan["launches"], "ragged_us": r["ragged"][0],
                            "ragged_spread_us": r["ragged"][1], "rows_us": r["rows"][0], "rows_spread_us": r["rows"][1]}
                    print(json.dumps(cell), flush=True)
                    res["equal"].append(cell)
                    del routes, keep
                del pools
                torch.cuda.empty_cache()
        for B in (16, 64):
            gen = torch.Generator()
            gen.manual_seed(100 + B)
            positions = sorted(int(v) for v in torch.randint(1024, 16385, (B,), generator=gen))
            n_sets = n_sets_for(B, sum(positions) // B)
            pools = make_pools(m, B, positions[-1] + 16, n_sets)
            for S in (1, 4):
                keep = []
                routes, plan = cell_routes(m, B, S, positions, pools, parent, keep)
                r = measure(routes, n_sets)
                cell = {"B": B, "S": S, "positions_min": positions[0], "positions_max": positions[-1], "pools": n_sets, "launches": plan["launches"],
                        "per_sequence_call": "nsa_layer_decode_rows" if S > 1 else "nsa_layer_decode_step"}
                for k, (us, sp) in r.items():
                    cell[k + "_us"], cell[k + "_spread_us"] = us, sp
                print(json.dumps(cell), flush=True)
                res["mixed"].append(cell)
                del routes, keep
            del pools
            torch.cuda.empty_cache()
    lines = ["(a) equal positions", "| context | B | S | pools | ragged us | rows call us | spread us |", "|---|---|---|---|---|---|---|"]
    for c in res["equal"]:
        lines.append(f"| {c['ctx']} | {c['B']} | {c['S']} | {c['pools']} | {c['ragged_us']:.1f} | {c['rows_us']:.1f} | {max(c['ragged_spread_us'], c['rows_spread_us']):.1f} |")
    lines += ["", "(b) positions drawn from [1k, 16k]", "| B | S | pools | one ragged call us | one B = 1 call per sequence us | the same on the parent library us | spread us |",
              "|---|---|---|---|---|---|---|"]
    for c in res["mixed"]:
        par = f"{c['per_sequence_parent_us']:.1f}" if "per_sequence_parent_us" in c else "not measured"
        sp = max(v for k, v in c.items() if k.endswith("_spread_us"))
        lines.append(f"| {c['B']} | {c['S']} | {c['pools']} | {c['ragged_us']:.1f} | {c['per_sequence_us']:.1f} | {par} | {sp:.1f} |")
    table = "\n".join(lines)
    print("\n" + table)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(out_path)[0] + ".txt", "w") as f:
        f.write(f"library {res['library']}\nparent library {parent_info}\n\n{table}\n")


if __name__ == "__main__":
    main()
