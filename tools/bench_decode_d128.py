"""Decode step of the selected branch at head dimension 128: device-event medians after warm-up, cache sets rotated so that
the figures at B >= 64 are cold, B in {1, 64, 256} x contexts {4k, 16k, 64k} at h = 6, G = 2, bf16, then the layer decode step at 16k / 64k
with B = 1.  Prints one JSON line per shape (time, algorithmic bytes, fraction of the 8 TB/s peak, the plan) and writes them to OUT.json.

    python tools/bench_decode_d128.py new profiles/decode_d128/new.json
    NSA_HIP_LIB=ab/parent.so python tools/bench_decode_d128.py parent profiles/decode_d128/parent.json   # make BUILD=... OUT=... of the parent
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsa_vibe_amd import _lib
import ctypes

try:  # a library built from an older commit (NSA_HIP_LIB) does not export the plan query: probe for it
    getattr(ctypes.CDLL(os.environ.get("NSA_HIP_LIB") or _lib.LIB_PATH), "nsa_sel_decode_step_plan")
    HAS_PLAN = True
except (AttributeError, OSError):
    HAS_PLAN = False
    _lib.SIGNATURES.pop("nsa_sel_decode_step_plan", None)
import nsa_vibe_amd as nv

tag, out = sys.argv[1], sys.argv[2]
G, h, D, n = 2, 6, 128, 16
dt = torch.bfloat16
res = {"tag": tag, "library": _lib.loaded_library(), "rows": []}
g = torch.Generator(device="cuda"); g.manual_seed(1)
for S in (4096, 16384, 65536):
    meta = nv.build_block_meta(S, 32, 16, 64, n, 512)
    for B in (1, 64, 256):
        touched = B * G * (meta.S_cmp * D * 2 + 2 * n * 64 * D * 2)
        per_set = B * G * (2 * S + meta.S_cmp) * D * 2
        nsets = 1 if B == 1 else max(2, min(8, -(-(600 << 20) // touched), (40 << 30) // per_set))
        sets = []
        for _ in range(nsets):
            mk = lambda *sh: torch.randn(*sh, device="cuda", generator=g, dtype=dt)
            sets.append((mk(B, 1, G, h, D), mk(B, G, meta.S_cmp, D), mk(B, G, S, D), mk(B, G, S, D)))
        O = torch.empty(B, 1, G, h, D, device="cuda", dtype=dt); rg = torch.empty(B, G, n, 2, device="cuda", dtype=torch.int32)
        t = S - 1
        plan = None
        if HAS_PLAN:
            plan = nv.selection_decode_step_plan(B, G, h, D, D, meta.S_cmp, meta.S_sel, S, n)
        def step(i):
            Q, Kc, K, V = sets[i % nsets]
            nv.selection_decode_step(Q, Kc, K, V, meta, n, t, out=O, ranges_out=rg)
        for i in range(12): step(i)
        torch.cuda.synchronize()
        reps = []
        for rep in range(3):
            ts = []
            for i in range(40):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); step(i); b.record(); b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            reps.append(statistics.median(ts))
        algo = touched + B * G * h * D * 2 * 2
        row = {"S": S, "B": B, "nsets": nsets, "us_median": statistics.median(reps), "us_reps": reps, "algo_bytes": algo,
               "frac_of_8TBs": algo / (statistics.median(reps) * 1e-6) / 8e12, "plan": plan}
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        del sets
        torch.cuda.empty_cache()
# layer decode step, B = 1
from nsa_vibe_amd.nsa_attention import NSAAttention
torch.manual_seed(0)
m = NSAAttention(1536, 12, 2, 128, 128).cuda().to(dt).eval()
for S in (16384, 65536):
    x = torch.randn(1, S + 64, 1536, device="cuda", dtype=dt)
    with torch.no_grad():
        kv = m.new_kv(1, S + 64, "cuda", dt)
        _, kv = m(x[:, :S], kv, prefill=True)
        ts = []
        for i in range(60):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); y, kv = m(x[:, S + i: S + i + 1], kv, prefill=False); b.record(); b.synchronize()
            if i >= 20: ts.append(a.elapsed_time(b) * 1e3)
    row = {"layer_decode_S": S, "B": 1, "us_median": statistics.median(ts), "us_min": min(ts)}
    print(json.dumps(row), flush=True)
    res["rows"].append(row)
    del kv, x
    torch.cuda.empty_cache()
json.dump(res, open(out, "w"), indent=1)
