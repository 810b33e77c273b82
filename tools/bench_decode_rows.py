#!/usr/bin/env python3
"""The decode rows of `bench.py --full` alone -- extra.layer_S*_B* (decode_us_per_step) and extra.model_m7c_125m_S*_B* (decode_ms_per_token)
by bench.py's own layer_bench / model_bench -- as one JSON line: what an A/B of the few-row projection kernels needs without the minutes
of prefill, training and CPU-baseline extras around it.  python3 tools/bench_decode_rows.py"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
import nsa_vibe_amd as nv

dev = torch.device("cuda")
out = {}
for S, B in ((4096, 8), (16384, 1), (65536, 1)):
    out[f"layer_S{S}_B{B}"] = bench.layer_bench(nv, B, S, dev)
for S, B in ((4096, 1), (16384, 1), (4096, 32)):
    out[f"model_m7c_125m_S{S}_B{B}"] = bench.model_bench(B, S, dev)
# one fp32 layer: its projections take the chunk-loop kernels (the bf16 rows above take the all-loads-first and MFMA forms)
for S, B in ((4096, 1), (4096, 2)):
    torch.manual_seed(0)
    m = nv.NSAAttention(768, 12, bench.G, bench.D, bench.D, bench.L_CMP, bench.D_CMP, bench.L_SEL, bench.N_SEL, 512, selector="batched").to(dev).eval()
    with torch.no_grad():
        kv = m.new_kv(B, S + 64, dev, torch.float32)
        _, kv = m(torch.randn(B, S, 768, device=dev), kv, prefill=True)
        xt = torch.randn(B, 1, 768, device=dev)
        for _ in range(8):
            _, kv = m(xt, kv, prefill=False)
        dt = 1e9
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                _, kv = m(xt, kv, prefill=False)
            torch.cuda.synchronize()
            dt = min(dt, (time.perf_counter() - t0) / 10)
    out[f"layer_fp32_S{S}_B{B}"] = {"decode_us_per_step": dt * 1e6}
print(json.dumps(out))
