#!/usr/bin/env python3
"""The one-row selection forward kernel (SEL_ROWS 0) under LDS-DMA and register staging, and its split-KV form on the last 64 rows, bf16 m7c,
timed the way tools/bench_blocks.py times the other forms (interleaved rounds in one process):
    python tools/bench_one_row.py"""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import nsa_vibe_amd as nv  # noqa: E402
dev = torch.device("cuda", 0)
for S, B in [(4096, 8), (16384, 2)]:
    meta, Q, Kc, K, V = bench.make_inputs(nv, B, S, dev, 1234)
    p = nv.selection_scores(Q, Kc, meta, 0.125, causal_skip=True, leave_skipped=True)
    rg = nv.select_topn_ranges_batched(p, meta, bench.N_SEL, S)
    res = {"stage1": [], "stage0": [], "split": []}
    for rnd in range(4):
        for name, stage in (("stage1", 1), ("stage0", 0)):
            nv._lib.set_tuning("SEL_ROWS", 0)
            nv._lib.set_tuning("ATTN_STAGE", stage)
            res[name].append(bench.time_events(lambda: nv.selection_attention_hip(Q, K, V, rg, variant=2), 5, warm=1))
        nv._lib.set_tuning("ATTN_STAGE", 1)
        Qs, rs = Q[:, -64:].contiguous(), rg[:, -64:].contiguous()  # R = B 64 G rows: the split-KV form
        res["split"].append(bench.time_events(lambda: nv.selection_attention_hip(Qs, K, V, rs, variant=2, return_lse=True), 5, warm=1))
    nv._lib.set_tuning("SEL_ROWS", -1)
    print(f"one_row S={S} B={B}: " + "  ".join(f"{k} {np.median(v) * 1e3:8.1f} us (min {min(v) * 1e3:.1f})" for k, v in res.items()), flush=True)
    del Q, Kc, K, V, p, rg
    torch.cuda.empty_cache()
