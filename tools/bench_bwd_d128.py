#!/usr/bin/env python3
"""Timing of the attention backward at head dimension 128 (bf16), device events after warm-up.

  selection: forward + backward at S = 4096, B = 8, G = 2, h = 6, n = 16 blocks of 64 for D = 128 MFMA (bwd_variant=2), D = 128 generic
             (bwd_variant=1) and D = 64 MFMA; one 64k-key shape (B = 1, S = 65536) at D = 128 MFMA
  band:      backward of the sliding (w = 512) and the compressed (l = 32, d = 16) branch at the same shape, D = 128, MFMA vs generic
  layer:     one training step (forward + backward) of NSAAttention(1536, 12, 2, 128, 128, l=32, d=16, l_sel=64, n_sel=16, w=512,
             selector="batched"), bf16, S = 4096, B = 8

Usage: bench_bwd_d128.py [all|layer]   (`layer` times only the training step: run it against two libraries through NSA_HIP_LIB,
tools/ab_libs.sh)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nsa_vibe_amd as nv  # noqa: E402
from nsa_vibe_amd import _lib  # noqa: E402
from nsa_vibe_amd.band_attention import band_attention_hip  # noqa: E402

WHAT = sys.argv[1] if len(sys.argv) > 1 else "all"
B, S, G, h, n = 8, 4096, 2, 6, 16


def timed(fn, iters, warm=2):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf = tb = 0.0
    for i in range(warm + iters):
        ev[0].record()
        out, back = fn()
        ev[1].record()
        back(out)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= warm:
            tf += ev[0].elapsed_time(ev[1])
            tb += ev[1].elapsed_time(ev[2])
    return tf / iters, tb / iters


def sel_case(B_, S_, D, bwd_variant, iters):
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    meta = nv.build_block_meta(S_, 32, 16, 64, n, 512)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()  # noqa: E731
    Q, K, V, dO = mk(B_, S_, G, h, D), mk(B_, G, S_, D), mk(B_, G, S_, D), mk(B_, S_, G, h, D)
    rg = nv.select_topn_ranges_batched(torch.rand(B_, S_, G, meta.S_sel, device="cuda", generator=g), meta, n, S_)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))

    def fn():
        q.grad = k.grad = v.grad = None
        return nv.selection_attention_hip(q, k, v, rg, bwd_variant=bwd_variant), lambda O: O.backward(dO)

    return timed(fn, iters)


def band_case(band, D, bwd_variant, iters):
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    S_kv = S if "w" in band else (S - band["a"]) // band["dd"] + 1
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()  # noqa: E731
    Q, K, V, dO = mk(B, S, G, h, D), mk(B, G, S_kv, D), mk(B, G, S_kv, D), mk(B, S, G, h, D)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))

    def fn():
        q.grad = k.grad = v.grad = None
        return band_attention_hip(q, k, v, bwd_variant=bwd_variant, **band), lambda O: O.backward(dO)

    return timed(fn, iters)


def layer_step(iters):
    from nsa_vibe_amd.nsa_attention import NSAAttention

    torch.manual_seed(0)
    m = NSAAttention(1536, 12, 2, 128, 128, l=32, d=16, l_sel=64, n_sel=16, w=512, selector="batched").cuda().bfloat16().train()
    x = torch.randn(B, S, 1536, device="cuda").bfloat16().requires_grad_(True)
    gout = torch.randn(B, S, 1536, device="cuda").bfloat16()

    def fn():
        m.zero_grad(set_to_none=True)
        x.grad = None
        out, _ = m(x, m.new_kv(B, S, "cuda", torch.bfloat16), prefill=True)
        return out, lambda o: o.backward(gout)

    return timed(fn, iters)


print(f"library: {_lib.loaded_library()}")
if WHAT == "all":
    print(f"selection attention, bf16, B={B} S={S} G={G} h={h} n={n}x64 (ms, fwd / bwd)")
    for label, args, iters in (("D=128 MFMA   ", (B, S, 128, 2), 10), ("D=128 generic", (B, S, 128, 1), 2), ("D=64  MFMA   ", (B, S, 64, 2), 10),
                               ("D=128 MFMA 64k keys (B=1 S=65536)", (1, 65536, 128, 2), 5)):
        f, b = sel_case(*args, iters)
        print(f"  {label}: fwd {f:.3f}  bwd {b:.3f}")
    print(f"band attention backward, bf16, D=128, B={B} S={S} G={G} h={h} (ms, fwd / bwd)")
    for name, band in (("sliding w=512", dict(w=512)), ("compressed l=32 d=16", dict(a=32, dd=16, c=1))):
        for bv, label in ((2, "MFMA"), (1, "generic")):
            f, b = band_case(band, 128, bv, 10 if bv == 2 else 2)
            print(f"  {name} {label}: fwd {f:.3f}  bwd {b:.3f}")
f, b = layer_step(5)
print(f"layer training step D=128 (NSAAttention(1536,12,2,128,128), bf16, B={B} S={S}): fwd {f:.3f} ms  bwd {b:.3f} ms  step {f + b:.3f} ms")
