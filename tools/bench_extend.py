"""Extend route figures (device-event time after warm-up, bf16 m7c_125m layer: dim 768, 12 heads, G 2, d_k = d_v = 64, l 32, d 16, l' 64,
n 16, w 512).  python tools/bench_extend.py [--quick]
  table 1: extend of S tokens onto a context of T tokens (one nsa_layer_extend call + its two GEMMs) against S decode steps of the same layer
           (the decode figure is the mean of 32 measured steps at that context times S)
  table 2: scores + select and the whole layer of a decode-normalised prefill from an empty cache (prefill_tile = S) against today's prefill"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nsa_vibe_amd as nv  # noqa: E402
from nsa_vibe_amd.nsa_attention import NSAAttention  # noqa: E402
from nsa_vibe_amd.selection_scorer import selection_scores_select  # noqa: E402


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2] * 1e3  # median, us


def layer():
    torch.manual_seed(0)
    return NSAAttention(768, 12, 2, 64, 64, l=32, d=16, l_sel=64, n_sel=16, w=512, selector="sequential").cuda().bfloat16().eval()


def reset(kv, t, n_cmp, nreads):
    kv.t, kv.n_cmp = t, n_cmp
    for lst in (kv.reads_pred, kv.reads_act_total, kv.reads_act_sel, kv.reads_act_cmp, kv.reads_act_win):
        del lst[nreads:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default="", help="'extend' or 'prefill'")
    a = ap.parse_args()
    m = layer()
    ctxs = (4096, 16384) if a.quick else (4096, 16384, 65536)
    Ss = (1, 4, 64, 512, 4096)
    with torch.no_grad():
        if a.only in ("", "extend"):
            for B in (1, 16):
                for T in ctxs:
                    x = torch.randn(B, T + max(Ss), 768, device="cuda").bfloat16()
                    kv = m.new_kv(B, T + max(Ss), "cuda", torch.bfloat16)
                    m(x[:, :T], kv, prefill=True)
                    t0, n0, r0 = kv.t, kv.n_cmp, len(kv.reads_pred)
                    xd = [x[:, T + i: T + i + 1].contiguous() for i in range(32)]

                    def dec():
                        for i in range(32):
                            m(xd[i], kv, prefill=False)
                        reset(kv, t0, n0, r0)

                    step = timed(dec, reps=3, warm=1) / 32
                    for S in Ss:
                        xs = x[:, T: T + S].contiguous()

                        def ext():
                            m(xs, kv, prefill=True)
                            reset(kv, t0, n0, r0)

                        us = timed(ext)
                        print(json.dumps({"table": "extend", "B": B, "T": T, "S": S, "extend_us": round(us, 1), "decode_step_us": round(step, 1),
                                          "decode_S_steps_us": round(step * S, 1), "speedup": round(step * S / us, 2)}), flush=True)
                    del x, kv
                    torch.cuda.empty_cache()
        if a.only in ("", "prefill"):
            for S, B in ((4096, 8), (65536, 16)):
                meta = nv.build_block_meta(S, 32, 16, 64, 16, 512)
                Q = torch.randn(B, S, 2, 6, 64, device="cuda").bfloat16()
                Kc = torch.randn(B, 2, meta.S_cmp, 64, device="cuda").bfloat16()
                sc_all = timed(lambda: selection_scores_select(Q, Kc, meta, 16, mode="sequential", scale=0.125))
                sc_dec = timed(lambda: selection_scores_select(Q, Kc, meta, 16, mode="sequential", scale=0.125, normalize="causal"))
                del Q, Kc
                x = torch.randn(B, S, 768, device="cuda").bfloat16()
                kv = m.new_kv(B, S, "cuda", torch.bfloat16)

                def run(tile):
                    m.prefill_tile = tile
                    reset(kv, 0, 0, 0)
                    m(x, kv, prefill=True)

                lay_pre = timed(lambda: run(0), reps=3, warm=1)
                lay_ext = timed(lambda: run(S), reps=3, warm=1)
                m.prefill_tile = 0
                print(json.dumps({"table": "prefill", "S": S, "B": B, "scores_select_prefill_us": round(sc_all, 1),
                                  "scores_select_decode_norm_us": round(sc_dec, 1), "layer_prefill_us": round(lay_pre, 1),
                                  "layer_extend_tile_S_us": round(lay_ext, 1)}), flush=True)
                del x, kv
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
