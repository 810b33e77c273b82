#!/usr/bin/env python3
"""Golden vectors for RoPE and the compressed-token pooling (g22), from the IMPORTED reference.

    python oracle/make_rope_pool_goldens.py

The parity targets are nsa/core/rope.py:6-51 (build_inv_freq, apply_rope: fp32 angles (pos / scale) inv_freq, sin / cos cast to the
activation dtype, the products in that dtype) and nsa/core/compress_pool.py:9-38 (avg_pool_phi_rope_kv with pos given: apply_rope WITHOUT
the position scale, then avg_pool2d over windows of l rows with stride d; no tokens when S < l).  Every case runs in fp32, bf16 and fp16 on
the CPU; the reference's own rounding in each dtype is what is pinned.

Inputs come from tests/golden_inputs.py (g22_inputs: PCG64, multiples of 1/32 below 8, exact in bf16 and fp16); the fixture holds, per case
and dtype, only outputs (fp32 as float32, bf16 as its uint16 bit pattern, fp16 as float16):
  inv_freq_<D>                   build_inv_freq(D) for every width used;
  rope_<case>_<dt>_y             apply_rope(x, pos, scale=s);
  rope_<case>_<dt>_dx            (cases with gradient) the autograd gradient of x for the upstream dy;
  pool_<case>_<dt>_Kc / _Vc      the stored windows (golden_inputs.g22_pool_windows) of avg_pool_phi_rope_kv(K, V, l, d, pos);
  pool_<case>_<dt>_dK / _dV      (cases with gradient) the autograd gradients of K and V for the upstream dKc / dVc.
Asserts before saving: the oracle (oracle/nsa_oracle.c: rope, rope_bwd, cmp_pool, cmp_pool_bwd) is within its error bound
(nsa_oracle.rope_bound & co.) of every stored vector, and its inv_freq table within 1 ulp.  The file is written with fixed zip timestamps, so
a rerun reproduces it byte for byte.  Output: tests/golden/g22_rope_pool.npz.
"""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("NSA_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import torch  # noqa: E402

import golden_inputs as gi  # noqa: E402
from nsa.core.compress_pool import avg_pool_phi_rope_kv  # noqa: E402
from nsa.core.rope import apply_rope, build_inv_freq  # noqa: E402

from oracle import nsa_oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g22_rope_pool.npz")
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def pack(t, dt):
    """a CPU tensor of dtype dt -> the stored array (bf16 as the uint16 bit pattern)"""
    t = t.detach()
    if dt == "bf16":
        return t.contiguous().view(torch.int16).numpy().view(np.uint16)
    return t.numpy().astype(np.float16 if dt == "fp16" else np.float32)


def ratio(got, ref, bound):
    """max |got - ref| / bound (an element with bound 0 must match exactly)"""
    e = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    assert (e[bound == 0] == 0).all()
    return float((e / np.where(bound > 0, bound, 1.0)).max()) if e.size else 0.0


store, worst = {}, {}
for D in sorted({c[0] for c in gi.G22_ROPE_CASES.values()} | {c[2] for c in gi.G22_POOL_CASES.values()}):
    f = build_inv_freq(D).numpy()
    store[f"inv_freq_{D}"] = f
    du = np.abs(orc.rope_inv_freq(D).view(np.int32).astype(np.int64) - f.view(np.int32))
    assert du.max() <= 1, (D, du.max())
    print(f"inv_freq D={D}: {int((du > 0).sum())} of {D // 2} entries 1 ulp from the correctly rounded value")

for case, (D, scale, _, grad) in gi.G22_ROPE_CASES.items():
    x = gi.g22_inputs(case)
    pos = torch.from_numpy(x["pos"])
    for dt, tdt in TDT.items():
        xt = torch.from_numpy(x["x"]).to(tdt).requires_grad_(grad)
        y = apply_rope(xt, pos, scale=scale)
        pre = f"rope_{case}_{dt}_"
        store[pre + "y"] = pack(y, dt)
        r = ratio(y.detach().float().numpy(), orc.rope(x["x"], x["pos"], dt, scale), orc.rope_bound(x["x"], x["pos"], dt, scale))
        worst[("rope", dt)] = max(worst.get(("rope", dt), 0.0), r)
        assert r <= 1.0, (case, dt, r)
        if grad:
            y.backward(torch.from_numpy(x["dy"]).to(tdt))
            store[pre + "dx"] = pack(xt.grad, dt)
            r = ratio(xt.grad.float().numpy(), orc.rope_bwd(x["dy"], x["pos"], dt, scale), orc.rope_bound(x["dy"], x["pos"], dt, scale))
            worst[("rope_bwd", dt)] = max(worst.get(("rope_bwd", dt), 0.0), r)
            assert r <= 1.0, (case, dt, "bwd", r)

for case, (l, d, D, S, p0, _, grad) in gi.G22_POOL_CASES.items():
    x = gi.g22_inputs(case)
    win = gi.g22_pool_windows(case)
    pos = torch.from_numpy(x["pos"])
    for dt, tdt in TDT.items():
        K = torch.from_numpy(x["K"]).to(tdt).requires_grad_(grad)
        V = torch.from_numpy(x["V"]).to(tdt).requires_grad_(grad)
        Kc, Vc = avg_pool_phi_rope_kv(K, V, l, d, pos=pos)
        n = 0 if S < l else (S - l) // d + 1
        assert Kc.shape == (1, 1, n, D) and Vc.shape == (1, 1, n, D), (case, Kc.shape)
        pre = f"pool_{case}_{dt}_"
        store[pre + "Kc"], store[pre + "Vc"] = pack(Kc[:, :, win], dt), pack(Vc[:, :, win], dt)
        oK, oV = orc.cmp_pool(x["K"], x["V"], l, d, x["pos"], dt)
        bK, bV = orc.cmp_pool_bound(x["K"], x["V"], l, d, x["pos"], dt)
        r = max(ratio(Kc.detach().float().numpy(), oK, bK), ratio(Vc.detach().float().numpy(), oV, bV))
        worst[("pool", dt)] = max(worst.get(("pool", dt), 0.0), r)
        assert r <= 1.0, (case, dt, r)
        if grad:
            torch.autograd.backward([Kc, Vc], [torch.from_numpy(x["dKc"]).to(tdt), torch.from_numpy(x["dVc"]).to(tdt)])
            store[pre + "dK"], store[pre + "dV"] = pack(K.grad, dt), pack(V.grad, dt)
            oK, oV = orc.cmp_pool_bwd(x["dKc"], x["dVc"], S, l, d, x["pos"], dt)
            bK, bV = orc.cmp_pool_bwd_bound(x["dKc"], x["dVc"], S, l, d, x["pos"], dt)
            r = max(ratio(K.grad.float().numpy(), oK, bK), ratio(V.grad.float().numpy(), oV, bV))
            worst[("pool_bwd", dt)] = max(worst.get(("pool_bwd", dt), 0.0), r)
            assert r <= 1.0, (case, dt, "bwd", r)
            last = (n - 1) * d + l  # rows after the last window: exactly 0 in the reference too
            assert (K.grad[:, :, last:] == 0).all() and (V.grad[:, :, last:] == 0).all()

print("worst oracle / reference error, as a fraction of the bound: " + ", ".join(f"{k[0]} {k[1]} {v:.3f}" for k, v in sorted(worst.items())))

# a deflated .npz written with fixed zip timestamps, so a rerun reproduces the file bit for bit (np.savez stamps the current time)
with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_DEFLATED) as zf:
    for k in sorted(store):
        info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        with zf.open(info, "w", force_zip64=True) as f:
            np.lib.format.write_array(f, np.ascontiguousarray(store[k]), allow_pickle=False)
print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(store)} arrays")
