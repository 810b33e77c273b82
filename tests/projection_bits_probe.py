"""The few-row projection kernels, the RoPE column map and their launch routes, bit for bit: runs a fixed table of cases on the native
library that NSA_HIP_LIB names (default: the product) and writes the raw bit patterns of every output to an .npz.

    python tests/projection_bits_probe.py OUT.npz          # run every case, write OUT.npz
    python tests/projection_bits_probe.py --list           # construct every case's inputs on the CPU and print the table (no device)

tests/golden/projection_bits.npz was recorded ONCE with this script from the library of the commit before the projection kernels were
folded onto two templates; tests/test_hip_projection_bits.py requires the product to reproduce it exactly (no atomics, fixed summation
order: there is no tolerance).  Inputs come from numpy PCG64 streams rounded to bf16-representable values on the host (the
tests/golden_inputs.py recipe); the device RNG is not used.

Stored form: uint16 (bf16 / fp16) or uint32 (fp32) bit patterns, one key per output.  An output of more than BIG elements is stored
as its first and last BIG / 2 elements plus `<key>.sha`, the SHA-256 of all of its bytes as 8 uint32 words, so that equality of the stored
arrays is still equality of every bit while the file stays under 300 KB.  (Shrinking N does not
help: the large outputs are those of the 4-row forms, which the route takes from N = 4096 on, and the B = 70 module case, whose batch is
what reaches the second row tile; stored raw the B = 70 case alone is 570 KB.)

Geometries: every case of the issue's table is taken as listed, except the module that reaches NC = 4 of the three-branch-mix form: that
form's K is n_heads * d_v, so the dim = 1032 module has 24 heads of 64 (K = 1536) where the rest of the table has 4; and the backward case
"dK_win and dV_cmp null": the entry point takes six gradients and has no V_cmp among them, so the null pair is dK_win and dV_raw, the
gradient of the raw values that V_cmp is pooled from."""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from golden_inputs import _bf16_round, _rng, randn  # noqa: E402

BIG = 1024
DTS = ("bf16", "fp16", "fp32")

# nsa_linear_small (M, N, K, epi): the all-loads-first forms when A is aligned ...
LINEAR_FAST = [(1, 40, 8, 2), (2, 37, 520, 1), (1, 36, 1032, 0), (2, 36, 3072, 2), (1, 36, 4096, 0), (2, 4100, 1000, 1), (1, 4097, 8, 0)]
# ... and the chunk loops when A starts 2 bytes off a 16-byte boundary (16-bit) or is fp32
LINEAR_LOOP = LINEAR_FAST + [(5, 37, 520, 1), (9, 36, 1032, 2), (2, 4100, 1000, 0), (1, 36, 4104, 0)]
# TinyLM(vocab, dim, layers, heads, groups, d_k, d_v, l, d, l_sel, n_sel, w), dtype, B
MODEL = [((131, 128, 3, 4, 2, 64, 64, 32, 16, 64, 4, 64), dt, B) for dt in ("bf16", "fp32") for B in (1, 2)] + \
        [((131, 1032, 1, 24, 2, 64, 64, 32, 16, 64, 4, 64), "bf16", 1)]
MODEL_PREFILL, MODEL_STEPS = 40, 6
# NSAAttention(dim, 4, 2, 16, 16, l=32, d=16, l_sel=64, n_sel=4, w=64): dtype, dim, B, NSA_ROPE_SCALE
QKV = [("bf16", 64, 1, 1), ("bf16", 64, 2, 1), ("fp16", 64, 1, 1), ("fp16", 64, 2, 1), ("bf16", 40, 3, 1), ("bf16", 40, 9, 1),
       ("fp32", 64, 3, 1), ("bf16", 64, 3, 1), ("bf16", 64, 70, 1), ("bf16", 64, 2, 3)]
QKV_PREFILL, QKV_LAST = 33, 48  # decode steps t = 33 .. 48; step 47 emits a compressed token
# nsa_rope_cache_append / _bwd at G 2, h 2, D 16: dtype, B, S, t0
ROPE = [(dt, B, S, t0) for dt in ("bf16", "fp32") for (B, S, t0) in ((2, 5, 0), (1, 3, 65533))]
ROPE_GEOM = (2, 2, 16, 16)
CACHES = ("K_sel", "V_sel", "K_win", "V_win", "K_raw", "V_raw")


def vals(*key_shape, key, scale=1.0):
    """fp32 array of bf16-representable values from the PCG64 stream `key`"""
    return _bf16_round(randn(_rng(31, *key), *key_shape) * np.float32(scale))


def linear_inputs(M, N, K, epi, ci):
    return dict(A=vals(M, K, key=(1, ci, 0)), W=vals(N, K, key=(1, ci, 1), scale=K ** -0.5), res=vals(M, N, key=(1, ci, 2)) if epi == 2 else None)


def module_state(module, tag):
    """{name: fp32 array} for every parameter in state-dict order: matrices ~ N(0, 1 / fan_in), norm weights ~ 1 + 0.1 N(0, 1), other vectors
    ~ 0.02 N(0, 1)"""
    out = {}
    for i, (name, p) in enumerate(module.state_dict().items()):
        shape = tuple(p.shape)
        if len(shape) == 2:
            out[name] = vals(*shape, key=(2, tag, i), scale=shape[1] ** -0.5)
        elif "norm" in name:
            out[name] = _bf16_round(np.float32(1.0) + vals(*shape, key=(2, tag, i), scale=0.1))
        else:
            out[name] = vals(*shape, key=(2, tag, i), scale=0.02)
    return out


def model_tokens(vocab, B, ci):
    return _rng(31, 3, ci).integers(0, vocab, (B, MODEL_PREFILL + MODEL_STEPS))


def qkv_inputs(dim, B, ci):
    return vals(B, QKV_LAST + 1, dim, key=(4, ci))


def rope_inputs(B, S, ci):
    G, h, Dk, Dv = ROPE_GEOM
    NQ = G * h * Dk
    g = {"proj": vals(B, S, NQ + 3 * G * Dk + 3 * G * Dv, key=(5, ci, 0)), "dQ": vals(B, S, NQ, key=(5, ci, 1))}
    for j, k in enumerate(CACHES):
        g["d" + k] = vals(B, G, S, Dk if k[0] == "K" else Dv, key=(5, ci, 2 + j))
    return g


class Out(dict):
    def put(self, key, t, big=None):
        """t: a device / host tensor of a kernel dtype -> its bit pattern (big: the size from which only the ends + SHA-256 are kept; default BIG)"""
        big = BIG if big is None else big
        import torch

        a = t.detach().contiguous().cpu()
        bits = a.view(torch.int16 if a.element_size() == 2 else torch.int32).numpy().view(np.uint16 if a.element_size() == 2 else np.uint32).reshape(-1)
        if bits.size > big:
            self[key + ".sha"] = np.frombuffer(hashlib.sha256(bits.tobytes()).digest(), np.uint32).copy()
            bits = np.concatenate([bits[:big // 2], bits[-big // 2:]])
        self[key] = bits.copy()


def run_linear(out):
    import torch
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _DT, _stream

    DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
    for dt in DTS:
        for form, table in (("fast", LINEAR_FAST), ("loop", LINEAR_LOOP)):
            if dt == "fp32" and form == "fast":
                continue
            for ci, (M, N, K, epi) in enumerate(table):
                g = linear_inputs(M, N, K, epi, ci)
                W = torch.from_numpy(g["W"]).to(DT[dt]).cuda()
                off = 1 if (form == "loop" and dt != "fp32") else 0  # elements: 2 bytes off a 16-byte boundary
                buf = torch.zeros(M * K + 8, dtype=DT[dt], device="cuda")
                A = buf[off: off + M * K].view(M, K)
                A.copy_(torch.from_numpy(g["A"]).to(DT[dt]))
                assert W.data_ptr() % 16 == 0 and (A.data_ptr() % 16 == 0) == (off == 0)
                res = torch.from_numpy(g["res"]).to(DT[dt]).cuda() if epi == 2 else None
                o = torch.empty(M, N, dtype=DT[dt], device="cuda")
                _lib.check(_lib.lib().nsa_linear_small(A.data_ptr(), W.data_ptr(), o.data_ptr(), M, N, K, _DT[DT[dt]], epi,
                                                       res.data_ptr() if res is not None else None, _stream(W.device)), "nsa_linear_small")
                torch.cuda.synchronize()
                out.put(f"linear/{dt}/{form}/M{M}_N{N}_K{K}_e{epi}", o)


def load_state(module, tag, dtype):
    import torch

    st = {k: torch.from_numpy(v) for k, v in module_state(module, tag).items()}
    module.load_state_dict(st)
    return module.cuda().to(dtype).eval()


def run_model(out):
    import torch
    from nsa_vibe_amd.llama_block_nsa import TinyLM

    DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
    for ci, (cfg, dt, B) in enumerate(MODEL):
        lm = load_state(TinyLM(*cfg), cfg[1], DT[dt])
        tok = torch.from_numpy(model_tokens(cfg[0], B, ci)).cuda()
        with torch.no_grad():
            caches = lm.new_caches(B, MODEL_PREFILL + MODEL_STEPS + 1, "cuda", DT[dt])
            lm.prefill(tok[:, :MODEL_PREFILL], caches)
            assert lm._native_decode_ok(tok[:, :1], caches), "the model decode step must take the one-call native route"
            for s in range(MODEL_STEPS):
                lg = lm.decode(tok[:, MODEL_PREFILL + s: MODEL_PREFILL + s + 1], caches)
                torch.cuda.synchronize()
                out.put(f"model/dim{cfg[1]}/{dt}/B{B}/step{s}", lg)


def run_qkv(out):
    import torch
    from nsa_vibe_amd.nsa_attention import NSAAttention

    DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
    saved = {k: os.environ.get(k) for k in ("NSA_HIP_STRICT", "NSA_ROPE_SCALE")}
    try:
        os.environ["NSA_HIP_STRICT"] = "1"
        for ci, (dt, dim, B, scale) in enumerate(QKV):
            os.environ["NSA_ROPE_SCALE"] = str(scale)
            m = load_state(NSAAttention(dim, 4, 2, 16, 16, l=32, d=16, l_sel=64, n_sel=4, w=64), dim, DT[dt])
            x = torch.from_numpy(qkv_inputs(dim, B, ci)).to(DT[dt]).cuda()
            with torch.no_grad():
                kv = m.new_kv(B, QKV_LAST + 2, "cuda", DT[dt])
                _, kv = m(x[:, :QKV_PREFILL], kv, prefill=True)
                ys = []
                for t in range(QKV_PREFILL, QKV_LAST + 1):
                    y, kv = m(x[:, t: t + 1], kv, prefill=False)
                    ys.append(y)
                torch.cuda.synchronize()
            assert m._fallback_counters["total_fallbacks"] == 0
            key = f"qkv/{dt}/dim{dim}/B{B}/s{scale}"
            out.put(key + "/y", torch.cat(ys, dim=1))
            for k in CACHES:
                out.put(f"{key}/{k}", getattr(kv, "_" + k)[:, :, QKV_PREFILL: QKV_LAST + 1])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_rope(out):
    import torch
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.selection_scorer import _stream

    DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
    G, h, Dk, Dv = ROPE_GEOM
    for ci, (dt, B, S, t0) in enumerate(ROPE):
        g = rope_inputs(B, S, ci)
        dev = {k: torch.from_numpy(v).to(DT[dt]).cuda() for k, v in g.items()}
        ds = _lib.NsaLayerDesc()
        ds.dim, ds.G, ds.h, ds.Dk, ds.Dv = G * h * Dv, G, h, Dk, Dv
        ds.l, ds.d, ds.l_sel, ds.n_sel, ds.w = 32, 16, 64, 16, 512
        ds.gate_hidden, ds.dtype, ds.gate_tau = 8, _lib.NSA_DT_F32 if dt == "fp32" else _lib.NSA_DT_BF16, 1.0
        ds.rope_base, ds.rope_scale = 10000.0, 1.0
        S_max = t0 + S + 8
        cache = {k: torch.zeros((B, G, S_max, Dk if k[0] == "K" else Dv), dtype=DT[dt], device="cuda") for k in CACHES}
        cache["K_cmp"], cache["V_cmp"] = (torch.zeros((B, G, 1, D), dtype=DT[dt], device="cuda") for D in (Dk, Dv))
        kd = _lib.NsaKvDesc()
        for k, v in cache.items():
            setattr(kd, k, v.data_ptr())
        kd.B, kd.S_max, kd.n_cmp_max = B, S_max, 1
        Q = torch.zeros((B, S, G * h * Dk), dtype=DT[dt], device="cuda")
        st = _stream(Q.device)
        _lib.check(_lib.lib().nsa_rope_cache_append(ctypes.byref(ds), ctypes.byref(kd), dev["proj"].data_ptr(), Q.data_ptr(), S, t0, st),
                   "nsa_rope_cache_append")
        torch.cuda.synchronize()
        key = f"rope/{dt}/B{B}_S{S}_t{t0}"
        out.put(key + "/Q", Q)
        for k in CACHES:
            out.put(f"{key}/{k}", cache[k][:, :, t0: t0 + S])
        # all six cache gradients given / dK_win and the compressed branch's value gradient (dV_raw, the source of V_cmp) null
        for name, null in (("all", ()), ("null", ("K_win", "V_raw"))):
            ptrs = [None if k in null else dev["d" + k].data_ptr() for k in CACHES]
            dproj = torch.zeros_like(dev["proj"])
            _lib.check(_lib.lib().nsa_rope_cache_append_bwd(ctypes.byref(ds), B, S, t0, dev["dQ"].data_ptr(), *ptrs, dproj.data_ptr(), st),
                       "nsa_rope_cache_append_bwd")
            torch.cuda.synchronize()
            out.put(f"{key}/bwd_{name}", dproj)


def run_cases():
    out = Out()
    run_linear(out)
    run_rope(out)
    run_qkv(out)
    run_model(out)
    return out


def list_cases():
    """every input builder, on the CPU: shapes, dtypes and pointer offsets of the case table"""
    n = 0
    for form, table in (("fast", LINEAR_FAST), ("loop", LINEAR_LOOP)):
        for ci, (M, N, K, epi) in enumerate(table):
            g = linear_inputs(M, N, K, epi, ci)
            assert g["A"].shape == (M, K) and g["W"].shape == (N, K) and (g["res"] is None) == (epi != 2) and g["A"].dtype == np.float32
            print(f"linear {form}: M {M} N {N} K {K} epi {epi}  A offset {2 if form == 'loop' else 0} bytes (16-bit), fp32 aligned")
            n += 1
    for ci, (dt, B, S, t0) in enumerate(ROPE):
        g = rope_inputs(B, S, ci)
        print(f"rope {dt}: B {B} S {S} t0 {t0}  proj {g['proj'].shape}  dK_sel {g['dK_sel'].shape}")
        n += 1
    for ci, (dt, dim, B, scale) in enumerate(QKV):
        print(f"qkv {dt}: dim {dim} B {B} scale {scale}  x {qkv_inputs(dim, B, ci).shape}")
        n += 1
    from nsa_vibe_amd.llama_block_nsa import TinyLM
    from nsa_vibe_amd.nsa_attention import NSAAttention

    for dim in sorted({c[1] for c in QKV}):
        m = NSAAttention(dim, 4, 2, 16, 16, l=32, d=16, l_sel=64, n_sel=4, w=64)
        m.load_state_dict({k: __import__("torch").from_numpy(v) for k, v in module_state(m, dim).items()})
    for ci, (cfg, dt, B) in enumerate(MODEL):
        lm = TinyLM(*cfg)
        lm.load_state_dict({k: __import__("torch").from_numpy(v) for k, v in module_state(lm, cfg[1]).items()})
        tok = model_tokens(cfg[0], B, ci)
        assert tok.shape == (B, MODEL_PREFILL + MODEL_STEPS) and tok.max() < cfg[0]
        print(f"model {dt}: TinyLM{cfg} B {B}  tokens {tok.shape}")
        n += 1
    print(f"{n} case groups constructed")


if __name__ == "__main__":
    if sys.argv[1:] == ["--list"]:
        list_cases()
    else:
        res = run_cases()
        np.savez_compressed(sys.argv[1], **res)
        print(f"{len(res)} arrays, {os.path.getsize(sys.argv[1])} bytes -> {sys.argv[1]}")
