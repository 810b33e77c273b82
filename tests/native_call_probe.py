"""What the Python package asks of the native library, call by call: a recording proxy in place of the loaded library object, a fixed table
of scenarios over every host route of the package, and the SHA-256 of everything they return and leave in the caches.

    python tests/native_call_probe.py OUT.json            # run every scenario on the device, write the record
    python tests/native_call_probe.py --merge A B OUT     # two records -> the fixture (the traces must agree; a hash is kept where both agree)

tests/golden/python_call_trace.json was recorded with this script, twice, from the package of the commit before the host idioms moved into
_native.py and the cache bookkeeping into NSA_KV; tests/test_hip_python_trace.py replays the scenarios on the package as it is.  A helper,
not a test.

A call is recorded as [entry point, [argument, ...]] by the C signature (nsa_vibe_amd._lib.SIGNATURES):
  * int / float arguments as they are; descriptor structs passed by reference (or as arrays) field by field;
  * a pointer -- descriptor fields included -- canonically: "null", "<name>+<byte offset>" of a registered tensor (inputs, parameters, the
    eight cache buffers), or "scratch/a<N>" with N the largest power of two up to 256 that divides the address;
  * a size_t (a workspace length) as "covers" when it is at least the answer of the workspace queries made since the previous launch (the
    largest of them; a call without a query of its own, such as a decode step on its cached context, is held to what the last call of the
    same entry point was held to), else the raw value: the pool only grows, so its surplus depends on what ran before;
  * out-int pointers of the plan calls as "out".
Pure queries (is_query) are part of the record; the replay holds the one-call routes to them and lists them for the per-stage routes.
Probe.decline(entry) makes the proxy answer a status for the next call of that entry point without calling it.

Inputs come from numpy PCG64 streams rounded to bf16-representable values (the tests/golden_inputs.py recipe)."""
import contextlib
import ctypes
import hashlib
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from golden_inputs import _bf16_round, _rng, randn  # noqa: E402

CACHES = ("_K_sel", "_V_sel", "_K_win", "_V_win", "_K_raw", "_V_raw", "_K_cmp", "_V_cmp")
READS = ("reads_pred", "reads_act_total", "reads_act_sel", "reads_act_cmp", "reads_act_win")
# not recorded: the library's own housekeeping, and the host builder of the block metadata (block_index.py; host pointers, and it runs only
# when the process-wide metadata cache misses, which depends on what ran before)
SILENT = ("nsa_hip_abi_version", "nsa_hip_last_error", "nsa_hip_set_tuning", "nsa_block_counts", "nsa_build_block_meta_host")
DIM, HEADS, G, D, L_, D_, LS, N, W, B = 256, 8, 2, 64, 32, 16, 64, 16, 512, 2
H = HEADS // G
ENV = ("NSA_HIP_STRICT", "NSA_FORCE_PARITY", "NSA_PREFILL_TILE", "NSA_PREFILL_BATCHED", "NSA_ROPE_SCALE", "NSA_FORCE_UNIFORM_GATE", "NSA_FORCE_BRANCH",
       "NSA_HIP_EAGER_TRAIN")


def is_query(name):
    return "_workspace" in name or name.endswith("_plan") or name in ("nsa_batched_ranges_width", "nsa_hip_get_tuning", "nsa_hip_device_check")


def vals(*shape, key, scale=1.0):
    return _bf16_round(randn(_rng(53, *key), *shape) * np.float32(scale))


def sha(t):
    a = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(a.view(__import__("torch").uint8).numpy().tobytes()).hexdigest()


class Probe:
    """stands where nsa_vibe_amd._lib keeps the loaded library: every attribute is the library's function behind a recorder"""

    def __init__(self, real, signatures):
        self.real, self.sig = real, signatures
        self.calls, self.registry, self.declined = [], [], {}
        self.pending, self.needs, self.need = [], {}, 0
        self.record = {}

    # ---- what the scenarios say --------------------------------------------------------------------------------------------------------
    def register(self, name, get):
        """a tensor (or a function returning the current one) whose addresses are recorded as name + offset"""
        self.registry.append((name, get if callable(get) else (lambda t=get: t)))

    def register_module(self, prefix, module):
        for n, p in module.named_parameters():
            self.register(f"{prefix}.{n}", p)

    def register_kv(self, prefix, kv):
        for c in CACHES:
            self.register(f"{prefix}.{c}", lambda kv=kv, c=c: getattr(kv, c))

    def decline(self, entry, status=3):
        self.declined[entry] = status

    @contextlib.contextmanager
    def scenario(self, name, one_call):
        """the calls and hashes of one scenario -> self.record[name]; one_call: the replay holds the pure queries to the record as well"""
        import torch

        self.calls, out = [], {}
        yield out
        torch.cuda.synchronize()
        assert name not in self.record and not self.declined, (name, self.declined)
        self.record[name] = {"one_call": bool(one_call), "calls": self.calls, "hashes": {k: (sha(v) if hasattr(v, "data_ptr") else v) for k, v in out.items()}}
        self.calls = []

    # ---- the proxy -------------------------------------------------------------------------------------------------------------------------
    def pointer(self, p):
        p = getattr(p, "value", p)
        if not p:
            return "null"
        for name, get in self.registry:
            t = get()
            if t is not None and t.data_ptr() <= p < t.data_ptr() + max(1, t.untyped_storage().nbytes() - (t.data_ptr() - t.untyped_storage().data_ptr())):
                return f"{name}+{p - t.data_ptr()}"
        return f"scratch/a{min(256, p & -p)}"

    def struct(self, s):
        out = {}
        for name, typ in s._fields_:
            v = getattr(s, name)
            out[name] = self.pointer(v) if typ is ctypes.c_void_p else self.struct(v) if isinstance(v, ctypes.Structure) else v
        return out

    def argument(self, typ, a):
        if typ is ctypes.c_void_p:
            return self.pointer(a)
        if typ is ctypes.c_size_t:
            return "covers" if int(a) >= self.need else int(a)
        if typ is ctypes.c_float:
            return float(a)
        if typ is ctypes.c_char_p:
            return a.decode()
        if typ in (ctypes.c_int, ctypes.c_int64):
            return int(a)
        if isinstance(a, ctypes.Array):  # an array of descriptors
            return [self.struct(e) for e in a]
        obj = getattr(a, "_obj", None)  # byref(x)
        if isinstance(obj, ctypes.Structure):
            return self.struct(obj)
        return "out"

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name in SILENT or name not in self.sig:
            return fn
        argtypes = self.sig[name][1]

        def call(*args):
            query = is_query(name)
            if not query:
                if self.pending:
                    self.needs[name], self.pending = max(self.pending), []
                self.need = self.needs.get(name, 0)
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            rec = [name, [self.argument(t, a) for t, a in zip(argtypes, args)]]
            self.calls.append(rec)
            if name in self.declined:
                rec.append("declined")
                return self.declined.pop(name)
            rc = fn(*args)
            if "_workspace" in name:
                self.pending.append(int(rc))
            return rc

        call.__name__ = name
        return call


def install():
    from nsa_vibe_amd import _lib

    real = _lib.lib()
    if isinstance(real, Probe):
        return real
    _lib._lib = Probe(real, _lib.SIGNATURES)
    return _lib._lib


def uninstall():
    from nsa_vibe_amd import _lib

    if isinstance(_lib._lib, Probe):
        _lib._lib = _lib._lib.real


# ---- scenarios -----------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def env(**kw):
    """the switches a module reads at construction: all unset but those given"""
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ["NSA_HIP_STRICT"] = "1"
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def load_state(module, tag):
    """parameters from the streams (matrices ~ N(0, 1 / fan_in), norm weights ~ 1 + 0.1 N, other vectors ~ 0.02 N), bf16 on the device"""
    import torch

    st = {}
    for i, (name, p) in enumerate(module.state_dict().items()):
        shape = tuple(p.shape)
        if len(shape) == 2:
            st[name] = vals(*shape, key=(1, tag, i), scale=shape[1] ** -0.5)
        elif "norm" in name:
            st[name] = _bf16_round(np.float32(1.0) + vals(*shape, key=(1, tag, i), scale=0.1))
        else:
            st[name] = vals(*shape, key=(1, tag, i), scale=0.02)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    return module.cuda().to(torch.bfloat16).eval()


def attention(tag, **kw):
    from nsa_vibe_amd.nsa_attention import NSAAttention

    return load_state(NSAAttention(DIM, HEADS, G, D, D, l=L_, d=D_, l_sel=LS, n_sel=N, w=W, **kw), tag)


def dev(a, dtype=None):
    import torch

    t = torch.from_numpy(a).cuda()
    return t.to(dtype or torch.bfloat16) if a.dtype == np.float32 else t


def put_kv(out, key, kv):
    out[f"{key}/t"], out[f"{key}/n_cmp"], out[f"{key}/meta_seq_len"] = int(kv.t), int(kv.n_cmp), int(kv.meta_seq_len)
    for r in READS:
        out[f"{key}/{r}"] = [int(v) for v in getattr(kv, r)]
    for c in CACHES:
        out[f"{key}/{c}"] = getattr(kv, c)[:, :, :(kv.n_cmp if "cmp" in c else kv.t)]


def put_layer(out, m, y, kv, key="kv"):
    out["y"], out["ranges"], out["gates"] = y, m._last_ranges, m._last_gates
    put_kv(out, key, kv)


def run_layer(p):
    """the module routes: prefill (both selectors), decode steps, decode_rows, extend, tiled prefill"""
    import torch

    x = dev(vals(B, 256, DIM, key=(2,)))
    for selector in ("sequential", "batched"):
        with env():
            m = attention(3, selector=selector)
        kv = m.new_kv(B, 256, "cuda", torch.bfloat16)
        p.registry = []
        p.register("x", x)
        p.register_module("m", m)
        p.register_kv("kv", kv)
        with p.scenario(f"prefill110/{selector}", True) as out:
            put_layer(out, m, m(x[:, :110], kv, prefill=True)[0], kv)
        if selector == "batched":
            continue
        for s in range(3):  # t = 110, 111, 112: the token count reaches 112 + 1, one compressed token is emitted
            with p.scenario(f"decode/step{s}", True) as out:
                put_layer(out, m, m(x[:, 110 + s: 111 + s], kv, prefill=False)[0], kv)
        with p.scenario("decode_rows/S16_from113", True) as out:  # crosses 128: the metadata refreshes
            put_layer(out, m, m.decode_rows(x[:, 113:129], kv)[0], kv)
        with p.scenario("decode_rows/S1", True) as out:  # the plan declines: a single step
            put_layer(out, m, m.decode_rows(x[:, 129:130], kv)[0], kv)
        with p.scenario("extend/40_onto_130", True) as out:
            put_layer(out, m, m(x[:, 130:170], kv, prefill=True)[0], kv)
    with env():
        m = attention(3, selector="sequential", prefill_tile=32)
    kv = m.new_kv(B, 128, "cuda", torch.bfloat16)
    p.registry = []
    p.register("x", x)
    p.register_module("m", m)
    p.register_kv("kv", kv)
    with p.scenario("prefill_tile32/100", True) as out:  # chunks of 32, 32, 32, 4
        put_layer(out, m, m(x[:, :100], kv, prefill=True)[0], kv)


def run_declined(p):
    """each one-call entry point answered with a status once: the per-stage routes, and decode_rows' single steps"""
    import torch

    x = dev(vals(B, 256, DIM, key=(2,)))
    with env(NSA_HIP_STRICT=0):
        m = attention(3, selector="sequential")
    kv = m.new_kv(B, 256, "cuda", torch.bfloat16)
    p.registry = []
    p.register("x", x)
    p.register_module("m", m)
    p.register_kv("kv", kv)
    steps = (("prefill", "nsa_layer_prefill", lambda: m(x[:, :110], kv, prefill=True)[0]),
             ("decode", "nsa_layer_decode_step", lambda: m(x[:, 110:111], kv, prefill=False)[0]),
             ("extend", "nsa_layer_extend", lambda: m(x[:, 111:151], kv, prefill=True)[0]),
             ("decode_rows", "nsa_layer_decode_rows", lambda: m.decode_rows(x[:, 151:167], kv)[0]))
    for name, entry, fn in steps:
        with p.scenario(f"declined/{name}", False) as out, warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            p.decline(entry)
            put_layer(out, m, fn(), kv)
            out["fallbacks"] = m.get_fallback_counters()
            out["reached"] = entry not in p.declined  # the entry point was called, and answered by the proxy
            p.declined.clear()


def run_parity(p):
    import torch

    x = dev(vals(B, 256, DIM, key=(2,)))
    with env(NSA_FORCE_PARITY=1):
        m = attention(3, selector="sequential")
    kv = m.new_kv(B, 128, "cuda", torch.bfloat16)
    p.registry = []
    p.register("x", x)
    p.register_module("m", m)
    p.register_kv("kv", kv)
    with p.scenario("parity/prefill110", False) as out:
        put_layer(out, m, m(x[:, :110], kv, prefill=True)[0], kv)
    with p.scenario("parity/step", False) as out:
        put_layer(out, m, m(x[:, 110:111], kv, prefill=False)[0], kv)


def run_train(p):
    """one training forward and backward, S = 64, B = 1: every stage a differentiable native op"""
    import torch

    with env():
        m = attention(3, selector="sequential").train()
    x = dev(vals(1, 64, DIM, key=(4,))).requires_grad_()
    dy = dev(vals(1, 64, DIM, key=(5,)))
    kv = m.new_kv(1, 64, "cuda", torch.bfloat16)
    p.registry = []
    p.register("x", x)
    p.register("dy", dy)
    p.register_module("m", m)
    p.register_kv("kv", kv)
    with p.scenario("train/S64", False) as out, torch.enable_grad():
        y, _ = m(x, kv, prefill=True)
        y.backward(dy)
        put_layer(out, m, y, kv)
        out["grad/x"] = x.grad
        for n, q in m.named_parameters():
            out[f"grad/{n}"] = q.grad


def run_block_and_model(p):
    import torch
    from nsa_vibe_amd.llama_block_nsa import LlamaBlockNSA, TinyLM

    x = dev(vals(B, 111, DIM, key=(6,)))
    with env():
        blk = load_state(LlamaBlockNSA(DIM, HEADS, G, D, D, L_, D_, LS, N, W), 7)
    kv = blk.attn.new_kv(B, 128, "cuda", torch.bfloat16)
    p.registry = []
    p.register("x", x)
    p.register_module("blk", blk)
    p.register_kv("kv", kv)
    with p.scenario("block/prefill110", True) as out:
        put_layer(out, blk.attn, blk(x[:, :110], kv, prefill=True), kv)
    with p.scenario("block/step", True) as out:
        put_layer(out, blk.attn, blk(x[:, 110:111], kv, prefill=False), kv)
    with env():
        lm = load_state(TinyLM(512, DIM, 2, HEADS, G, D, D, L_, D_, LS, N, W), 8)
    tok = torch.from_numpy(_rng(53, 9).integers(0, 512, (B, 111))).cuda()
    caches = lm.new_caches(B, 128, "cuda", torch.bfloat16)
    p.registry = []
    p.register("tokens", tok)
    p.register_module("lm", lm)
    for i, c in enumerate(caches):
        p.register_kv(f"kv{i}", c)
    with p.scenario("model/prefill110", True) as out:
        out["logits"] = lm.prefill(tok[:, :110], caches)
        for i, c in enumerate(caches):
            put_kv(out, f"kv{i}", c)
    with p.scenario("model/step", True) as out:
        out["logits"], out["next"] = lm.decode(tok[:, 110:111], caches, return_next=True)
        for i, c in enumerate(caches):
            put_kv(out, f"kv{i}", c)


def run_operators(p):
    """the operator level, S = 64 rows at tokens 64 .. 127 of S_kv = 128"""
    import torch
    import nsa_vibe_amd as nv
    from nsa_vibe_amd import selection_attention as sa

    S, S_kv, t0 = 64, 128, 64
    meta = nv.build_block_meta(S_kv, L_, D_, LS, N, W)
    n_cmp = (S_kv - L_) // D_ + 1
    Q, K, V = dev(vals(B, S, G, H, D, key=(10,))), dev(vals(B, G, S_kv, D, key=(11,))), dev(vals(B, G, S_kv, D, key=(12,)))
    Kc, Vc = dev(vals(B, G, n_cmp, D, key=(13,))), dev(vals(B, G, n_cmp, D, key=(14,)))
    dO = dev(vals(B, S, G, H, D, key=(15,)))
    r = _rng(53, 16)
    lo = r.integers(0, S_kv - 8, (B, S, G, 5))
    rg = dev(np.stack((lo, lo + r.integers(0, 40, lo.shape)), axis=-1).astype(np.int32))
    pos_dev = torch.tensor([112, 50], dtype=torch.int32, device="cuda")
    p.registry = []
    for n, t in (("Q", Q), ("K", K), ("V", V), ("Kc", Kc), ("Vc", Vc), ("dO", dO), ("ranges", rg), ("pos", pos_dev)):
        p.register(n, t)

    def grads(fn, *qkv):
        q, k, v = (t.detach().clone().requires_grad_() for t in qkv)
        for n, t in (("q", q), ("k", k), ("v", v)):
            p.register("grad_in_" + n, t)
        with torch.enable_grad():
            O = fn(q, k, v)
            O.backward(dO)
        return {"O": O, "dQ": q.grad, "dK": k.grad, "dV": v.grad}

    with p.scenario("op/sel_attn_fwd_lse", True) as out:
        out["O"], out["lse"] = nv.selection_attention_hip(Q, K, V, rg, return_lse=True)
    with p.scenario("op/sel_attn_bwd", True) as out:
        out.update(grads(lambda q, k, v: nv.selection_attention_hip(q, k, v, rg), Q, K, V))
    with p.scenario("op/scores", True) as out:
        out["p_grp"] = p_grp = nv.selection_scores(Q, Kc, meta)
        out["p_grp_rows"] = nv.selection_scores(Q, Kc, meta, q0=t0, normalize="causal")
        out["p_grp_skip"] = nv.selection_scores(Q, Kc, meta, causal_skip=True, q0=t0)
    p.register("p_grp", p_grp)
    for mode in ("batched", "sequential"):
        with p.scenario(f"op/select_and_attend/{mode}", True) as out:
            out["ranges"], out["O"] = nv.select_and_attend(p_grp, Q, K, V, meta, N, mode=mode, t0=t0)
        with p.scenario(f"op/scores_select/{mode}", True) as out:
            out["p_grp"], out["ranges"] = nv.selection_scores_select(Q, Kc, meta, N, mode=mode, leave_skipped=False)
            out["p_grp_rows"], out["ranges_rows"] = nv.selection_scores_select(Q, Kc, meta, N, mode=mode, t0=t0, q0=t0, normalize="causal",
                                                                               leave_skipped=False)
    with p.scenario("op/parity_modes", True) as out:
        out["first_key"] = nv.selection_attention_first_key_parity(Q, K, V, rg)
        out["head_causal"] = nv.selection_attention_head_causal_parity(Q, K, V, rg)
    with p.scenario("op/band_fwd", True) as out:
        out["win"], out["win_lse"] = nv.band_attention_hip(Q, K, V, t0=t0, w=50, return_lse=True)
        out["cmp"] = nv.batched_causal_attention_compressed(Q, Kc, Vc, L_, D_, t0=t0)
        out["win_host_pos"] = nv.sliding_window_attention(Q, K, V, 50, t_pos=[64, 30])
        out["cmp_host_pos"] = nv.batched_causal_attention_compressed(Q, Kc, Vc, L_, D_, t_pos=[64, 30])
    with p.scenario("op/band_bwd/win", True) as out:
        out.update(grads(lambda q, k, v: nv.sliding_window_attention(q, k, v, 50, t0=t0), Q, K, V))
    with p.scenario("op/band_bwd/cmp", True) as out:
        out.update(grads(lambda q, k, v: nv.batched_causal_attention_compressed(q, k, v, L_, D_, t0=t0), Q, Kc, Vc))
    with p.scenario("op/decode", True) as out:
        out["step_O"], out["step_ranges"] = nv.selection_decode_step(Q[:, :1], Kc, K, V, meta, N, S_kv - 1)
        out["rows_O"], out["rows_ranges"] = sa.selection_decode_rows(Q[:, :16], Kc, K, V, meta, N, 112)
        out["ragged_O"], out["ragged_ranges"] = sa.selection_decode_ragged(Q[:, :16], Kc, K, V, meta, N, pos_dev, t_max=127)
    with p.scenario("op/plans", True) as out:
        out["step"] = sa.selection_decode_step_plan(B, G, H, D, D, n_cmp, meta.S_sel, S_kv, N)
        out["rows"] = sa.selection_decode_rows_plan(B, 16, G, H, D, D, n_cmp, meta.S_sel, S_kv, N)
        out["ragged"] = sa.selection_decode_ragged_plan(B, 16, G, H, D, D, n_cmp, meta.S_sel, S_kv, N, 127)
        with env():
            m = attention(3, selector="sequential")
        out["layer_rows"] = m.decode_rows_plan(B, 16, 256, 113, 3)
    # host positions at a t_max the ragged plan declines (D = 128: more than 16 chunks of compressed tokens): one rows call per live sequence
    T, D2 = 20000, 128
    nc = (T - L_) // D_ + 1
    meta2 = nv.build_block_meta(T, L_, D_, LS, N, W)
    tile = lambda n, key: dev(vals(B, G, 500, D2, key=key)).repeat(1, 1, (n + 499) // 500, 1)[:, :, :n].contiguous()  # noqa: E731
    Q2, K2, V2, Kc2 = dev(vals(B, 2, G, H, D2, key=(20,))), tile(T, (21,)), tile(T, (22,)), tile(nc, (23,))
    p.registry = []
    for n, t in (("Q", Q2), ("K", K2), ("V", V2), ("Kc", Kc2)):
        p.register(n, t)
    with p.scenario("op/decode_ragged_host_declined", False) as out:
        out["O"], out["ranges"] = sa.selection_decode_ragged(Q2, Kc2, K2, V2, meta2, N, [T - 2, 100])


def run_all():
    import torch

    p = install()
    p.record = {}
    try:
        with torch.no_grad():
            for fn in (run_layer, run_declined, run_parity, run_train, run_block_and_model, run_operators):
                fn(p)
        return p.record
    finally:
        uninstall()


def launches(calls):
    """the calls that can launch or write"""
    return [c for c in calls if not is_query(c[0])]


def merge(a, b):
    """two records of the same package -> the fixture; the second return value names the hashes that differ"""
    out, differ = {}, []
    assert a.keys() == b.keys()
    for name in a:
        assert a[name]["calls"] == b[name]["calls"], f"{name}: the two recordings made different calls"
        keep = {k: v for k, v in a[name]["hashes"].items() if b[name]["hashes"].get(k) == v}
        differ += [f"{name}:{k}" for k in a[name]["hashes"] if k not in keep]
        out[name] = {"one_call": a[name]["one_call"], "calls": a[name]["calls"], "hashes": keep}
    return out, differ


if __name__ == "__main__":
    if sys.argv[1:2] == ["--merge"]:
        rec, differ = merge(json.load(open(sys.argv[2])), json.load(open(sys.argv[3])))
        print(f"{len(rec)} scenarios, {sum(len(v['calls']) for v in rec.values())} calls, {sum(len(v['hashes']) for v in rec.values())} hashes kept; "
              f"differing: {differ}")
        json.dump(rec, open(sys.argv[4], "w"), separators=(",", ":"))
    else:
        rec = run_all()
        json.dump(rec, open(sys.argv[1], "w"), separators=(",", ":"))
        print(f"{len(rec)} scenarios, {sum(len(v['calls']) for v in rec.values())} calls -> {sys.argv[1]}")
