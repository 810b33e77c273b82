"""CPU (no GPU): the C-ABI library loads and exports every symbol include/nsa_sel_hip.h declares, host-side
logic (block meta closed form, forced-column rule, error behaviour, sharding) is correct, and the N>1 path's
host plumbing works under gloo with world_size 2.  No device compute is called here."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def nv():
    import nsa_vibe_amd
    from nsa_vibe_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return nsa_vibe_amd


def test_library_exports_every_declared_symbol(nv):
    from nsa_vibe_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "nsa_sel_hip.h")).read()
    declared = set(re.findall(r"NSA_API\s+[\w\s\*]+?\b(nsa_\w+)\s*\(", hdr))
    assert len(declared) >= 14
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in the header but not exported"
    assert declared == set(_lib.SIGNATURES), "python binding table and header disagree"
    assert _lib.lib().nsa_hip_abi_version() == 1


def test_product_never_touches_the_oracle():
    """The oracle is test infrastructure: nothing under nsa_vibe_amd/ may import or load it."""
    pkg = os.path.join(ROOT, "nsa_vibe_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "nsa_oracle" not in txt and "oracle/" not in txt and "from oracle" not in txt, f


def test_missing_library_fails_loudly(nv, tmp_path, monkeypatch):
    from nsa_vibe_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError):
        _lib.lib()


def test_cpu_tensors_are_rejected_not_emulated(nv):
    with pytest.raises(RuntimeError):
        nv.selection_attention_hip(torch.zeros(1, 1, 1, 1, 8), torch.zeros(1, 1, 4, 8), torch.zeros(1, 1, 4, 8),
                                   torch.zeros(1, 1, 1, 1, 2, dtype=torch.int32))
    m = nv.build_block_meta(256, 32, 16, 64, 16, 512)
    with pytest.raises(RuntimeError):
        nv.select_topn_ranges(torch.zeros(1, 1, m.S_sel), m, 4, 100)
    with pytest.raises(RuntimeError):
        nv.compute_pcmp_all(torch.zeros(1, 2, 1, 1, 8), torch.zeros(1, 1, 3, 8), 1.0)


def test_block_meta_closed_form_matches_reference_goldens(nv):
    g = load_golden("g1_block_meta")
    for i, (S, l, d, ls) in enumerate(g["cases"]):
        m = nv.build_block_meta(int(S), int(l), int(d), int(ls), 16, 512)
        assert np.array_equal(m.cmp_starts.numpy(), g[f"c{i}_cmp_starts"])
        assert np.array_equal(m.sel_starts.numpy(), g[f"c{i}_sel_starts"])
        assert np.array_equal(m.M_csl_indptr.numpy(), g[f"c{i}_indptr"])
        assert np.array_equal(m.M_csl_indices.numpy(), g[f"c{i}_indices"])
        assert np.array_equal(m.M_csl_values.numpy(), g[f"c{i}_values"])
        assert np.array_equal(m.M_csl_coo_indices.numpy(), g[f"c{i}_coo"])
        assert m.M_csl_indptr.dtype == torch.int32 and m.M_csl_values.dtype == torch.float32
        # CSC = the same entries regrouped by selection block, ascending compressed row inside a block
        rows, cols = g[f"c{i}_coo"]
        vals = g[f"c{i}_values"]
        order = np.lexsort((rows, cols))
        assert np.array_equal(m.csc_rows.numpy(), rows[order])
        assert np.array_equal(m.csc_vals.numpy(), vals[order])
        assert np.array_equal(np.diff(m.csc_ptr.numpy()), np.bincount(cols, minlength=m.S_sel))


def test_block_meta_64k_is_fast_and_closed_form(nv):
    import time

    t0 = time.perf_counter()
    m = nv.build_block_meta(65536, 32, 16, 64, 16, 512)
    assert time.perf_counter() - t0 < 1.0  # the reference's Python double loop takes seconds here
    assert m.S_cmp == 4095 and m.S_sel == 1024
    # 5-tap stencil 1/2,1,1,1,1/2 on rows 4j-1..4j+3
    j = 500
    k0, k1 = int(m.csc_ptr[j]), int(m.csc_ptr[j + 1])
    assert m.csc_rows[k0:k1].tolist() == [4 * j - 1, 4 * j, 4 * j + 1, 4 * j + 2, 4 * j + 3]
    assert m.csc_vals[k0:k1].tolist() == [0.5, 1.0, 1.0, 1.0, 0.5]


def test_divisibility_guards(nv):
    with pytest.raises(ValueError):
        nv.build_block_meta(1024, 30, 16, 64, 16, 512)
    with pytest.raises(ValueError):
        nv.build_block_meta(1024, 32, 12, 60, 16, 512)
    with pytest.raises(ValueError):
        nv.build_block_starts(10, 0, 1, 1)


def test_batched_width_rule_matches_oracle(nv, orc):
    """closed-form forced-column rule (csrc/sel_select.hip batched_keepmask) vs the oracle's brute force."""
    for S in (1, 40, 63, 64, 65, 100, 127, 128, 129, 192, 193, 200, 1000, 4096):
        for ls in (16, 64):
            for n_top in (1, 2, 3, 4, 16, 100):
                for fi, fl in ((True, 2), (False, 2), (True, 0), (False, 0), (True, 3), (False, 1)):
                    m = orc.build_block_meta(S, ls, ls, ls, n_top, 512)
                    S_sel = m.sel_starts.size
                    want = orc.select_topn_ranges_batched(np.zeros((1, S, 1, S_sel), np.float32), m, n_top, S, fi, fl).shape[3]
                    got = nv.batched_ranges_width(S_sel, ls, n_top, S, fi, fl)
                    assert got == want, (S, ls, n_top, fi, fl)


def test_sharding_covers_every_row_once(nv):
    from nsa_vibe_amd.sharding import shard_batch, shard_bg

    for B in (1, 7, 8, 9, 64):
        for W in (1, 2, 3, 4, 8):
            spans = [shard_batch(B, W, r) for r in range(W)]
            assert spans[0][0] == 0 and spans[-1][1] == B
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert max(e - s for s, e in spans) - min(e - s for s, e in spans) <= 1
            got = sorted(p for r in range(W) for p in shard_bg(B, 2, W, r))
            assert got == [(b, g) for b in range(B) for g in range(2)]
    with pytest.raises(ValueError):
        shard_batch(4, 2, 2)


_WORKER = r"""
import os, sys, json
sys.path.insert(0, {root!r})
import torch, torch.distributed as dist
from nsa_vibe_amd.sharding import shard_batch, shard_bg, max_over_ranks, sum_over_ranks, barrier
dist.init_process_group(backend="gloo", init_method="tcp://127.0.0.1:{port}", rank=int(sys.argv[1]), world_size=2)
r = dist.get_rank()
B, G = 5, 2
s, e = shard_batch(B, 2, r)
# every rank "processes" its own sequences; no data-path collective: only the timing reductions bench.py uses
barrier()
t = max_over_ranks(1.0 + r)
n = sum_over_ranks(float(e - s))
owned = shard_bg(B, G, 2, r)
out = [None, None]
dist.all_gather_object(out, owned)
barrier()
if r == 0:
    print(json.dumps({{"tmax": t, "nsum": n, "pairs": sorted(tuple(p) for o in out for p in o)}}))
dist.destroy_process_group()
"""


def test_two_rank_gloo_sharding(tmp_path):
    """world_size 2 on CPU (gloo): the N>1 path = disjoint shards + barrier + max-over-ranks timing."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, port=port))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=240) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    import json

    res = json.loads(outs[0][0].strip().splitlines()[-1])
    assert res["tmax"] == 2.0 and res["nsum"] == 5.0
    assert res["pairs"] == [[b, g] for b in range(5) for g in range(2)]


def test_llama_block_state_dict_matches_reference():
    """LlamaBlockNSA / NSAAttention parameter names and shapes = the reference's (nsa/model/llama_block_nsa.py:33-63), so its
    checkpoints load unchanged (golden written from the imported reference module)"""
    import json
    import os

    from nsa_vibe_amd.llama_block_nsa import LlamaBlockNSA, TinyLM

    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "g14_llama_block_state_dict.json")))
    blk = LlamaBlockNSA(**g["args"])
    mine = {k: list(v.shape) for k, v in blk.state_dict().items()}
    assert mine == g["state_dict"]
    lm = TinyLM(100, 64, 2, 4, 2, 16, 16, 8, 4, 8, 4, 16)
    keys = set(lm.state_dict().keys())
    assert {"embed.weight", "norm_f.weight", "lm_head.weight", "blocks.0.attn.W_Q.weight", "blocks.1.mlp.fc2.weight"} <= keys


def test_kv_cache_grows_in_place_of_the_reference_cat(nv):
    """NSA_KV.reserve / ensure_capacity: contents kept, views keep the reference's shapes, cached native descriptors dropped;
    auto_grow=False restores the hard limit"""
    from nsa_vibe_amd.kv_cache import NSA_KV

    kv = NSA_KV(2, 2, 8, 8, 20, 4, 2, 8, 2, 16, "cpu", torch.float32)
    tok = lambda n: [torch.randn(2, 2, n, 8) for _ in range(6)]  # noqa: E731
    first = tok(20)
    kv.write_tokens(*first)
    kv.write_compressed(torch.ones(2, 2, 9, 8), torch.ones(2, 2, 9, 8), at=0)
    kv._native["desc"] = kv._native["layer_decode"] = object()
    more = tok(5)
    kv.write_tokens(*more)  # 25 > 20: doubles
    assert kv.S_max == 40 and kv._K_sel.shape[2] == 40 and kv._K_cmp.shape[2] == (40 - 4) // 2 + 1
    assert not kv._native
    assert torch.equal(kv.K_sel, torch.cat([first[0], more[0]], dim=2)) and torch.equal(kv.V_cmp_raw_seq[:, :, :20], first[5])
    assert kv.K_cmp.shape[2] == 9 and bool((kv.K_cmp == 1).all())
    assert kv.K_win.shape[2] == 16
    kv.reserve(30)  # never shrinks
    assert kv.S_max == 40
    fixed = NSA_KV(1, 1, 8, 8, 4, 4, 2, 8, 2, 16, "cpu", torch.float32, auto_grow=False)
    with pytest.raises(RuntimeError, match="capacity exceeded"):
        fixed.write_tokens(*[torch.zeros(1, 1, 5, 8) for _ in range(6)])


def test_ranges_shape_normalisation_like_the_reference_wrapper():
    """over-nested (extra singleton dims) and batch-less ranges are accepted as the reference's wrapper accepts them
    (test_ranges_normalization.py:6-24); anything else is a ValueError; the caller's int64 tensor is never modified"""
    from nsa_vibe_amd.selection_attention import _prep_ranges

    t6 = torch.zeros((1, 1, 2, 1, 1, 2), dtype=torch.int32)
    assert _prep_ranges(t6).shape == (1, 2, 1, 1, 2) or _prep_ranges(t6).dim() == 5
    t4 = torch.tensor([[[[0, 10], [40, 60]]]], dtype=torch.int64)
    keep = t4.clone()
    out = _prep_ranges(t4)
    assert out.shape == (1, 1, 1, 2, 2) and out.dtype == torch.int32 and out.is_contiguous() and torch.equal(t4, keep)
    with pytest.raises(ValueError):
        _prep_ranges(torch.zeros((2, 3, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        _prep_ranges(torch.zeros((1, 1, 1, 2, 3), dtype=torch.int32))


@pytest.mark.parametrize("flag,idx", [("cmp", 0), ("sel", 1), ("win", 2)])
def test_gate_force_branch_env_like_the_reference(flag, idx, monkeypatch):
    """NSA_FORCE_BRANCH / NSA_FORCE_UNIFORM_GATE are read at construction and override the gate (reference test_force_branch_gates.py,
    nsa_attention.py:42-70); the kernel-side parameters (fc2_params) encode the same override"""
    from nsa_vibe_amd.nsa_attention import GateMLP

    monkeypatch.setenv("NSA_FORCE_BRANCH", flag)
    g = GateMLP(d_k=8)
    p = g(torch.randn(2, 3, 8))
    assert p.shape == (2, 3, 3) and torch.all(torch.argmax(p, dim=-1) == idx) and torch.allclose(p.sum(-1), torch.ones(2, 3))
    w2, b2 = g.fc2_params()
    assert not w2.any() and int(torch.argmax(b2)) == idx and float(b2.max() - b2.min()) > 50.0
    monkeypatch.delenv("NSA_FORCE_BRANCH")
    monkeypatch.setenv("NSA_FORCE_UNIFORM_GATE", "1")
    u = GateMLP(d_k=8)
    assert torch.allclose(u(torch.randn(4, 8)), torch.full((4, 3), 1.0 / 3.0))
    w2, b2 = u.fc2_params()
    assert not w2.any() and not b2.any()
    monkeypatch.delenv("NSA_FORCE_UNIFORM_GATE")
    plain = GateMLP(d_k=8)
    assert plain.fc2_params()[0] is plain.fc2.weight and not plain.forced()


def test_eq9_slow_path_matches_the_oracle_mapping(nv, orc):
    """map_pcmp_to_pslc_slow_path (dense p . M, the reference's verifier path selection_scorer.py:608-655) == the oracle's Eq.9 stencil"""
    rng = np.random.default_rng(5)
    S = 1000
    meta = nv.build_block_meta(S, 32, 16, 64, 16, 512)
    om = orc.build_block_meta(S, 32, 16, 64, 16, 512)
    p = rng.random((1, 3, 2, 4, meta.S_cmp), dtype=np.float32)
    p_slc, _ = orc.map_pcmp_to_pslc_and_pgrp(p, om)
    got = nv.map_pcmp_to_pslc_slow_path(torch.from_numpy(p), meta).numpy()
    assert np.abs(got - p_slc).max() <= 1e-6
    short = nv.map_pcmp_to_pslc_slow_path(torch.from_numpy(p[..., :10]), meta)  # fewer compressed rows than the meta covers
    assert short.shape[-1] == meta.S_sel and not short[..., 4:].any()
    ok, info = nv.verify_mapping_equivalence(torch.from_numpy(p), meta)
    assert ok and info["status"] == "skipped"


def test_routing_contract_counts_a_failed_native_call_and_raises(monkeypatch):
    """counterpart of nsa/tests/test_cuda_loader_fallback.py:6-38 for the routing contract of nsa_attention.py:764-782: a native call
    that fails bumps selection_hip_fails / total_fallbacks; on the CPU no native executor is left to fall back to (CPU tensors make every
    native entry refuse: the per-stage composition is already the last one), so the error is raised.  The fall-back of the one-call layer
    to the per-stage native route is pinned on the GPU (tests/test_hip_module.py::test_native_call_failure_is_counted_and_falls_back)"""
    import torch

    from nsa_vibe_amd.nsa_attention import NSAAttention

    m = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=16, n_sel=4, w=16).eval()
    x = torch.randn(1, 24, 64)
    with torch.no_grad():
        for i in range(2):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                m(x, m.new_kv(1, 32, "cpu", torch.float32), prefill=True)
            c = m.get_fallback_counters()
            assert c["selection_hip_fails"] == i + 1 and c["total_fallbacks"] == i + 1
    assert m.reset_fallback_counters()["selection_hip_fails"] == 2 and m.get_fallback_counters()["total_fallbacks"] == 0


def test_routing_contract_failing_library_call(monkeypatch):
    """a library whose entry point returns an error status (the BadExt of test_cuda_loader_fallback.py:9-22): RuntimeError with the
    library's message + counter, nothing is silently rerouted"""
    import torch

    import nsa_vibe_amd.selection_scorer as sc
    from nsa_vibe_amd import _lib
    from nsa_vibe_amd.nsa_attention import NSAAttention

    def bad_scores(*a, **k):
        _lib.check(-2, "nsa_sel_scores (synthetic forward failure)")

    monkeypatch.setattr("nsa_vibe_amd.nsa_attention.selection_scores", bad_scores)
    monkeypatch.setattr(sc, "_need_gpu", lambda *t: t[0].device)  # let CPU tensors reach the (failing) native call
    m = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=16, n_sel=4, w=16).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="synthetic forward failure"):
        m(torch.randn(1, 24, 64), m.new_kv(1, 32, "cpu", torch.float32), prefill=True)
    assert m.get_fallback_counters()["selection_hip_fails"] == 1


def test_force_parity_flag_is_read_at_construction(monkeypatch):
    """NSA_FORCE_PARITY (nsa_attention.py:300-332 flag cache, :704-708): read once when the module is built"""
    from nsa_vibe_amd.nsa_attention import NSAAttention

    monkeypatch.setenv("NSA_FORCE_PARITY", "1")
    m = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=16, n_sel=4, w=16)
    monkeypatch.setenv("NSA_FORCE_PARITY", "0")
    m2 = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=16, n_sel=4, w=16)
    assert m._force_parity and not m2._force_parity


def test_kv_cache_must_match_the_input():
    """the native calls walk kv.B sequences of the cache's dtype: a cache built for another batch / dtype / geometry is refused
    before any kernel can run out of bounds"""
    import torch

    from nsa_vibe_amd.llama_block_nsa import LlamaBlockNSA
    from nsa_vibe_amd.nsa_attention import NSAAttention

    m = NSAAttention(64, 4, 2, 16, 16, l=8, d=4, l_sel=16, n_sel=4, w=16).eval()
    x = torch.randn(2, 24, 64)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="does not match the input"):
            m(x, m.new_kv(3, 32, "cpu", torch.float32), prefill=True)  # larger batch in the cache
        with pytest.raises(RuntimeError, match="does not match the input"):
            m(x, m.new_kv(2, 32, "cpu", torch.bfloat16), prefill=True)  # other dtype
        other = NSAAttention(64, 4, 1, 16, 16, l=8, d=4, l_sel=16, n_sel=4, w=16)
        with pytest.raises(RuntimeError, match="geometry"):
            m(x, other.new_kv(2, 32, "cpu", torch.float32), prefill=True)
        blk = LlamaBlockNSA(64, 4, 2, 16, 16, l=8, d=4, l_sel=16, n_sel=4, w=16).eval()
        with pytest.raises(RuntimeError, match="does not match the input"):
            blk(x[:, :1], blk.attn.new_kv(5, 32, "cpu", torch.float32), prefill=False)
    assert m.get_fallback_counters()["total_fallbacks"] == 0  # refused before any native call: not a kernel failure


def test_tuning_switches_roundtrip():
    """nsa_hip_set_tuning / nsa_hip_get_tuning: process-wide A/B switches (nothing reads the environment per launch)"""
    from nsa_vibe_amd import _lib

    old = _lib.get_tuning("SEL_ROWS")
    try:
        _lib.set_tuning("NSA_HIP_SEL_ROWS", 3)
        assert _lib.get_tuning("sel_rows") == 3
    finally:
        _lib.set_tuning("SEL_ROWS", old)
    with pytest.raises(RuntimeError, match="unknown tuning switch"):
        _lib.set_tuning("NO_SUCH_SWITCH", 1)


def test_bench_gpus_flag_launches_the_ranks_itself():
    """`python bench.py --gpus 2` with no launcher environment must start two ranks: rehearsed on the CPU with
    --dry --backend gloo (rendezvous on 127.0.0.1, barrier, max-over-ranks timing, ONE JSON line from rank 0 with n_gpus = 2); a
    launcher that started a different number of ranks than --gpus says is refused"""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry", "--backend", "gloo", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["scaling"] == "weak" and rec["config"]["global_batch"] == 2 * 16
    # the line verifies itself: an all-reduce over the measurement's own process group counted the ranks
    rk = rec["ranks"]
    assert rk["ranks_seen"] == 2 and rk["backend"] == "gloo" and rk["rccl"] is False
    assert 0 < rk["ms_per_step_rank_min"] <= rk["ms_per_step_rank_max"] and abs(rk["ms_per_step_rank_max"] - rec["ms_per_step"]) < 1e-6
    env["WORLD_SIZE"] = "3"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry", "--backend", "gloo"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 2 and "refusing" in r.stderr
