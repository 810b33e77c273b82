"""Host only: the bookkeeping NSA_KV keeps for the rows a native call appends (begin_rows / end_rows, n_cmp_at, snapshot / restore, the native
descriptor), on a CPU-device cache.

tests/golden/kv_rows.json holds what NSAAttention._extend_begin / _extend_end -- the module methods these were before they moved to the cache
-- left for every (t0, S) of the table: a cache as a prefill of t0 tokens leaves it (capacity, metadata of t0 tokens, no read counters; t0 = 0:
a fresh cache), then begin, then end.  Geometry l 32, d 16, l_sel 64, n_sel 16, w 512; the cache starts with room for 16 tokens, so begin also
grows it."""
import json
import os

import pytest
import torch

from conftest import GOLDEN

READS = ("reads_pred", "reads_act_total", "reads_act_sel", "reads_act_cmp", "reads_act_win")
with open(os.path.join(GOLDEN, "kv_rows.json")) as _f:
    ROWS = json.load(_f)
GEO = ROWS["geometry"]


def cache(t0=0, S_max=16):
    from nsa_vibe_amd.kv_cache import NSA_KV

    kv = NSA_KV(1, 2, 8, 8, S_max, GEO["l"], GEO["d"], GEO["l_sel"], GEO["n_sel"], GEO["w"], "cpu", torch.float32)
    if t0:
        kv.ensure_capacity(t0)
        kv.ensure_meta(t0)
        kv.t, kv.n_cmp = t0, kv.n_cmp_at(t0)
    return kv


def state(kv):
    return {"t": kv.t, "n_cmp": kv.n_cmp, "meta_seq_len": kv.meta_seq_len, **{r: list(getattr(kv, r)) for r in READS}}


def test_the_table_is_the_issue_s():
    assert [(c["t0"], c["S"]) for c in ROWS["cases"]] == [(t0, S) for t0 in (0, 31, 32, 47, 63, 64, 100, 127) for S in (1, 2, 16)]


@pytest.mark.parametrize("c", ROWS["cases"], ids=lambda c: f"t0_{c['t0']}_S{c['S']}")
def test_begin_end_rows_leave_the_recorded_state(c):
    kv = cache(c["t0"])
    t0, meta = kv.begin_rows(c["S"])
    assert t0 == c["t0"] and meta is kv.meta
    assert {"meta_seq_len": kv.meta_seq_len, "S_sel": int(kv.meta.S_sel), "capacity": kv._K_sel.shape[2]} == c["after_begin"]
    kv.end_rows(t0, c["S"])
    assert state(kv) == {k: c[k] for k in ("t", "n_cmp", "meta_seq_len", *READS)}


def test_n_cmp_at_is_truncate_s_count():
    kv = cache(130, S_max=130)
    for t in range(130, -1, -1):
        kv.truncate(t)
        assert kv.n_cmp_at(t) == kv.n_cmp, t
    assert [kv.n_cmp_at(t) for t in (0, 31, 32, 47, 48, 130)] == [0, 0, 1, 1, 2, 7]


def test_snapshot_restore_round_trip():
    kv = cache(47)
    kv.end_rows(*kv.begin_rows(2)[:1], 2)
    before, saved = state(kv), kv.snapshot()
    t0, _ = kv.begin_rows(16)
    kv.end_rows(t0, 16)
    assert kv.t == 65 and len(kv.reads_pred) == 18
    kv.restore(saved)
    after = state(kv)
    assert after.pop("meta_seq_len") >= before.pop("meta_seq_len")  # the metadata stays: it covers more tokens than it has to
    assert after == before


def test_reserve_drops_the_cached_descriptor():
    kv = cache(10)
    d = kv.native_desc()
    assert kv.native_desc() is d and (d.B, d.S_max, d.n_cmp_max) == (1, 16, 1) and d.K_sel == kv._K_sel.data_ptr()
    kv._native["layer_decode"] = object()  # (what a single-step route keeps beside it)
    kv.reserve(40)
    assert not kv._native
    d2 = kv.native_desc()
    assert d2 is not d and (d2.S_max, d2.n_cmp_max) == (40, 1) and d2.K_sel == kv._K_sel.data_ptr() and d2.V_cmp == kv._V_cmp.data_ptr()


def test_a_shallow_copy_does_not_share_the_descriptor():
    """copy.copy(kv) followed by new buffers (what the GPU tests' clone helper does) must get a descriptor of ITS buffers"""
    import copy

    kv = cache(10)
    d = kv.native_desc()
    kv._native["layer_decode"] = object()
    c = copy.copy(kv)
    assert c._native == {} and kv.native_desc() is d and (c.t, c.meta) == (kv.t, kv.meta)
    c._K_sel = kv._K_sel.clone()
    assert c.native_desc().K_sel == c._K_sel.data_ptr() != d.K_sel
