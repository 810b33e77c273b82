"""GPU: the Python package asks of the native library what it asked before its host idioms and cache bookkeeping were folded, and gets the
same bits.  tests/native_call_probe.py replays its scenarios (every module route, the declined one-call entry points, parity mode, a training
step, block, model, the operators) on the package as it is; tests/golden/python_call_trace.json is that probe's record of the package before
the fold (two recordings: the traces agreed, and so did every hash, the gradients included).

Per scenario: every call that can launch or write equals the record, argument by argument; on the one-call routes the pure queries
(workspace sizes, plans, nsa_batched_ranges_width, tuning getters) do too, on the per-stage routes they may differ in number and are printed;
every output and the cache state (t, n_cmp, the read lists, meta_seq_len, the eight buffers up to t / n_cmp) has the recorded SHA-256."""
import json
import os

import pytest

import native_call_probe as ncp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "python_call_trace.json")) as _f:
    RECORD = json.load(_f)
_RUN = {}


def replay():
    if not _RUN:
        _RUN.update(json.loads(json.dumps(ncp.run_all())))  # (through JSON, as the record went: tuples become lists)
    return _RUN


def difference(got, want):
    """the first place two call lists part, in words"""
    for i, (g, w) in enumerate(zip(got, want)):
        if g[0] != w[0] or len(g) != len(w):
            return f"call {i}: {g[0]}{g[2:]} instead of {w[0]}{w[2:]}"
        for j, (a, b) in enumerate(zip(g[1], w[1])):
            if a != b:
                return f"call {i} ({g[0]}), argument {j}: {a!r} instead of {b!r}"
    return None if len(got) == len(want) else f"{len(got)} calls instead of {len(want)}: {[c[0] for c in got]} / {[c[0] for c in want]}"


def test_every_scenario_ran():
    assert list(replay()) == list(RECORD)


@pytest.mark.parametrize("name", list(RECORD))
def test_calls_match_the_record(name):
    got, want = replay()[name], RECORD[name]
    assert difference(ncp.launches(got["calls"]), ncp.launches(want["calls"])) is None
    if want["one_call"]:
        assert difference(got["calls"], want["calls"]) is None
    elif got["calls"] != want["calls"]:
        print(f"{name}: pure queries {[c[0] for c in got['calls'] if ncp.is_query(c[0])]}, recorded {[c[0] for c in want['calls'] if ncp.is_query(c[0])]}")


@pytest.mark.parametrize("name", list(RECORD))
def test_outputs_and_cache_state_match_the_record(name):
    got, want = replay()[name]["hashes"], RECORD[name]["hashes"]
    assert got.keys() == want.keys()
    assert {k: v for k, v in got.items() if v != want[k]} == {}
