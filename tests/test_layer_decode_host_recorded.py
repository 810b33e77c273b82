"""Host side of the layer decode family against its recorded results (no GPU).

`dispatch_check <library> layer_ragged | layer_paged | decode_long` (csrc/dispatch_check.cpp: the library's host code against a HIP runtime
that counts and refuses every launch) prints, for every case of nsa_layer_decode_ragged and nsa_layer_decode_paged, the launchers in order,
their geometry, the argument blocks of the launches that depend on the positions, the plan's answer, every decline with its message -- with
two defects at once: the message that wins -- and the tail of every call that runs: the finish (or gate) block and the output projection,
member by member.  tests/golden/layer_decode_host_{ragged,paged,long}.json hold these outputs as the library printed them before the
family's host code was folded onto one plan and one body; the code as it stands must print the same, member for member."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

MODES = {"layer_ragged": "ragged", "layer_paged": "paged", "decode_long": "long"}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_host_route_is_the_recorded_one(mode):
    from nsa_vibe_amd import _lib

    env = {k: v for k, v in os.environ.items() if not k.startswith("NSA_HIP_")}
    r = subprocess.run([os.path.join(ROOT, "nsa_vibe_amd", "dispatch_check"), _lib.LIB_PATH, mode], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    with open(os.path.join(ROOT, "tests", "golden", f"layer_decode_host_{MODES[mode]}.json")) as f:
        want = json.load(f)
    differ = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    for k in differ[:8]:
        print(f"{k}:\n  recorded {json.dumps(want.get(k))}\n  got      {json.dumps(got.get(k))}")
    assert not differ, f"{len(differ)} of {len(want)} records differ from the recorded ones: {differ}"
    assert any(k.endswith("_tail") for k in got)
