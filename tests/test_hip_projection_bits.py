"""GPU: the few-row projection kernels (chunk-loop and all-loads-first templates, every A-operand and epilogue policy), the MFMA form's
RoPE epilogue and the prefill RoPE column map forward and back reproduce, bit for bit, what the kernels they were folded from computed.

tests/golden/projection_bits.npz holds the outputs of the case table of tests/projection_bits_probe.py (which documents the cases and the
stored form), recorded once on the MI355X from the library of the commit before the fold; two recordings were identical.  These kernels
have no atomics and a fixed summation order, so every stored array must be reproduced exactly: there is no tolerance."""
import os

import numpy as np
import pytest

import projection_bits_probe as probe

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "projection_bits.npz")
GROUPS = {"linear": probe.run_linear, "rope": probe.run_rope, "qkv": probe.run_qkv, "model": probe.run_model}


@pytest.mark.parametrize("group", list(GROUPS))
def test_projection_outputs_equal_the_recorded_bits(group):
    want = {k: v for k, v in np.load(GOLDEN).items() if k.startswith(group + "/")}
    assert want, "the fixture has no case of this group"
    got = probe.Out()
    GROUPS[group](got)
    assert sorted(got) == sorted(want)
    bad = [k for k in want if not (got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]
    assert not bad, f"{len(bad)} of {len(want)} outputs differ from the recorded bits: {bad[:8]}"
