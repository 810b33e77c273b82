"""GPU: the MFMA attention kernels that walk K/V in tiles (one-row, rows and block form of the selection forward with and without the fused
selector, band forward plain / split / inside the layer decode step, the dQ kernels of both backwards) reproduce, bit for bit, what they
computed before their K/V tile plumbing moved into attn_mfma_tiles.hpp.

tests/golden/attention_bits.npz holds the outputs of the case table of tests/attention_bits_probe.py (which documents the cases, the kernel
each one launches and the stored form), recorded on the MI355X from the library of the commit before the move; it was recorded twice and
holds the arrays on which both recordings agree (the probe names the others).  Every stored array must be reproduced exactly: there is no
tolerance."""
import os

import numpy as np
import pytest

import attention_bits_probe as probe

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "attention_bits.npz")


@pytest.mark.parametrize("group", list(probe.RUN))
def test_attention_outputs_equal_the_recorded_bits(group):
    want = {k: v for k, v in np.load(GOLDEN).items() if k.startswith(group + "/")}
    assert want, "the fixture has no case of this group"
    got = probe.Out()
    probe.RUN[group](got)
    assert sorted(got) == sorted(want)
    bad = [k for k in want if not (got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]
    assert not bad, f"{len(bad)} of {len(want)} outputs differ from the recorded bits: {bad[:8]}"
