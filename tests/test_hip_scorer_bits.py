"""GPU: the two fused MFMA selection scorers (16x16x32 tiles in every group size and the FLAT layout, 32x32x16 tiles with and without the
top-n selector in the launch) reproduce, bit for bit, what they computed before their K_cmp staging, sweep bounds and exact sweep-1 update
moved into sel_scores_mfma.hpp.

tests/golden/scorer_bits.npz holds the outputs of the case table of tests/scorer_bits_probe.py (which documents the cases, the kernel each
one launches and the stored form), recorded on the MI355X from the library of the commit before the move; it was recorded twice and holds
the arrays on which both recordings agree (all of them: the scorers have no atomics).  Every stored array must be reproduced exactly: there
is no tolerance."""
import os

import numpy as np
import pytest

import scorer_bits_probe as probe

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "scorer_bits.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("group", list(probe.RUN))
def test_scorer_outputs_equal_the_recorded_bits(group, golden):
    want = {k: v for k, v in golden.items() if k.startswith(group + "/")}
    assert want, "the fixture has no case of this group"
    got = probe.Out()
    probe.RUN[group](got)
    assert sorted(got) == sorted(want)
    bad = [k for k in want if not (got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]
    assert not bad, f"{len(bad)} of {len(want)} outputs differ from the recorded bits: {bad[:8]}"
