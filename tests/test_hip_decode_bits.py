"""GPU: the one-launch decode step of the selected branch (decode_step_kernel in every form -- unsplit, team, four chunks per wave, rows,
ragged, paged, long-row -- decode_step_onepass_kernel and the band workgroups of a layer step) reproduces, bit for bit, what it computed
before the two kernel templates' shared phases and the launchers' kernel table were written once.

tests/golden/decode_step_bits.npz holds the outputs of the case table of tests/decode_bits_probe.py (which documents the cases, the form
each one must be planned in and the stored form), recorded on the MI355X from the library of the commit before the fold; it was recorded
twice and holds the arrays on which both recordings agree (all of them).  Every stored array must be reproduced exactly: there is no
tolerance."""
import os

import numpy as np
import pytest

import decode_bits_probe as probe

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "decode_step_bits.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("group", list(probe.RUN))
def test_decode_outputs_equal_the_recorded_bits(group, golden):
    want = {k: v for k, v in golden.items() if k.startswith(group + "/")}
    assert want, "the fixture has no case of this group"
    got = probe.Out()
    probe.RUN[group](got)
    assert sorted(got) == sorted(want)
    bad = [k for k in want if not (got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]
    assert not bad, f"{len(bad)} of {len(want)} outputs differ from the recorded bits: {bad[:8]}"
