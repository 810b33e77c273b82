"""GPU parity: the long-row form (switch DECODE_LONG = 1, plan form 3) of the ragged decode step over PAGED caches, rows of up to 128
chunks -- table entries up to index 127, lanes L and L + 64 of the kernel's table check.

As in tests/test_hip_decode_paged.py the specification is an equality: for a table that scatters contiguous caches into pool pages in a
random order, ranges and O are those of the long ragged call on the contiguous caches bit for bit (that call is pinned to single steps by
tests/test_hip_decode_long.py).  Pools are poisoned (+-3e4) wherever nobody's tokens lie, and the table entries nobody needs point at a
valid, poisoned page."""
import pytest
import torch

from test_hip_decode_long import CASES
from test_hip_decode_paged import paged, pools_of, ragged_ref
from test_hip_decode_ragged import G, N_TOP, make_case
from test_hip_decode_ragged import plan as ragged_plan
from test_hip_selection import nv  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,waves", [("d128_S1", None), ("d128_128_chunks", None), ("d64_S1", None), ("d64_S3", None), ("d64_waves8", 8)])
def test_long_paged_equals_long_ragged_bit_for_bit(nv, tune, name, waves):
    tune("DECODE_LONG", 1)
    if waves:
        tune("DECODE_WAVES", waves)
    c = make_case(nv, **CASES[name])
    pl = pools_of(c)
    m = c["meta"]
    p = nv.selection_decode_paged_plan(c["B"], c["S"], G, c["h"], c["D"], c["D"], m.S_cmp, m.S_sel, pl["max_pages"], N_TOP, c["t_max"], c["dtype"])
    assert p == {"launches": 1, "form": 3} == ragged_plan(nv, c), p
    O, rg = paged(nv, c, pl)
    O1, r1 = ragged_ref(nv, c)  # (the 8-wave case is only ever run at DECODE_WAVES = 8: its cached reference is the 8-wave call)
    torch.cuda.synchronize()
    assert torch.isfinite(O.float()).all()
    assert torch.equal(rg, r1)
    assert torch.equal(O, O1)


def test_bad_table_entry_at_an_index_beyond_63(nv, tune):
    """entry 100 of the sequence at 131,069 (it needs entries 0 .. 127) outside [0, n_pages): that sequence is inactive -- zero O and ranges
    rows -- and the others keep their bits; the same bad values BEHIND the last needed entry of a sequence leave it live"""
    tune("DECODE_LONG", 1)
    c = make_case(nv, **CASES["d64_S1"])
    pl = pools_of(c)
    O1, r1 = ragged_ref(nv, c)
    b_long = c["t_pos"].index(131069)
    assert pl["max_pages"] == 129
    for bad in (pl["n_pages"], -1):
        table = [row[:] for row in pl["table"]]
        table[b_long][100] = bad
        table[b_long][128] = bad                             # behind its last needed entry (127)
        table[0][65566 // 1024 + 1] = bad                    # behind the last needed entry of the sequence at 65,566 (64)
        O, rg = paged(nv, c, pl, table=table)
        torch.cuda.synchronize()
        assert not O[b_long].any() and not rg[b_long].any(), bad
        for b in range(c["B"]):
            if b != b_long:
                assert torch.equal(O[b], O1[b]) and torch.equal(rg[b], r1[b]), (bad, b)
        table[b_long][100] = pl["table"][b_long][100]        # only the entries nobody needs are bad: every sequence is live
        O, rg = paged(nv, c, pl, table=table)
        torch.cuda.synchronize()
        assert torch.equal(O, O1) and torch.equal(rg, r1), bad
