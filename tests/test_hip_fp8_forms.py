"""Every FP8 (e4m3 K/V) instantiation that tests/test_hip_decode_fp8.py and tests/test_hip_band_fp8.py do not launch, or launch only against
itself, compared with plain float64 attention at general scales -- the table in DESIGN.md (4.1m) names the test id behind each of the 20
decode-step and 12 band kernels.

Decode step (dstep_kernel_fp8: (NW, CPW, D) x HC x ragged / paged): the cases below reach (16,4,64) HC 0, (8,2,64) HC 0, (8,4,64) HC 6 and 0
and (8,2,128) HC 0; the eight-wave kernels at fewer than 257 rows through DECODE_WAVES = 8, which the plan reads as the launch does.
Band (band_attn_fwd_fp8_kernel<D, NT, SPLIT, PAGED>): the unsplit NT = 1 and NT = 3 / 2 forms at general scales.

Inputs, poison (+-448 at scale 64 behind each sequence's own rows) and the general scales (per-row powers of two that cannot cancel) are those
of the two files above; the bounds are theirs too."""
import pytest
import torch

import test_hip_band_fp8 as bf8
from test_hip_band_paged import BANDS, PAGE, key_rows, workspace_bytes
from test_hip_decode_fp8 import fp8_case, fp8_pools, ragged8, worst_error
from test_hip_decode_paged import paged
from test_hip_decode_ragged import G, N_TOP, ragged
from test_hip_selection import nv  # noqa: F401

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
_S1 = [1055, 40, 9, 4100, -1]
# id: (case, DECODE_WAVES or None, the form the plan must give, the kernel reached)
DECODE = {
    "form1_h4": (dict(t_pos=[32796, 100], S=8, h=4), None, 1, "(16,4,64) HC 0"),          # 2049 compressed tokens: 33 chunks > 2 * 16
    "waves8_h4": (dict(t_pos=_S1, S=1, h=4), 8, 0, "(8,2,64) HC 0"),
    "waves8_h16": (dict(t_pos=_S1, S=1, h=16), 8, 0, "(8,2,64) HC 0, all 16 slots"),
    "waves8_form1": (dict(t_pos=[17000, 100], S=2), 8, 1, "(8,4,64) HC 6"),                 # t = 17001: 1061 compressed tokens = 17 chunks, 2 * 8 < 17 <= 4 * 8
    "waves8_form1_h4": (dict(t_pos=[17000, 100], S=2, h=4), 8, 1, "(8,4,64) HC 0"),
    "d128_h4": (dict(t_pos=[1052, 40, 9000], S=4, D=128, h=4), None, 0, "(8,2,128) HC 0"),   # t = 9003: 561 compressed tokens = 9 chunks <= 2 * 8
}


def decode_case(nv, tune, name):
    """the case with its switch set for the test, and the plan asserted before anything is launched: one launch in the expected form"""
    case, waves, form, _ = DECODE[name]
    if waves is not None:
        tune("DECODE_WAVES", waves)
    c, f = fp8_case(nv, case)
    m = c["meta"]
    p = nv.selection_decode_ragged_fp8_plan(c["B"], c["S"], G, c["h"], c["D"], c["D"], m.S_cmp, m.S_sel, c["K"].shape[2], N_TOP, c["t_max"])
    assert p == {"launches": 1, "form": form}, (name, p)
    assert c["B"] * c["S"] * G <= 256  # (below the row count that selects eight waves by itself: the switch, or D = 128, does)
    return c, f


@pytest.mark.parametrize("name", list(DECODE))
def test_decode_general_scales_against_float64(nv, tune, name):
    """O against plain float64 softmax attention over the call's own ranges on K^ = K8 * k_scale, V^ = V8 * v_scale: 1e-2 absolute, the project's
    bf16 bound on unit-normal data (tests/test_hip_decode_fp8.py keeps K^, V^ unit normal by construction).  Ranges are the bf16 call's;
    inactive slots give zero rows (worst_error asserts it); scales behind each sequence's tokens set to inf change no bit."""
    c, f = decode_case(nv, tune, name)
    O, rg = ragged8(nv, c, f, f["ks"], f["vs"])
    assert O.dtype == BF16 and torch.isfinite(O.float()).all()
    assert torch.equal(rg, ragged(nv, c)[1])
    worst = worst_error(c, O, rg, f["K8"].double() * f["ks"].double()[..., None], f["V8"].double() * f["vs"].double()[..., None])
    print(f"decode fp8 {name} [{DECODE[name][3]}]: worst |O - float64| = {worst:.3e}")
    assert worst <= 1e-2
    ki, vi = f["ks"].clone(), f["vs"].clone()
    for b, t0 in enumerate(c["t_pos"]):
        ki[b, :, max(t0 + c["S"], 0):] = vi[b, :, max(t0 + c["S"], 0):] = float("inf")
    assert torch.equal(ragged8(nv, c, f, ki, vi)[0], O)


@pytest.mark.parametrize("name", list(DECODE))
def test_decode_paged_is_the_ragged_call_bit_for_bit(nv, tune, name):
    """pools behind a permuted table, general scales: O and ranges torch.equal with the FP8 ragged call, under the same switch"""
    c, f = decode_case(nv, tune, name)
    pl, zk, zv = fp8_pools(c, f, f["ks"], f["vs"])
    m = c["meta"]
    p = nv.selection_decode_paged_plan(c["B"], c["S"], G, c["h"], c["D"], c["D"], m.S_cmp, m.S_sel, pl["max_pages"], N_TOP, c["t_max"])
    assert p == {"launches": 1, "form": DECODE[name][2]}, p
    O, rg = paged(nv, c, pl, k_scale_pool=zk, v_scale_pool=zv)
    O1, r1 = ragged8(nv, c, f, f["ks"], f["vs"])
    assert torch.equal(rg, r1) and torch.equal(O, O1)


@pytest.mark.parametrize("name", list(DECODE))
def test_decode_unit_scales_are_the_bf16_call_bit_for_bit(nv, tune, name):
    """all scales 1.0f: O and ranges torch.equal with selection_decode_ragged on the dequantised caches, under the same switch"""
    c, f = decode_case(nv, tune, name)
    O, rg = ragged8(nv, c, f, f["one"], f["one"])
    O1, r1 = ragged(nv, f["deq"])
    assert torch.isfinite(O.float()).all()
    assert torch.equal(rg, r1) and torch.equal(O, O1)


# ---- band branches: the unsplit forms ---------------------------------------------------------------------------------------------------

def float64_rows(c, Q, Kh, Vh, branch):
    """bf8.float64_ref with the rows of a sequence in one masked einsum (S = 256, B = 32 is too slow row by row): plain float64 softmax
    attention of EVERY row (b, s) over its own [lo, hi) on Kh, Vh [B,G,n,D] -> O, lse (zeros / -inf for an empty interval)"""
    band, D, S = BANDS[branch], Q.shape[-1], c["S"]
    O = torch.zeros(Q.shape, dtype=torch.float64, device="cuda")
    lse = torch.full(Q.shape[:-1], -float("inf"), dtype=torch.float64, device="cuda")
    for b, t0 in enumerate(c["t_pos"]):
        if t0 < 0:
            continue
        hi = torch.tensor([key_rows(band, t0 + s, 1)[1] for s in range(S)], device="cuda")
        lo = (hi - band["w"]).clamp(min=0)
        n = int(hi.max())
        if n == 0:
            continue
        k = torch.arange(n, device="cuda")
        keep = (k[None] >= lo[:, None]) & (k[None] < hi[:, None])  # [S, n]
        x = torch.einsum("sghd,gkd->sghk", Q[b].double(), Kh[b, :, :n]) * D ** -0.5
        x = x.masked_fill(~keep[:, None, None], -float("inf"))
        live = hi > lo
        l = torch.logsumexp(x[live], -1)
        lse[b, live] = l
        O[b, live] = torch.einsum("sghk,gkd->sghd", torch.exp(x[live] - l[..., None]), Vh[b, :, :n])
    return O, lse


def test_float64_rows_is_float64_ref(nv):
    """the vectorised reference against the row-by-row one of tests/test_hip_band_fp8.py, on a case small enough for both"""
    c, Q = bf8.get_case("set", "S3_boundaries", 64)
    for branch in bf8.BRANCHES:
        f = bf8.fp8_case(c, branch)
        Kh, Vh = f["K8"].double() * f["ks"].double()[..., None], f["V8"].double() * f["vs"].double()[..., None]
        a, b = float64_rows(c, Q, Kh, Vh, branch), bf8.float64_ref(c, Q, Kh, Vh, branch)
        assert torch.equal(torch.isfinite(a[1]), torch.isfinite(b[1]))
        live = torch.isfinite(b[1])
        assert (a[0] - b[0]).abs().max().item() <= 1e-12 and (a[1] - b[1])[live].abs().max().item() <= 1e-12


UNSPLIT = [(32, 64), (32, 128), (256, 64), (256, 128)]  # S = 32: unsplit NT = 1; S = 256: NT = 3 (D = 64) / 2 (D = 128)


@pytest.mark.parametrize("branch", bf8.BRANCHES)
@pytest.mark.parametrize("S,D", UNSPLIT)
def test_band_unsplit_general_scales_against_float64(nv, S, D, branch):
    """the unsplit kernels at general scales, every row of the call: O within 1e-2 of float64 on K^ = K8 * k_scale, V^ = V8 * v_scale; lse
    within twice the bf16 call's worst on the dequantised caches + 1e-5 (bound and derivation: test_general_scales_against_float64 of
    tests/test_hip_band_fp8.py); inf scales behind each sequence's keys change no bit"""
    assert workspace_bytes(nv, 32, S, D) == 0  # unsplit
    c, Q = bf8.get_case("unsplit", S, D)
    f = bf8.fp8_case(c, branch)
    got = bf8.call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=f["ks"], v_scale=f["vs"])
    Kh, Vh = f["K8"].double() * f["ks"].double()[..., None], f["V8"].double() * f["vs"].double()[..., None]
    dO, dl = bf8.worst(got, float64_rows(c, Q, Kh, Vh, branch))
    Kb, Vb = Kh.to(BF16), Vh.to(BF16)  # beside it: the bf16 call on the dequantised caches against float64 on those
    dO16, dl16 = bf8.worst(bf8.call(nv, c, Q, Kb, Vb, branch), float64_rows(c, Q, Kb.double(), Vb.double(), branch))
    print(f"band fp8 unsplit {branch} S={S} D={D}: worst |dO| {dO:.3e} (bf16 call {dO16:.3e}), worst |dlse| {dl:.3e} (bf16 call {dl16:.3e})")
    assert dO <= 1e-2
    assert dl <= 2 * dl16 + 1e-5
    ki, vi = f["ks"].clone(), f["vs"].clone()
    for b in range(c["B"]):
        ki[b, :, bf8.own_rows(c, branch, b):] = vi[b, :, bf8.own_rows(c, branch, b):] = float("inf")
    bf8.assert_equal_bits(bf8.call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=ki, v_scale=vi), got)


@pytest.mark.parametrize("branch", bf8.BRANCHES)
@pytest.mark.parametrize("S,D", [(32, 64), (32, 128), (256, 128)])
def test_band_unsplit_paged_is_ragged_bit_for_bit(nv, S, D, branch):
    """general scales behind a permuted table, the unsplit combinations tests/test_hip_band_fp8.py leaves out (it has S = 256 at D = 64)"""
    assert workspace_bytes(nv, 32, S, D) == 0
    c, Q = bf8.get_case("unsplit", S, D)
    f = bf8.fp8_case(c, branch)
    pl = bf8.fp8_pools(c, f, branch, PAGE[branch])
    bf8.assert_equal_bits(bf8.paged8(nv, c, Q, pl, branch), bf8.call(nv, c, Q, f["K8"], f["V8"], branch, k_scale=f["ks"], v_scale=f["vs"]))
