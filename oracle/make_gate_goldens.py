#!/usr/bin/env python3
"""Golden vectors for the gate MLP + three-branch mix of the layer (g21), from the IMPORTED reference.

    python oracle/make_gate_goldens.py

The parity target is what the reference module runs by default: GateMLP.forward (nsa/core/nsa_attention.py:32-82, including the
"top-2 logit gap > 50 -> one-hot" rule) on q_gp = Q.mean(dim=3) of the post-RoPE Q, then the module's eager mix
O = g_cmp O_cmp + g_sel O_sel + g_win O_win (prefill :1380-1395; decode :931-950, q_gp = Q_t.mean(dim=2), the same expression on
[B,G,..] -- checked here to give the same bits).  The fused forms _fused_gate_combine_bsg / _bg (:85-124, run only under
NSA_GATE_COMPILE) lack the peaked rule: the script asserts they equal the eager mix on the non-peaked rows and stores their output, so the
difference on peaked rows is recorded, not guessed.

Inputs come from tests/golden_inputs.py (g21_inputs: PCG64, bf16-representable); the fixture holds outputs only, per case (fp32, CPU):
  gates [R,3], logits [R,3] (fc2 output / max(tau, 1e-6)) and the top-2 logit gap [R] of every row R = S G;
  for the first G21_RD rows: O, the fused forms' O, and the reference autograd gradients of the gate+mix expression for the seeded dO
  (dQ through the mean, dO_cmp, dO_sel, dO_win, dW1, db1, dW2, db2);
  m7c only: the same module in bf16 on CPU (gates_bf16 [R,3], O_bf16 for the dense rows) -- the rounding chain the kernels follow.
Asserts: the non-peaked cases are non-uniform (some row has max gate >= 0.7, some min gate <= 0.1, every branch wins some rows); the peaked
case has rows on both sides of the threshold; tau = 0 is clamped (every row one-hot).  The oracle gate (oracle/nsa_oracle.c) is checked
against every vector before saving.  Output: tests/golden/g21_gate.npz.
"""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("NSA_REFERENCE_ROOT", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
for k in ("NSA_FORCE_UNIFORM_GATE", "NSA_FORCE_BRANCH", "NSA_GATE_COMPILE", "NSA_STOPGRAD_GATES"):
    os.environ.pop(k, None)

import torch  # noqa: E402

import golden_inputs as gi  # noqa: E402
from nsa.core.nsa_attention import GateMLP, _fused_gate_combine_bg, _fused_gate_combine_bsg  # noqa: E402

from oracle import nsa_oracle as orc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g21_gate.npz")


def gate_module(x, dtype):
    torch.manual_seed(0)
    g = GateMLP(x["Dk"], x["Hd"])
    with torch.no_grad():
        for p, k in ((g.fc1.weight, "w1"), (g.fc1.bias, "b1"), (g.fc2.weight, "w2"), (g.fc2.bias, "b2")):
            p.copy_(torch.from_numpy(x[k]))
    return g.to(dtype)


def prefill_mix(gate, Q, Oc, Os, Ow, tau):
    """the module's prefill gate + mix (nsa_attention.py:1380-1395, the NSA_GATE_COMPILE=0 branch)"""
    B, S, G = Q.shape[:3]
    q_gp = Q.mean(dim=3)  # [B,S,G,Dk]
    gates = gate(q_gp.reshape(B * S * G, q_gp.shape[-1]), tau=tau).view(B, S, G, 3)
    w_cmp, w_sel, w_win = gates[..., 0:1].unsqueeze(3), gates[..., 1:2].unsqueeze(3), gates[..., 2:3].unsqueeze(3)
    return w_cmp * Oc + w_sel * Os + w_win * Ow, gates


def decode_mix(gate, Q_t, Oc, Os, Ow, tau):
    """the module's decode gate + mix (nsa_attention.py:931-950): Q_t [B,G,h,Dk]"""
    q_gp = Q_t.mean(dim=2, dtype=Q_t.dtype)
    gates = gate(q_gp, tau=tau)
    w_cmp, w_sel, w_win = gates[..., 0:1].unsqueeze(-1), gates[..., 1:2].unsqueeze(-1), gates[..., 2:3].unsqueeze(-1)
    return w_cmp * Oc + w_sel * Os + w_win * Ow, gates


def logits_of(gate, Q, tau):
    with torch.no_grad():
        q = Q.mean(dim=3).reshape(-1, Q.shape[-1])
        return gate.fc2(torch.nn.functional.silu(gate.fc1(q))) / max(tau, 1e-6)


store = {}
RD = gi.G21_RD
for case in gi.G21_CASES:
    x = gi.g21_inputs(case)
    tau, h, Dk, Dv = x["tau"], x["h"], x["Dk"], x["Dv"]
    gate = gate_module(x, torch.float32)
    tQ, tOc, tOs, tOw, tdO = (torch.from_numpy(x[k]) for k in ("Q", "O_cmp", "O_sel", "O_win", "dO"))
    with torch.no_grad():
        O_all, gates = prefill_mix(gate, tQ, tOc, tOs, tOw, tau)
        # decode form: the S tokens as a batch of single-token steps -> the same bits
        O_dec, gates_dec = decode_mix(gate, tQ[0], tOc[0], tOs[0], tOw[0], tau)
        assert torch.equal(gates_dec.reshape(-1, 3), gates.reshape(-1, 3)) and torch.equal(O_dec, O_all[0]), case
    gates = gates.reshape(-1, 3).numpy()
    lg = logits_of(gate, tQ, tau)
    top2 = torch.topk(lg, k=2, dim=-1).values
    gap = (top2[:, 0] - top2[:, 1]).numpy()
    peaked = gap > 50.0
    # fused forms (no peaked rule): equal to the eager mix on the non-peaked rows
    with torch.no_grad():
        args = (gate.fc1.weight, gate.fc1.bias, gate.fc2.weight, gate.fc2.bias, float(tau))
        Ob = _fused_gate_combine_bsg(tQ.mean(dim=3), tOc, tOs, tOw, *args)
        Obg = _fused_gate_combine_bg(tQ[0].mean(dim=2), tOc[0], tOs[0], tOw[0], *args)
    Ob_rows, O_rows = Ob.reshape(-1, h, Dv).numpy(), O_all.reshape(-1, h, Dv).numpy()
    fused_err = float(np.abs(Ob_rows - O_rows)[~peaked].max()) if (~peaked).any() else 0.0
    assert fused_err <= 1e-6, (case, fused_err)
    assert torch.equal(Obg, Ob[0]), case
    fused_peaked_diff = float(np.abs(Ob_rows - O_rows)[peaked].max()) if peaked.any() else 0.0

    R = gates.shape[0]
    if case == "peaked":
        assert 0.2 < peaked.mean() < 0.8, peaked.mean()  # rows on both sides of the threshold
        assert (np.abs(gap - 50.0) > 1e-3).all()  # no row is decided by rounding
    elif case == "clamp":
        assert peaked.all()  # tau = 0 -> max(tau, 1e-6): logits x 1e6, every row one-hot
    else:
        assert not peaked.any(), case
        assert gates.max(1).max() >= 0.7 and gates.min(1).min() <= 0.1, (case, gates.max(1).max(), gates.min(1).min())
        wins = np.bincount(gates.argmax(1), minlength=3)
        assert (wins > 0).all(), (case, wins)
        assert gates.max(1).mean() < 0.9, case  # not saturated

    # autograd gradients of the module's expression on the dense rows (the first RD rows = RD / G tokens)
    n_tok = RD // gi.G21_G
    ins = [t[:, :n_tok].clone().requires_grad_(True) for t in (tQ, tOc, tOs, tOw)]
    O_d, _ = prefill_mix(gate, *ins, tau)
    gate.zero_grad()
    (O_d * tdO[:, :n_tok]).sum().backward()
    assert (O_d.detach() - O_all[:, :n_tok]).abs().max().item() <= 1e-6  # (the GEMMs of another row count: not always the same bits)
    pre = f"{case}_"
    store.update({pre + "gates": gates, pre + "logits": lg.numpy(), pre + "gap": gap.astype(np.float32),
                  pre + "O": O_rows[:RD], pre + "dQ": ins[0].grad.reshape(RD, h, Dk).numpy(),
                  pre + "dO_cmp": ins[1].grad.reshape(RD, h, Dv).numpy(), pre + "dO_sel": ins[2].grad.reshape(RD, h, Dv).numpy(),
                  pre + "dO_win": ins[3].grad.reshape(RD, h, Dv).numpy(), pre + "dW1": gate.fc1.weight.grad.numpy(),
                  pre + "db1": gate.fc1.bias.grad.numpy(), pre + "dW2": gate.fc2.weight.grad.numpy(), pre + "db2": gate.fc2.bias.grad.numpy()})
    if case in ("m7c", "peaked"):
        store[pre + "O_fused_bsg"] = Ob_rows[:RD]
    if case == "m7c":
        gb = gate_module(x, torch.bfloat16)
        with torch.no_grad():
            Obf, gbf = prefill_mix(gb, *(t.bfloat16() for t in (tQ, tOc, tOs, tOw)), tau)
        store[pre + "gates_bf16"] = gbf.float().reshape(-1, 3).numpy()
        store[pre + "O_bf16"] = Obf.float().reshape(-1, h, Dv)[:RD].numpy()
        print(f"  bf16 run: max|gates_bf16 - gates| = {np.abs(store[pre + 'gates_bf16'] - gates).max():.3e}")

    # the oracle against this case before saving
    q2 = x["Q"].reshape(R, h, Dk)
    o2 = [x[k].reshape(R, h, Dv) for k in ("O_cmp", "O_sel", "O_win")]
    og, oO = orc.gate_combine(q2, *o2, x["w1"], x["b1"], x["w2"], x["b2"], tau)
    eg, eO = float(np.abs(og - gates).max()), float(np.abs(oO[:RD] - O_rows[:RD]).max())
    bw = orc.gate_combine_bwd(q2[:RD], *(o[:RD] for o in o2), x["w1"], x["b1"], x["w2"], x["b2"], tau, x["dO"].reshape(R, h, Dv)[:RD])
    ref_g = {k: store[pre + k] for k in ("dQ", "dO_cmp", "dO_sel", "dO_win", "dW1", "db1", "dW2", "db2")}
    egr = {k: float(np.abs(bw[k] - v).max() / max(1.0, np.abs(v).max())) for k, v in ref_g.items()}
    print(f"g21 {case}: R={R} peaked={int(peaked.sum())} gates [{gates.min():.3f}, {gates.max():.3f}] wins={np.bincount(gates.argmax(1), minlength=3)}"
          f"  |fused-eager| non-peaked {fused_err:.1e} peaked {fused_peaked_diff:.2e}  oracle: gates {eg:.1e} O {eO:.1e} grads {max(egr.values()):.1e}")
    assert eg <= 1e-6 and eO <= 1e-5 * max(1.0, float(np.abs(O_rows).max())) and max(egr.values()) <= 1e-5, (case, eg, eO, egr)

# a deflated .npz written with fixed zip timestamps, so a rerun reproduces the file bit for bit (np.savez stamps the current time)
with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_DEFLATED) as zf:
    for k in sorted(store):
        info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        with zf.open(info, "w", force_zip64=True) as f:
            np.lib.format.write_array(f, np.ascontiguousarray(store[k]), allow_pickle=False)
print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
