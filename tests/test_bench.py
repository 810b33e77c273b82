"""bench.py's result line and --dump-outputs: the dump helper and the argument checks on the CPU, a plain run of the hot path on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _bench_env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("rows", "ranges", "O")}


def test_dump_outputs_writes_a_fixed_sample_of_the_step_outputs(tmp_path, monkeypatch):
    """rows / ranges / O as float64 / float64 / float32, the values of the sampled rows exactly, the same sample every time; at the
    headline shape (B = 16, S = 65536, m7c) the files stay under 64 MiB"""
    import bench

    B, S = 2, 300
    g = torch.Generator().manual_seed(0)
    ranges = torch.randint(0, S, (B, S, bench.G, bench.N_SEL, 2), generator=g, dtype=torch.int32)
    O = torch.randn(B, S, bench.G, bench.H, bench.D, generator=g).bfloat16()
    monkeypatch.setattr(bench, "DUMP_ROWS", 64)
    bench.dump_outputs(str(tmp_path / "a"), ranges, O)
    bench.dump_outputs(str(tmp_path / "b"), ranges, O)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a["rows"].dtype == a["ranges"].dtype == np.float64 and a["O"].dtype == np.float32
    rows = a["rows"].astype(np.int64)
    assert rows.size == 64 and np.all(np.diff(rows) > 0) and rows[-1] < B * S
    assert np.array_equal(a["ranges"], ranges.reshape(B * S, bench.G, bench.N_SEL, 2)[rows].numpy())
    assert np.array_equal(a["O"], O.float().reshape(B * S, bench.G, bench.H, bench.D)[rows].numpy())
    for n in a:
        assert np.array_equal(a[n], b[n])
    monkeypatch.undo()
    per_row = bench.G * bench.H * bench.D * 4 + bench.G * bench.N_SEL * 2 * 8 + 8
    assert bench.DUMP_ROWS <= 16 * 65536 and bench.DUMP_ROWS * per_row <= 64 * 2 ** 20


def test_bench_refuses_arguments_it_cannot_honour():
    """--steps below 1 has no step to time; --dump-outputs names outputs of the hot path, which --dry does not run"""
    for extra in (["--steps", "0"], ["--dry", "--backend", "gloo", "--dump-outputs", "unused"]):
        r = subprocess.run([sys.executable, BENCH] + extra, capture_output=True, text=True, env=_bench_env(), timeout=120)
        assert r.returncode == 2 and "error" in r.stderr, (extra, r.stderr[-2000:])


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_it_is_given_and_dumps_them(tmp_path):
    """a plain run prints the headline fields only (no stage / roofline / extra runs) with steps = --steps, and two runs with the same
    arguments dump the same outputs"""
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--seq", "4096", "--batch", "2"]
    recs = []
    for d in ("a", "b"):
        r = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, env=_bench_env(), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        recs.append(json.loads(lines[0]))
    for rec in recs:
        assert rec["metric"] == "sel_branch_hot_path_prefill_tok_per_s" and rec["unit"] == "tok/s" and rec["higher_is_better"] is True
        assert rec["dtype"] == "bf16" and rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
        assert rec["value"] == pytest.approx(2 * 4096 / (rec["ms_per_step"] * 1e-3))
        assert not {"stages_ms", "roofline", "extra", "cpu_baseline"} & set(rec)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a["rows"].size == 2 * 4096 and a["O"].shape == (2 * 4096, 2, 6, 64) and a["ranges"].shape == (2 * 4096, 2, 16, 2)
    assert np.isfinite(a["O"]).all()
    for n in a:
        assert np.array_equal(a[n], b[n]), n
