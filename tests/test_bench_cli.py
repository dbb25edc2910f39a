"""bench.py's command line: what a plain run prints and what --dump-outputs writes.

A plain run times exactly --steps steps in one block and prints only the headline line (the
probes, whole solves and CPU baseline are --full's); --dump-outputs writes the last timed step's
outputs as float64 .npy files, at most bench.DUMP_LIMIT_BYTES, a seeded sample of the problems
when a batch is larger than that."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


class _FakeSystem:
    """The three reads dump_outputs makes of a System, for B problems."""

    def __init__(self, B, n, mi):
        rng = np.random.default_rng(1)
        self.vec = {"p": rng.standard_normal((B, n)), "p_s": rng.standard_normal((B, mi)),
                    "p_z": rng.standard_normal((B, mi))}
        self.reg = rng.standard_normal((B, 2))

    def get(self, which):
        return self.vec[which]

    def regularization(self):
        return self.reg


def test_dump_outputs_keeps_every_problem_under_the_limit(tmp_path):
    import bench

    B, n, mi = 3, 7, 4
    fake = _FakeSystem(B, n, mi)
    bench.dump_outputs(tmp_path, fake, [5, 6, 7], np.array([0, 1, 0], dtype=np.int32))
    out = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert set(out) == {"p", "p_s", "p_z", "regularization", "status", "problem_ids"}
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["p"], fake.vec["p"]) and np.array_equal(out["regularization"], fake.reg)
    assert out["status"].tolist() == [0.0, 1.0, 0.0] and out["problem_ids"].tolist() == [5.0, 6.0, 7.0]


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(tmp_path, monkeypatch):
    import bench

    B, n, mi = 50, 20, 10
    row_bytes = 8 * (n + 2 * mi + 2 + 1 + 1)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 12 * row_bytes + 5)
    fake = _FakeSystem(B, n, mi)
    ids = list(range(100, 100 + B))
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, fake, ids, np.zeros(B, dtype=np.int32))
    total = sum(f.stat().st_size - 128 for f in (tmp_path / "a").glob("*.npy"))  # (128-byte .npy headers)
    assert total <= bench.DUMP_LIMIT_BYTES
    kept = np.load(tmp_path / "a" / "problem_ids.npy")
    assert len(kept) == 12 and np.all(np.diff(kept) > 0)
    assert np.array_equal(np.load(tmp_path / "b" / "problem_ids.npy"), kept)
    rows = (kept - 100).astype(int)
    assert np.array_equal(np.load(tmp_path / "a" / "p.npy"), fake.vec["p"][rows])


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_asked_for_and_dumps_its_outputs(slpx, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 7 and line["timing"]["repeats"] == 1 and len(line["timing"]["block_ms"]) == 1
    assert line["ms_per_step"] == pytest.approx(line["timing"]["block_ms"][0] / 7)
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"])
    assert not {"roofline", "whole_solve", "batched", "cpu_baseline"} & set(line)
    cfg = line["config"]
    out = {f.stem: np.load(f) for f in (tmp_path / "out").glob("*.npy")}
    assert out["p"].shape == (1, cfg["n"] + cfg["m_e"]) and out["p_s"].shape == out["p_z"].shape == (1, cfg["m_i"])
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in out.values())
    assert out["status"].tolist() == [0.0] and np.any(out["p"] != 0)
