"""bench.py's plain run and --dump-outputs: the number of timed steps, the legs a plain run leaves to --full, and the
arrays written from the last timed step (same arguments -> same arrays).  CPU tests use the stand-in engine of --dry-run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_TRAJECTORY = ("cost", "alpha", "change", "tracking_error", "terminal_error", "attempts")
NAMES = set(PER_TRAJECTORY) | {"cost_allreduce", "u_sample", "phi_sample"}


def _bench(args, timeout=300):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=timeout)


def _result(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[:2000]
    return json.loads(lines[0])


def _load(d, prefix=""):
    return {n: np.load(os.path.join(d, prefix + n + ".npy"), allow_pickle=False) for n in NAMES}


def test_steps_must_be_positive():
    r = _bench(["--steps", "0", "--dry-run"])
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dry_run_dump_outputs_single_rank(tmp_path):
    """One rank, two contexts of two: exactly --steps timed steps, no roofline / CPU baseline without --full, and the
    last step's results in float64 (the stand-in engine reports cost 1/k at its k-th iteration: warm-up 1 + 3 steps)."""
    out = _result(_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dry-run", "--contexts", "2",
                          "--batch-per-gpu", "4", "--dump-outputs", str(tmp_path)]))
    assert out["steps"] == 3 and len(out["cost_sum_per_step"]) == 3 and out["ms_per_step"] > 0
    assert out["roofline"] is None and out["cpu_baseline"] is None
    assert {f[:-4] for f in os.listdir(tmp_path)} == NAMES
    d = _load(tmp_path)
    assert all(a.dtype == np.float64 for a in d.values())
    for n in PER_TRAJECTORY:
        assert d[n].shape == (4,)
    assert np.allclose(d["cost"], 0.25) and np.allclose(d["attempts"], 0.0)
    assert np.isclose(d["cost_allreduce"][4], out["cost_sum_per_step"][-1])
    assert d["u_sample"].shape == (4, 12) and np.allclose(d["u_sample"], 0.25)


def test_dry_run_dump_outputs_two_ranks(tmp_path):
    """Two ranks (the bare command starts them): each writes its own trajectories under a rank prefix."""
    _result(_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run", "--contexts", "1", "--batch-per-gpu", "2",
                    "--dump-outputs", str(tmp_path)]))
    assert {f[:-4] for f in os.listdir(tmp_path)} == {f"rank{r}.{n}" for r in (0, 1) for n in NAMES}
    for r in (0, 1):
        d = _load(tmp_path, f"rank{r}.")
        assert d["cost"].shape == (2,) and np.allclose(d["cost"], 1.0 / 3)
        assert np.allclose(d["cost_allreduce"][4], 4.0 / 3)


class _FakeEngine:
    def __init__(self, B, offset):
        self.B, self.offset = B, offset

    def pgd_get(self, what):
        base = np.arange(self.B * 5 * 4 * 4, dtype=np.float64).reshape(self.B, 5, 4, 4)
        return base + self.offset + (0.5 if what == "phi" else 0.0)


def test_dump_samples_the_same_positions_of_every_trajectory(tmp_path, monkeypatch):
    """A history larger than its share of the budget is sampled at positions drawn from a fixed seed: the same sorted,
    distinct positions for every trajectory and context, and the same again in a second call."""
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ENTRIES", 64)         # 4 trajectories -> 16 of the 80 entries each
    engs = [_FakeEngine(2, 0.0), _FakeEngine(2, 1000.0)]
    rs = [dict((k, np.full((2, 1), 1.0 + i)) for k in PER_TRAJECTORY) for i in range(2)]
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), (rs, np.arange(5.0)), engs, 1, 0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(a[n], b[n])
    u = a["u_sample"]
    assert u.shape == (4, 16)
    pos = u[0]                                                    # trajectory 0 holds its own flat positions
    assert np.all(np.diff(pos) > 0) and pos.max() < 80
    for t, e_off in ((1, 0.0), (2, 1000.0), (3, 1000.0)):
        assert np.array_equal(u[t], pos + (t % 2) * 80 + e_off)
    assert np.array_equal(a["phi_sample"], u + 0.5)
    assert np.array_equal(a["cost"], [1.0, 1.0, 2.0, 2.0])


@pytest.mark.gpu
def test_bench_plain_run_dumps_identical_outputs(tmp_path):
    """On the card at a small size: a plain run times --steps steps and runs neither the roofline iteration nor the CPU
    baseline; two runs with the same arguments write the same last-step arrays bit for bit (the engine's arithmetic is
    deterministic and the inputs are seeded), within the 64 MB budget, consistent with the result line."""
    args = ["--grid", "64", "--time-steps", "20", "--batch-per-gpu", "2", "--contexts", "2", "--steps", "3", "--warmup", "1"]
    outs = [_result(_bench(args + ["--dump-outputs", str(tmp_path / tag)], timeout=600)) for tag in ("a", "b")]
    for out in outs:
        assert out["steps"] == 3 and len(out["cost_sum_per_step"]) == 3 and out["ms_per_step"] > 0
        assert out["roofline"] is None and out["cpu_baseline"] is None
    assert outs[0]["cost_sum_per_step"] == outs[1]["cost_sum_per_step"]
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for n in NAMES:
        assert a[n].dtype == np.float64
        assert np.array_equal(a[n], b[n], equal_nan=True), n
    assert a["u_sample"].shape == (2, 21 * 65 * 65) and a["phi_sample"].shape == (2, 21 * 65 * 65)
    assert np.isfinite(a["u_sample"]).all() and np.isfinite(a["phi_sample"]).all()
    assert a["cost_allreduce"][4] == outs[0]["cost_sum_per_step"][-1]
