"""bench.py on the GPU, on a small workload: a plain run times exactly --steps candidate evaluations (9 at pop 6: the
whole population, then its first 3 candidates) and measures nothing else;
--full adds the CPU-baseline, lone-candidate and isolated-kernel legs behind `cpu_baseline` / `roofline`; --dump-outputs
writes what the timed steps returned, one row per step.  With the same arguments both runs return the same objectives (a
candidate's result is bit-identical across runs: fixed-order reductions, no float atomics; its seed is cfg.seed + the
running candidate index, so step k of a run is the same in every run)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--clips", "3000", "--epochs", "1", "--pop", "6", "--slots", "4", "--warmup", "1"]


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    # warm-up steps are steps of the same kind: the run cannot have been shorter than its timed and warm-up steps
    assert (d["steps"] + d["warmup"]) * d["ms_per_step"] / 1e3 <= time.perf_counter() - t0, d
    return d


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_full_run_keeps_the_extra_legs(tmp_path):
    plain = _bench(["--steps", "9", "--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == plain["steps_requested"] == 9 and plain["data"] == "synthetic"
    assert plain["roofline"] is None and "cpu_baseline" not in plain and plain["ms_per_step"] > 0
    assert abs(plain["value"] - 3.6e6 / plain["ms_per_step"]) < 1e-3 * plain["value"]

    full = _bench(["--steps", "9", "--full", "--cpu-baseline-s", "3", "--lone-steps", "8", "--dump-outputs", str(tmp_path / "full")])
    assert full["steps"] == 9 and full["cpu_baseline"]["value"] > 0
    r = full["roofline"]
    assert r["bound"] == "mfma" and r["achieved"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["lone_candidate"]["train_steps"] == 8 and len(r["isolated_single_stream"]) == 3 and "aggregate_timed_region" in r

    for name, shape in (("objs.npy", (9, 3)), ("cv.npy", (9,))):
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.shape == shape and a.dtype == np.float64 and np.isfinite(a).all()
        assert np.array_equal(a, b), name
    assert np.allclose(-np.load(tmp_path / "plain" / "objs.npy")[:, 0].mean(), plain["mean_val_accuracy"], atol=1e-4)
