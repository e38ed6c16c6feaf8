"""bench.py's command line: --steps is checked, a plain run prints the headline line only, --dump-outputs writes the same
outputs (up to rounding) in two runs with the same arguments, --full adds the secondary measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT

DUMPED = ("grad_norm.npy", "grads.npy", "loss.npy", "weights.npy")


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    return r


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_steps_must_be_positive():
    r = _bench("--steps", "0")
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_dump_outputs_are_the_same_in_two_runs(tmp_path):
    lines = []
    for run in ("a", "b"):
        lines.append(_line(_bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / run))))
    for d in lines:
        assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert "roofline" not in d and "cpu_baseline" not in d  # a plain run: the headline only
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == list(DUMPED)
    for name in DUMPED:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), name
        a64 = a.astype(np.float64)
        assert np.linalg.norm(a64 - b) <= 1e-5 * np.linalg.norm(a64) + 1e-30, name  # atomics' rounding only


@pytest.mark.gpu
def test_full_adds_the_secondary_measurements():
    d = _line(_bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-hifigan",
                     "--no-fp32", "--no-inference"))
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert d["roofline"]["forward_ms"] > 0 and d["roofline"]["families"], d["roofline"]
