"""bench.py's command line without a GPU: a plain run leaves the secondary measurements to --full, and --dump-outputs writes
float .npy files of bounded size that are identical from run to run."""
import os
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_leaves_secondary_measurements_to_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.skip_topdown_leg and a.no_secondary


def test_full_keeps_todays_default_legs(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not a.no_cpu_baseline and not a.skip_topdown_leg and not a.no_secondary
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--dump-outputs", "out")
    assert a.no_cpu_baseline and not a.no_secondary and a.dump_outputs == "out"


@pytest.mark.parametrize("n", [1000, bench.DUMP_LIMIT + 12345])
def test_dump_outputs_types_size_and_repeatability(tmp_path, n):
    rng = np.random.default_rng(3)
    labels = rng.integers(-1, 9, n, dtype=np.int32)
    ranks = rng.random(n, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"labels": labels, "ranks": ranks})
    for name, src in (("labels", labels), ("ranks", ranks)):
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == (np.float64 if name == "labels" else np.float32)
        assert a.shape == (min(n, bench.DUMP_LIMIT),) and np.array_equal(a, b)
        if n <= bench.DUMP_LIMIT:
            assert np.array_equal(a, src.astype(a.dtype))
        else:  # a sample of the elements, in index order
            assert set(np.unique(a)) <= set(np.unique(src.astype(a.dtype)))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1000 * 1000
