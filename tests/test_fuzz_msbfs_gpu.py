"""Randomised parity sweep of the multi-source BFS (tools/fuzz_msbfs.py) as part of the GPU suite: fixed seed, bounded time budget.
Random sizes and densities, directed and undirected graphs, injected duplicates and loops, shuffled rows, 1..200 sources with
repeats, random direction, inverse, wave_min_row, thresholds and store_depths; every case bit-exact against the CPU checker."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "15")


def test_fuzz_msbfs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_msbfs.py"), BUDGET_S, "20261018"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
