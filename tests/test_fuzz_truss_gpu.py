"""Randomised parity sweep of per-edge support and the k-truss decomposition (tools/fuzz_truss.py) as part of the GPU suite: fixed
seed, bounded time budget.  Random sizes and densities, directed and undirected inputs, shuffled rows and injected duplicates and
loops, random schedule, wave_min_row, device-loop thresholds and k_limit; every case bit-exact against the numpy peel."""
import os
import subprocess
import sys

import pytest

import _truss_checker  # noqa: F401  (the sweep's reference)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "15")


def test_fuzz_truss():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_truss.py"), BUDGET_S, "20261017"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
