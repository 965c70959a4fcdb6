"""Randomised parity sweep of the bipartite matching (tools/fuzz_bipartite.py) as part of the GPU suite: fixed seed, bounded time
budget.  Rectangular R-MAT-like and G(n, p) patterns of up to 2^9 rows and columns, tall and wide, with injected empty rows and
columns and duplicate entries; random strategy, thresholds, schedule, greedy start and random valid warm starts; every case equal
to the checker, twice on one handle under different options."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "6")


def test_fuzz_bipartite():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_bipartite.py"), BUDGET_S, "20261021"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
