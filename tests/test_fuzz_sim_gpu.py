"""Randomised parity sweep of vertex similarity (tools/fuzz_sim.py) as part of the GPU suite: fixed seed, bounded time budget.
R-MAT, G(n, p), random bipartite graphs and hubs of up to 2^9 vertices, mirrored, one-way, shuffled or dirty entries, random metric,
strategy, thresholds, scratch budget, grid, k and skip_neighbors; every case bit-exact against the dense form of the checker in both
modes, twice on one handle under different options."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "6")


def test_fuzz_sim():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_sim.py"), BUDGET_S, "20261020"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
