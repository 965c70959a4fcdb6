"""Randomised parity sweep of subgraph matching (tools/fuzz_sm.py) as part of the GPU suite: fixed seed, bounded time budget.
G(n, p) and R-MAT graphs of up to 2^7 vertices as CSRs with duplicates and self-loops; random connected patterns of 2 .. 5 vertices
(6 on graphs of up to 24 vertices); random labels, wildcards, induced or not; random symmetry breaking, strategy, group threshold,
order rule and per_vertex; every case equal to the checker, twice on one handle under different options."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "6")


def test_fuzz_sm():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_sm.py"), BUDGET_S, "20261021"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
