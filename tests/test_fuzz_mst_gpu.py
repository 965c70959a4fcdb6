"""Randomised parity sweep of the minimum spanning forest (tools/fuzz_mst.py) as part of the GPU suite: fixed seed, bounded time
budget.  R-MAT (directed and mirrored), random COO with duplicates, chains, stars and sparse forests; weights in 1..2 (ties
everywhere) or over the whole int32 range; every case bit-exact against the Kruskal checker."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "15")


def test_fuzz_mst():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_mst.py"), BUDGET_S, "20261016"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 20, tail
