"""Randomised parity sweep of the maximal independent set / greedy colourings (tools/fuzz_mis.py) as part of the GPU suite: fixed
seed, bounded time budget.  R-MAT (directed and mirrored), random COO with duplicates, chains, stars and sparse forests; hashed
order or random int32 priorities with many ties; all three modes, every case bit-exact against the sequential greedy pass."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "15")


def test_fuzz_mis():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_mis.py"), BUDGET_S, "20261016"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
