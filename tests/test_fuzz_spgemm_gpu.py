"""Randomised parity sweep of the sparse product (tools/fuzz_spgemm.py) as part of the GPU suite: fixed seed, bounded time budget.
Shapes of up to 300 rows, inner and cols, uniform or with dense rows, signed, non-negative or absent values, shuffled rows and
duplicates, the right operand A, its transpose or given; random strategy, thresholds, scratch budget, grid and pattern_only; every
case bit-exact against the expand form of the checker, twice on one handle under different options."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "6")


def test_fuzz_spgemm():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_spgemm.py"), BUDGET_S, "20261020"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 24, tail
