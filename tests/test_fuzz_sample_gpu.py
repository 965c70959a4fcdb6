"""Randomised parity sweep of the neighbourhood sampling (tools/fuzz_sample.py) as part of the GPU suite: fixed seed, bounded time
budget.  R-MAT and G(n, p) graphs of up to 2^9 vertices, entries as built, shuffled or dirty, random mode, fanout list, seeds, strategy,
grid, `long_row` and `eids`; every case bit-exact against the vectorised form of the checker, twice on one handle under different
options."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "6")


def test_fuzz_sample():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_sample.py"), BUDGET_S, "20261020"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
