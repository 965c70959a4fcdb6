"""Randomised parity sweep of colour refinement (tools/fuzz_wl.py) as part of the GPU suite: fixed seed, bounded time budget.
R-MAT, G(n, p), hubs, twins, paths and disjoint copies of up to 2^9 vertices, mirrored or one-way entries with injected loops and
duplicates, random labels, strategy, thresholds, table sizes, sig_bits in {128, 8, 2}, seed, max_rounds and history; every case
bit-exact against the checker, twice on one handle under different options."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "6")


def test_fuzz_wl():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_wl.py"), BUDGET_S, "20261020"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
