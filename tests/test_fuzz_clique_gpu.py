"""Randomised parity sweep of k-clique counting (tools/fuzz_clique.py) as part of the GPU suite: fixed seed, bounded time budget.
R-MAT, G(n, p), planted cliques and complete multipartite graphs of up to 2^10 vertices, mirrored or one-way entries with injected
loops and duplicates, random k, bitmap_rows, strategy and rank; every case bit-exact against the checker and against one other
configuration of itself.  The sweep fails when it skips more than one case in ten."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "12")


def test_fuzz_clique():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_clique.py"), BUDGET_S, "20261019"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
