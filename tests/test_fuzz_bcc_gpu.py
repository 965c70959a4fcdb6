"""Randomised parity sweep of the biconnected components (tools/fuzz_bcc.py) as part of the GPU suite: fixed seed, bounded time
budget.  Random sizes and densities, planted and unplanted graphs, injected duplicates and loops, shuffled rows, permuted ids, random
schedule, wave_min_row and device-loop thresholds; every case bit-exact against the CPU checker."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "15")


def test_fuzz_bcc():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_bcc.py"), BUDGET_S, "20261019"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
