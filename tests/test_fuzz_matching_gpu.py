"""Randomised parity sweep of the heavy-edge matching and its contraction (tools/fuzz_matching.py) as part of the GPU suite: fixed
seed, bounded time budget.  Random sizes up to 2^12 and densities, four graph families, mirrored or one-way entries, injected
duplicates and self-loops, shuffled rows, NULL, single-valued, tied, wide and extreme weights, random seed, schedule, wave_min_row and
device-loop thresholds; the matching, the round count and one contraction per case bit-exact against the CPU checker."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "15")


def test_fuzz_matching():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_matching.py"), BUDGET_S, "20261019"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
