"""Randomised parity sweep of the maximum flow and the minimum cuts (tools/fuzz_maxflow.py) as part of the GPU suite: fixed seed,
bounded time budget.  Random sizes up to 2^12 and densities, four graph families, unit, small, wide and huge capacities, injected
parallel and antiparallel arcs and loops, shuffled rows, several (src, sink) pairs per handle, random schedule, wave_min_row,
discharge_steps, relabel_interval and device-loop thresholds; every unique result bit-exact against the CPU checker, every flow
validated."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_S = os.environ.get("GUNROCK_FUZZ_SECONDS", "15")


def test_fuzz_maxflow():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_maxflow.py"), BUDGET_S, "20261019"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    tail = "\n".join(r.stdout.splitlines()[-15:])
    assert r.returncode == 0 and "fuzz ok:" in r.stdout, tail
    assert int(r.stdout.split("fuzz ok:")[1].split()[0]) >= 5, tail
