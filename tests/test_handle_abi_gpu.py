"""The handle C ABI's shared host scaffold (csrc/gunrock/app/handle_runner.hpp) seen through every family's Python class, on
tests/golden/chesapeake.mtx (39 vertices, read undirected, unit weights where a family takes weights).

Every family: create, init, then reset / enact / extract twice on the same handle.  Both enacts must report a finite elapsed time
above zero and both extracts the same result -- the event pair a runner times with is made once, reused by every run, and is the
one that brackets the enactor.  Integer results must be equal; PageRank and BC sum float32 with atomics in no fixed order, so their
two runs are compared within the tolerances tests/test_pr_gpu.py and tests/test_bc_gpu.py use against the oracle.

The families that guard their phases (MST, MIS, TC, k-core, truss): reset and enact on a handle that took no graph are refused
before any GPU work, and the handle still takes a graph afterwards and computes what a fresh one does.  (The other families do not
guard their phases: the same calls there would read a slice that does not exist, so they are not made.)"""
import math
import os

import numpy as np
import pytest

import gunrockinst_amd as ga

pytestmark = pytest.mark.gpu

PR_RTOL, PR_ATOL = 1e-4, 1e-6      # tests/test_pr_gpu.py
BC_RTOL, BC_ATOL = 1e-3, 1e-3      # tests/test_bc_gpu.py
SRC = 0


@pytest.fixture(scope="module")
def graph(golden_dir):
    g = ga.HostGraph.from_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    ro, ci = np.array(g.row_offsets), np.array(g.col_indices)
    nodes = g.nodes
    g.close()
    assert nodes == 39 and ro.shape[0] == 40 and ci.shape[0] == ro[-1] > 0
    for a in (ro, ci):
        a.setflags(write=False)
    return nodes, ro, ci


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def _pr_same(a, b):
    """(ids, ranks) in descending rank order: compared by vertex, so a tie inside the tolerance may swap places"""
    by_vertex = [np.zeros(ids.shape[0], np.float64) for ids, _ in (a, b)]
    for out, (ids, ranks) in zip(by_vertex, (a, b)):
        assert sorted(ids.tolist()) == list(range(ids.shape[0]))
        out[ids] = ranks
    return np.allclose(by_vertex[0], by_vertex[1], rtol=PR_RTOL, atol=PR_ATOL)


def _bc_same(a, b):
    (sig_a, bc_a), (sig_b, bc_b) = a, b
    return np.array_equal(sig_a, sig_b) and np.all(np.abs(bc_a.astype(np.float64) - bc_b) <= BC_RTOL * np.abs(bc_b) + BC_ATOL)


def _weights(ci, dtype):
    return np.ones(ci.shape[0], dtype=dtype)


def _run(reset, enact):
    """one run on an initialised problem: (elapsed ms, the extract with its arrays copied)"""
    def run(p):
        reset(p)
        ms = enact(p)
        return ms, tuple(x.copy() if isinstance(x, np.ndarray) else x for x in p.extract())
    return run


# family -> (make an initialised problem from (nodes, ro, ci), one run, compare two results)
FAMILIES = {
    "bfs": (lambda n, ro, ci: ga.BfsProblem().init(n, ro, ci), _run(lambda p: p.reset(SRC), lambda p: p.enact(SRC)), _same),
    "bc": (lambda n, ro, ci: ga.BcProblem().init(n, ro, ci), _run(lambda p: None, lambda p: p.run(-1)), _bc_same),
    "cc": (lambda n, ro, ci: ga.CcProblem().init(n, ro, ci), _run(lambda p: p.reset(), lambda p: p.enact()), _same),
    "sssp": (lambda n, ro, ci: ga.SsspProblem().init(n, ro, ci, _weights(ci, np.uint32)),
             _run(lambda p: p.reset(SRC), lambda p: p.enact(SRC)), _same),
    "pr": (lambda n, ro, ci: ga.PrProblem().init(n, ro, ci).set_inverse_graph(), _run(lambda p: p.reset(), lambda p: p.enact()), _pr_same),
    "mst": (lambda n, ro, ci: ga.MstProblem().init(n, ro, ci, _weights(ci, np.int32)), _run(lambda p: p.reset(), lambda p: p.enact()), _same),
    "mis": (lambda n, ro, ci: ga.MisProblem().init(n, ro, ci), _run(lambda p: p.reset(), lambda p: p.enact()), _same),
    "tc": (lambda n, ro, ci: ga.TcProblem().init(n, ro, ci), _run(lambda p: p.reset(), lambda p: p.enact()), _same),
    "kcore": (lambda n, ro, ci: ga.KcoreProblem().init(n, ro, ci), _run(lambda p: p.reset(), lambda p: p.enact()), _same),
    "truss": (lambda n, ro, ci: ga.TrussProblem().init(n, ro, ci), _run(lambda p: p.reset(), lambda p: p.enact()), _same),
}
# the same init on a handle made earlier, for the families whose phases are guarded
GUARDED = {
    "mst": (ga.MstProblem, lambda p, n, ro, ci: p.init(n, ro, ci, _weights(ci, np.int32))),
    "mis": (ga.MisProblem, lambda p, n, ro, ci: p.init(n, ro, ci)),
    "tc": (ga.TcProblem, lambda p, n, ro, ci: p.init(n, ro, ci)),
    "kcore": (ga.KcoreProblem, lambda p, n, ro, ci: p.init(n, ro, ci)),
    "truss": (ga.TrussProblem, lambda p, n, ro, ci: p.init(n, ro, ci)),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_two_runs_on_one_handle(graph, family):
    make, run, same = FAMILIES[family]
    p = make(*graph)
    (ms1, first), (ms2, second) = run(p), run(p)
    p.close()
    print("%s: %.6f ms, %.6f ms" % (family, ms1, ms2))
    assert math.isfinite(ms1) and ms1 > 0 and math.isfinite(ms2) and ms2 > 0
    assert same(first, second)


@pytest.mark.parametrize("family", sorted(GUARDED))
def test_phases_before_init_are_refused_and_leave_the_handle_usable(graph, family):
    cls, init = GUARDED[family]
    run, same = FAMILIES[family][1:]
    p = cls()
    with pytest.raises(RuntimeError, match="failed"):
        p.reset()
    with pytest.raises(RuntimeError, match="failed"):
        p.enact()
    init(p, *graph)
    ms, late = run(p)
    p.close()
    fresh = FAMILIES[family][0](*graph)
    _, want = run(fresh)
    fresh.close()
    assert math.isfinite(ms) and ms > 0
    assert same(late, want)
