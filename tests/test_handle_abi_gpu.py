"""The handle C ABI's shared host scaffold (csrc/gunrock/app/handle_runner.hpp) seen through every family's Python class, on
tests/golden/chesapeake.mtx (39 vertices, read undirected, unit weights where a family takes weights).

Every family (the five the benchmark times and the eighteen whose problems keep their device arrays in owning members): create,
init, then reset / enact / extract twice on the same handle.  Both enacts must report a finite elapsed time
above zero and both extracts the same result -- the event pair a runner times with is made once, reused by every run, and is the
one that brackets the enactor.  Integer results must be equal; PageRank and BC sum float32 with atomics in no fixed order, so their
two runs are compared within the tolerances tests/test_pr_gpu.py and tests/test_bc_gpu.py use against the oracle.

The families that guard their phases (MST, MIS, TC, k-core, truss): reset and enact on a handle that took no graph are refused
before any GPU work, and the handle still takes a graph afterwards and computes what a fresh one does.  (The other families do not
guard their phases: the same calls there would read a slice that does not exist, so they are not made.)

The eighteen again, for the ways a problem goes: a handle closed before any init (no slice to free), a handle whose init refused
a malformed CSR (a slice built as far as the check, freed by its members), and a fresh handle afterwards that computes what a
clean one does."""
import gc
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


def _parts(result):
    """a family's extract as a sequence: a dict's values in the order of its keys"""
    return [result[k] for k in sorted(result)] if isinstance(result, dict) else result


def _run(reset, enact, extract=lambda p: p.extract()):
    """one run on an initialised problem: (elapsed ms, the extract with its arrays copied)"""
    def run(p):
        reset(p)
        ms = enact(p)
        return ms, tuple(x.copy() if isinstance(x, np.ndarray) else x for x in _parts(extract(p)))
    return run


def _plain(cls):
    """a family that takes the CSR alone and has reset() / enact() / extract()"""
    return (lambda n, ro, ci: cls().init(n, ro, ci), _run(lambda p: p.reset(), lambda p: p.enact()), _same)


def _with_options(cls, options, then=lambda p: None):
    """a family whose handle takes options before its first reset"""
    def make(n, ro, ci):
        p = cls().init(n, ro, ci)
        for name, value in options:
            p.set_option(name, value)
        then(p)
        return p
    return make


_lp = _with_options(ga.LpProblem, (("mode", ga.LP_SYNC), ("max_rounds", 0)))
_rw = _with_options(ga.RwProblem, (("length", 8), ("seed", 7), ("weighted", 0), ("bias_return", 1), ("bias_in", 1), ("bias_out", 1),
                                   ("tries", 32), ("visits", 0)))
_sample = _with_options(ga.SampleProblem, (("seed", 7), ("replace", 0), ("weighted", 0)), lambda p: p.set_fanouts((5, 3)))
_sim = _with_options(ga.SimProblem, (("metric", ga.SIM_JACCARD),))


def _msbfs_results(p):
    return (p.depths(),) + tuple(p.source_summary()) + tuple(p.vertex_summary())


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
    "scc": _plain(ga.SccProblem),
    "bcc": _plain(ga.BccProblem),
    "matching": _plain(ga.MatchingProblem),
    "c4": _plain(ga.C4Problem),
    "lp": (_lp, _run(lambda p: p.reset(), lambda p: p.enact()), _same),
    "wl": _plain(ga.WlProblem),
    "maxflow": (lambda n, ro, ci: ga.MaxflowProblem().init(n, ro, ci), _run(lambda p: p.reset(SRC, p.nodes - 1), lambda p: p.enact()), _same),
    "clique": (lambda n, ro, ci: ga.CliqueProblem().init(n, ro, ci), _run(lambda p: p.reset(), lambda p: p.enact(3)), _same),
    "rw": (_rw, _run(lambda p: p.reset(np.arange(p.nodes)), lambda p: p.enact()), _same),
    "sample": (_sample, _run(lambda p: p.reset([p.nodes - 1, 0, 7]), lambda p: p.enact()), _same),
    "sim": (_sim,
            _run(lambda p: p.reset(), lambda p: p.pairs(np.arange(p.nodes - 1), np.arange(1, p.nodes)), lambda p: p.extract_pairs()), _same),
    "spgemm": (lambda n, ro, ci: ga.SpgemmProblem().init((n, n), ro, ci), _run(lambda p: p.reset(), lambda p: p.enact()), _same),
    "msbfs": (lambda n, ro, ci: ga.MsbfsProblem().init(n, ro, ci),
              _run(lambda p: p.reset(np.arange(p.nodes)), lambda p: p.enact(), _msbfs_results), _same),
}
# the families whose problems own their device arrays through their members
OWNING = ("bcc", "c4", "clique", "kcore", "lp", "matching", "maxflow", "mis", "msbfs", "mst", "rw", "sample", "scc", "sim", "spgemm", "tc",
          "truss", "wl")
CLASSES = {"bcc": ga.BccProblem, "c4": ga.C4Problem, "clique": ga.CliqueProblem, "kcore": ga.KcoreProblem, "lp": ga.LpProblem,
           "matching": ga.MatchingProblem, "maxflow": ga.MaxflowProblem, "mis": ga.MisProblem, "msbfs": ga.MsbfsProblem, "mst": ga.MstProblem,
           "rw": ga.RwProblem, "sample": ga.SampleProblem, "scc": ga.SccProblem, "sim": ga.SimProblem, "spgemm": ga.SpgemmProblem,
           "tc": ga.TcProblem, "truss": ga.TrussProblem, "wl": ga.WlProblem}
# no CSR: the offsets of 4 vertices decrease between rows 1 and 2
MALFORMED = (4, np.array([0, 2, 1, 3, 3], dtype=np.int32), np.array([1, 2, 3], dtype=np.int32))
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


@pytest.mark.parametrize("family", OWNING)
def test_a_problem_goes_cleanly_however_far_it_was_built(graph, family):
    make, run, same = FAMILIES[family]
    clean = make(*graph)
    _, want = run(clean)
    clean.close()
    # 1. no init: the problem goes without a slice
    CLASSES[family]().close()
    # 2. an init that refuses its graph: the slice goes as far as its build came
    with pytest.raises(RuntimeError, match=r"code -2\b"):
        make(*MALFORMED)
    gc.collect()  # (the refused handle has gone before the next one is made)
    # 3. and the next handle is none the worse for it
    fresh = make(*graph)
    ms, got = run(fresh)
    fresh.close()
    assert math.isfinite(ms) and ms > 0
    assert same(got, want)
