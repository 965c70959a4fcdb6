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
clean one does.

The five, whose slices are views of owners held beside them in the problem: a handle closed before any init; a CSR on the device
that the test owns (gunrockinst_amd/devgraph.py), borrowed by one handle after the other, and intact after each close; the builds
a handle may repeat (the relabelled copy and the inverse of BFS, the transposes SSSP and PageRank build themselves), which must
compute what a handle that built once does; and a second init on one handle."""
import gc
import math
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

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


# ---- the five families the benchmark times: the slice is a view, its owners sit beside it in the problem ----
FIVE = ("bc", "bfs", "cc", "pr", "sssp")
FIVE_CLASSES = {"bc": ga.BcProblem, "bfs": ga.BfsProblem, "cc": ga.CcProblem, "pr": ga.PrProblem, "sssp": ga.SsspProblem}
# the same init on a handle made earlier
FIVE_INIT = {
    "bc": lambda p, n, ro, ci: p.init(n, ro, ci),
    "bfs": lambda p, n, ro, ci: p.init(n, ro, ci),
    "cc": lambda p, n, ro, ci: p.init(n, ro, ci),
    "pr": lambda p, n, ro, ci: p.init(n, ro, ci).set_inverse_graph(),
    "sssp": lambda p, n, ro, ci: p.init(n, ro, ci, _weights(ci, np.uint32)),
}
SSSP_DELTA = 16.0  # (any bucket width: distances do not depend on it)


@pytest.fixture(scope="module")
def wanted(graph):
    """what a clean handle of each of the five computes, once"""
    out = {}
    for family in FIVE:
        make, run, _ = FAMILIES[family]
        p = make(*graph)
        out[family] = run(p)[1]
        p.close()
    return out


@pytest.mark.parametrize("family", FIVE)
def test_the_five_closed_before_any_init(graph, wanted, family):
    make, run, same = FAMILIES[family]
    FIVE_CLASSES[family]().close()  # no slice, no graph slice, no stream: nothing to free
    fresh = make(*graph)
    ms, got = run(fresh)
    fresh.close()
    assert math.isfinite(ms) and ms > 0
    assert same(got, wanted[family])


@pytest.fixture(scope="module")
def device_graph(graph):
    """chesapeake's CSR in device arrays the test owns, built from its (row, column) pairs by the library's device sort"""
    import torch
    nodes, ro, ci = graph
    rows = torch.from_numpy(np.repeat(np.arange(nodes, dtype=np.int32), np.diff(ro))).cuda()
    cols = torch.from_numpy(np.array(ci, dtype=np.int32)).cuda()
    d_ro, d_ci = devgraph.csr_from_tuples_device(nodes, rows, cols, undirected=False)
    d_w = torch.ones(ci.shape[0], dtype=torch.int32, device="cuda")  # (the bits of uint32 ones)
    torch.cuda.synchronize()
    return d_ro, d_ci, d_w


def _intact(device_graph, graph):
    d_ro, d_ci, d_w = device_graph
    h_ro, h_ci = devgraph.to_host_csr(d_ro, d_ci)
    return np.array_equal(h_ro, graph[1]) and np.array_equal(h_ci, graph[2]) and bool((d_w == 1).all())


@pytest.mark.parametrize("family", FIVE)
def test_a_borrowed_csr_outlives_the_handles_that_used_it(graph, device_graph, wanted, family):
    nodes, _, ci = graph
    d_ro, d_ci, d_w = device_graph
    run, same = FAMILIES[family][1:]
    assert _intact(device_graph, graph)
    results = []
    for _ in range(2):  # the second handle reads what the first one's close must not have freed
        p = FIVE_CLASSES[family]()
        if family == "sssp":
            p.init_device(nodes, ci.shape[0], d_ro.data_ptr(), d_ci.data_ptr(), d_w.data_ptr(), SSSP_DELTA)
        else:
            p.init_device(nodes, ci.shape[0], d_ro.data_ptr(), d_ci.data_ptr())
        if family == "pr":
            p.set_inverse_graph()
        ms, got = run(p)
        p.close()
        assert math.isfinite(ms) and ms > 0
        assert _intact(device_graph, graph)
        results.append(got)
    assert same(results[0], results[1])
    assert same(results[0], wanted[family])


def _valid_parents(graph, labels, preds, src):
    """every reached vertex but the source has a parent one level up that lists it; the source -1, the unreached -2"""
    _, ro, ci = graph
    for v, (l, p) in enumerate(zip(labels.tolist(), preds.tolist())):
        if v == src:
            ok = (l, p) == (0, -1)
        elif l < 0:
            ok = p == -2
        else:
            ok = p >= 0 and labels[p] == l - 1 and v in ci[ro[p]:ro[p + 1]]
        if not ok:
            return False
    return True


@pytest.mark.parametrize("mark_pred", (False, True))
def test_bfs_rebuilds_its_copy_and_its_inverse(graph, mark_pred):
    """The relabelled copy is built by auto_inverse(), again by another relabel_hubs, and again by a second auto_inverse(); every
    search on the copy gives the depths of a handle that built once.  Which of several parents one level up a vertex gets is decided
    by the order two wavefronts arrive in, on a single build as well, so parents are checked for being parents."""
    def search(p):
        p.reset(SRC)
        ms = p.enact(SRC, traversal_mode=2)
        labels, preds = p.extract()
        assert math.isfinite(ms) and ms > 0
        assert preds is None or _valid_parents(graph, labels, preds, SRC)
        return labels.copy()

    once = ga.BfsProblem(mark_pred=mark_pred).init(*graph)
    assert once.auto_inverse()[0]
    once.set_option("relabel", 1)
    want = search(once)
    once.close()
    assert want[SRC] == 0 and want.max() > 0

    p = ga.BfsProblem(mark_pred=mark_pred).init(*graph)
    assert p.auto_inverse()[0]
    p.set_option("relabel", 1)
    hubs = p.relabel_info()["hubs"]
    assert hubs >= 0
    first = search(p)
    p.set_option("relabel_hubs", 2 if hubs != 2 else 3)  # another hub tier: the copy is built again
    assert p.relabel_info()["hubs"] != hubs
    second = search(p)
    assert p.auto_inverse()[0]  # the inverse and the copy once more
    third = search(p)
    p.close()
    assert np.array_equal(first, want) and np.array_equal(second, want) and np.array_equal(third, want)


def test_sssp_builds_its_inverse_twice(graph, wanted):
    nodes, ro, ci = graph
    results = []
    for builds in (1, 2):
        p = ga.SsspProblem().init(nodes, ro, ci, _weights(ci, np.uint32))
        for _ in range(builds):
            p.set_inverse_graph(pull_min_edges=1)  # the weighted transpose, built by the problem; every level may pull
        _, got = FAMILIES["sssp"][1](p)
        p.close()
        results.append(got)
    assert _same(results[0], results[1])
    assert _same(results[1], wanted["sssp"])


def test_pr_builds_its_inverse_twice(graph, wanted):
    nodes, ro, ci = graph
    results = []
    for builds in (1, 2):
        p = ga.PrProblem().init(nodes, ro, ci)
        for _ in range(builds):
            p.set_inverse_graph(build=True)  # the transpose, built by the problem
        _, got = FAMILIES["pr"][1](p)
        p.close()
        results.append(got)
    assert _pr_same(results[0], results[1])
    assert _pr_same(results[1], wanted["pr"])


@pytest.mark.parametrize("family", FIVE)
def test_a_second_init_on_one_handle(graph, wanted, family):
    """init, run, init again with the same graph, run: the first slice and its arrays go, the second run computes the same"""
    run, same = FAMILIES[family][1:]
    p = FIVE_CLASSES[family]()
    FIVE_INIT[family](p, *graph)
    _, first = run(p)
    FIVE_INIT[family](p, *graph)
    ms, second = run(p)
    p.close()
    assert math.isfinite(ms) and ms > 0
    assert same(first, second)
    assert same(second, wanted[family])
