"""4-cycle (butterfly) counting on the GPU (grx_c4_*): `cycles`, `edge_cycles` and `total` must equal tests/_c4_checker.py's two forms
or its closed forms, int64 against int64 with np.array_equal, and must not move under anything that is not the graph: the regime, the
thresholds, the scratch budget, the grid, the form the CSR comes in.  Which regime took a start vertex is asserted from stats against
the checker's W(u) and a restatement of the rule: the smallest regime that holds W, not below a forced one."""
import os
from math import comb

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _c4_checker as k
from _tc_checker import simple_edges

pytestmark = pytest.mark.gpu

STRATEGIES = (ga.C4_AUTO, ga.C4_LANE, ga.C4_WAVE, ga.C4_BLOCK, ga.C4_GLOBAL)
REGIMES = ("lane", "wave", "block", "global")
NOT_READY = "code 600"  # hipErrorNotReady
LOW = {"lane_max_wedges": 4, "table_slots": 64, "block_slots": 256}  # the borders at W = 4, 32 and 128
DEFAULTS = {"strategy": ga.C4_AUTO, "lane_max_wedges": 16, "table_slots": 1024, "block_slots": 8192, "scratch_mib": 1024, "edges": 1,
            "count_limit": 2.0 ** 62}


def _regime(w, strategy=ga.C4_AUTO, lane_max_wedges=16, table_slots=1024, block_slots=8192):
    r = max(strategy, ga.C4_LANE)
    if r == ga.C4_LANE and w > lane_max_wedges:
        r = ga.C4_WAVE
    if r == ga.C4_WAVE and w > table_slots // 2:
        r = ga.C4_BLOCK
    if r == ga.C4_BLOCK and w > block_slots // 2:
        r = ga.C4_GLOBAL
    return r


def _expected_regimes(W, **options):
    """({regime: start vertices}, {regime: wedges}) for the checker's W under the options"""
    vertices, wedges = dict.fromkeys(REGIMES, 0), dict.fromkeys(REGIMES, 0)
    for w in W[W >= 2].tolist():
        name = REGIMES[_regime(w, **{key: v for key, v in options.items() if key in ("strategy",) + tuple(LOW)}) - 1]
        vertices[name] += 1
        wedges[name] += w
    return vertices, wedges


def _run(p, max_grid_size=0, **options):
    for key, value in {**DEFAULTS, **options}.items():
        assert p.set_option(key, value) == 0, key
    p.reset()
    p.enact(max_grid_size)
    cycles, total = p.extract()
    assert cycles.dtype == np.int64 and int(cycles.sum()) == 4 * total
    assert p.extract(cycles=False) == (None, total)
    edge = None
    if options.get("edges", 1):
        edge = p.extract_edges().copy()
        assert edge.dtype == np.int64 and int(edge.sum()) == 4 * total
    return cycles.copy(), edge, total, p.stats()


def _same(got, want, what=""):
    """got: _run's tuple; want: (cycles, edge_cycles or None, total)"""
    assert np.array_equal(got[0], want[0]), "%s: cycles differ at %s" % (what, np.flatnonzero(got[0] != want[0])[:10])
    if got[1] is not None and want[1] is not None:
        assert np.array_equal(got[1], want[1]), "%s: edge_cycles differ at %s" % (what, np.flatnonzero(got[1] != want[1])[:10])
    assert got[2] == want[2], what


def _stats_match(st, ref, **options):
    vertices, wedges = _expected_regimes(ref["W"], **options)
    assert {name: st[name + "_vertices"] for name in REGIMES} == vertices, (st, vertices)
    assert {name: st[name + "_wedges"] for name in REGIMES} == wedges, (st, wedges)
    assert st["wedges"] == ref["wedges"] and st["simple_edges"] == ref["src"].shape[0]


def _ref(n, ro, ci):
    r = k.ranked(n, ro, ci)
    return (r["cycles"], r["edge_cycles"], r["total"]), r


@pytest.fixture(scope="module")
def chesapeake(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    return g.nodes, g.row_offsets, g.col_indices


@pytest.fixture(scope="module")
def rmat10():
    g = o.rmat_seeded(10, 8 << 10)
    want, r = _ref(g.nodes, g.row_offsets, g.col_indices)
    _same(k.dense(g.nodes, g.row_offsets, g.col_indices), want, "the two forms on rmat10")
    return g.nodes, g.row_offsets, g.col_indices, want, r


# ---------------- golden graphs ----------------

def test_chesapeake(chesapeake):
    n, ro, ci = chesapeake
    want, r = _ref(n, ro, ci)
    _same(k.dense(n, ro, ci), want)
    p = ga.C4Problem().init(n, ro, ci)
    for strategy in STRATEGIES:
        got = _run(p, strategy=strategy)
        _same(got, want, "strategy %d" % strategy)
        _stats_match(got[3], r, strategy=strategy)
    src, dst = p.edges()
    p.close()
    assert np.array_equal(src, r["src"]) and np.array_equal(dst, r["dst"]) and src.dtype == np.int32
    assert (got[2], int(got[0].max()), int(got[1].max()), got[3]["wedges"]) == (1762, 944, 94, 692)
    assert got[3]["bound"] == r["bound"]  # (multiples of 1/2 far below 2^53: exact in any order)
    cycles, total = ga.gunrock_four_cycles(n, ro, ci)
    assert np.array_equal(cycles, want[0]) and total == 1762
    src, dst, edge, total = ga.gunrock_edge_four_cycles(n, ro, ci)
    assert np.array_equal(src, r["src"]) and np.array_equal(dst, r["dst"]) and np.array_equal(edge, want[1]) and total == 1762


def test_bips98_606(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "bips98_606.mtx"), undirected=True)
    want, r = _ref(g.nodes, g.row_offsets, g.col_indices)
    p = ga.C4Problem().init(g.nodes, g.row_offsets, g.col_indices)
    for options in ({}, LOW):
        got = _run(p, **options)
        _same(got, want, "bips98_606 %s" % options)
        _stats_match(got[3], r, **options)
    p.close()
    assert want[2] > 0


def test_rmat10(rmat10):
    n, ro, ci, want, r = rmat10
    p = ga.C4Problem().init(n, ro, ci)
    got = _run(p)
    p.close()
    _same(got, want, "rmat10")
    _stats_match(got[3], r)
    assert got[3]["bound"] >= want[2] and got[3]["table_probes"] > 0


# ---------------- closed forms ----------------

CLOSED = {
    "K_3_5": (k.complete_bipartite(3, 5), k.complete_bipartite_counts(3, 5)),
    "K_1_7": (k.complete_bipartite(1, 7), k.complete_bipartite_counts(1, 7)),
    "K_6": (k.complete(6), k.complete_counts(6)),
    "Q_4": (k.hypercube(4), k.hypercube_counts(4)),
    "grid_5x7": (k.grid(5, 7), (k.grid_total(5, 7), None, None)),
    "C_4": (k.cycle(4), (1, np.ones(4, np.int64), np.ones(4, np.int64))),
    "C_5": (k.cycle(5), (0, np.zeros(5, np.int64), np.zeros(5, np.int64))),
    "petersen": (k.petersen(), (0, np.zeros(10, np.int64), np.zeros(15, np.int64))),
    "n_1": (k.edgeless(1), (0, np.zeros(1, np.int64), np.zeros(0, np.int64))),
    "n_2": (k.complete(2), (0, np.zeros(2, np.int64), np.zeros(1, np.int64))),
    "edgeless": (k.edgeless(9), (0, np.zeros(9, np.int64), np.zeros(0, np.int64))),
}


@pytest.mark.parametrize("name", sorted(CLOSED))
def test_closed_forms(name):
    graph, (total, per_vertex, per_edge) = CLOSED[name]
    n, ro, ci = k.mirrored(graph)
    want, r = _ref(n, ro, ci)
    assert want[2] == total and (per_vertex is None or np.array_equal(want[0], per_vertex)) and (per_edge is None or np.array_equal(want[1], per_edge))
    p = ga.C4Problem().init(n, ro, ci)
    for strategy in STRATEGIES:
        got = _run(p, strategy=strategy)
        _same(got, want, "%s strategy %d" % (name, strategy))
        _stats_match(got[3], r, strategy=strategy)
    p.close()


@pytest.mark.parametrize("n", [4, 5, 33, 65])
def test_complete_graphs(n):
    """K_n: every degree ties, the rank is the id"""
    _, ro, ci = k.mirrored(k.complete(n))
    total, per_vertex, per_edge = k.complete_counts(n)
    r = k.ranked(n, ro, ci)
    p = ga.C4Problem().init(n, ro, ci)
    for options in ({}, LOW, dict(LOW, strategy=ga.C4_GLOBAL)):
        got = _run(p, **options)
        _same(got, (per_vertex, per_edge, total), "K_%d %s" % (n, options))
        _stats_match(got[3], r, **options)
    p.close()


# ---------------- the borders of the regimes ----------------

@pytest.mark.parametrize("t", [1, 2, 3, 4, 5, 31, 32, 33, 127, 128, 129])
def test_table_borders(t):
    """theta(t): one start vertex with t wedges into one end; spider(t): one with t wedges into t ends, a full table"""
    n, ro, ci = k.mirrored(k.union(k.theta(t), k.spider(t)))
    want, r = _ref(n, ro, ci)
    assert want[2] == comb(t, 2)
    p = ga.C4Problem().init(n, ro, ci)
    got = _run(p, **LOW)
    _same(got, want, "t %d" % t)
    _stats_match(got[3], r, **LOW)
    if t >= 3:
        regime = "lane" if t <= 4 else "wave" if t <= 32 else "block" if t <= 128 else "global"
        assert got[3][regime + "_vertices"] == 2 and got[3][regime + "_wedges"] == 2 * t
        assert sum(got[3][name + "_vertices"] for name in REGIMES) == 2
    for strategy in STRATEGIES[1:]:
        forced = _run(p, strategy=strategy, **LOW)
        _same(forced, want, "t %d strategy %d" % (t, strategy))
        _stats_match(forced[3], r, strategy=strategy, **LOW)
    p.close()


def test_regimes_agree(rmat10):
    n, ro, ci, want, r = rmat10
    vertices, _ = _expected_regimes(r["W"], **LOW)
    assert all(vertices[name] > 0 for name in REGIMES), vertices  # (on the CPU: the graph fills every regime at these thresholds)
    p = ga.C4Problem().init(n, ro, ci)
    auto = _run(p, **LOW)
    _same(auto, want, "AUTO")
    _stats_match(auto[3], r, **LOW)
    assert all(auto[3][name + "_vertices"] > 0 for name in REGIMES), auto[3]
    for strategy in STRATEGIES[1:]:
        for options in (LOW, {}):
            got = _run(p, strategy=strategy, **options)
            assert got[0].tobytes() == auto[0].tobytes() and got[1].tobytes() == auto[1].tobytes() and got[2] == auto[2], (strategy, options)
            _stats_match(got[3], r, strategy=strategy, **options)
            for below in REGIMES[:strategy - 1]:
                assert got[3][below + "_vertices"] == 0
    p.close()


def test_one_global_slot_and_one_workgroup(rmat10):
    n, ro, ci, want, r = rmat10
    p = ga.C4Problem().init(n, ro, ci)
    for what, grid, options in (("scratch_mib 1 (4 n bytes a row: 256 rows)", 0, dict(LOW, scratch_mib=1)),
                                ("max_grid_size 1", 1, LOW), ("max_grid_size 1, all GLOBAL", 1, dict(LOW, strategy=ga.C4_GLOBAL)),
                                ("max_grid_size 3, all GLOBAL", 3, dict(LOW, strategy=ga.C4_GLOBAL, scratch_mib=1))):
        got = _run(p, grid, **options)
        _same(got, want, what)
        _stats_match(got[3], r, **options)
    p.close()
    # one slot: a graph whose row of 4 n bytes does not fit the budget twice
    big = 300_000
    graph = k.union(k.theta(200), k.spider(150), k.edgeless(big))
    n, ro, ci = k.mirrored(graph)
    want, r = _ref(n, ro, ci)
    p = ga.C4Problem().init(n, ro, ci)
    got = _run(p, strategy=ga.C4_GLOBAL, scratch_mib=2)  # 2 MiB / 1.2 MB: one row
    p.close()
    _same(got, want, "one counter row")
    assert got[3]["global_vertices"] == 2 and want[2] == comb(200, 2)


# ---------------- the graph's form, the options ----------------

def test_input_forms():
    rng = np.random.default_rng(11)
    a, b = np.nonzero(np.triu(rng.random((140, 140)) < 0.12, 1))
    graph = (150, a, b)  # G(n, p) on the first 140 vertices; the last 10 are isolated
    forms = k.entry_forms(graph, rng)
    want, r = _ref(150, *forms["mirrored"])
    assert want[2] > 0 and not want[0][140:].any()
    for name, (ro, ci) in forms.items():
        p = ga.C4Problem().init(150, ro, ci)
        got = _run(p, **LOW)
        src, dst = p.edges()
        p.close()
        _same(got, want, name)
        assert np.array_equal(src, r["src"]) and np.array_equal(dst, r["dst"]), name
    cycles, total = ga.gunrock_four_cycles(3, np.array([0, 1, 3, 3], np.int32), np.array([0, 1, 1], np.int32))  # only self-loops
    assert cycles.tolist() == [0, 0, 0] and total == 0


def test_without_edges(rmat10):
    n, ro, ci, want, r = rmat10
    p = ga.C4Problem().init(n, ro, ci)
    got = _run(p, edges=0, **LOW)
    _same(got, want, "edges = 0")
    assert got[1] is None and p.device_results()["edge_cycles"] is None
    with pytest.raises(RuntimeError, match="code -1"):
        p.extract_edges()
    _same(_run(p, **LOW), want, "edges = 1 behind edges = 0")
    _same(_run(p, edges=0), want, "edges = 0 behind edges = 1")
    with pytest.raises(RuntimeError, match="code -1"):
        p.extract_edges()
    p.close()


def test_overflow_is_refused():
    n, ro, ci = k.mirrored(k.complete_bipartite(8, 8))
    want, r = _ref(n, ro, ci)
    assert r["bound"] == 784.0 == want[2]  # every degree 8: rank = id, the far side's vertex j has 8 j wedges under 8 neighbours
    p = ga.C4Problem().init(n, ro, ci)
    assert p.stats()["bound"] == 784.0
    assert p.set_option("count_limit", 784) == 0
    p.reset()
    with pytest.raises(ga.C4Overflow):
        p.enact()
    assert p.stats()["bound"] == 784.0 and p.stats()["kernel_launches"] == 0
    for call in (p.extract, p.extract_edges):
        with pytest.raises(RuntimeError, match=NOT_READY):
            call()
    _same(_run(p, count_limit=785), want, "count_limit = bound + 1")
    assert p.set_option("count_limit", 784) == 0
    with pytest.raises(ga.C4Overflow):  # refused again, and without a reset: the result is gone
        p.enact()
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.extract()
    _same(_run(p), want, "the default limit behind a refusal")
    _same(_run(p), (k.complete_bipartite_counts(8, 8)[1], k.complete_bipartite_counts(8, 8)[2], 784))
    for bad in (0, -1, 2.0 ** 63):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option("count_limit", bad)
    p.close()


def test_handle_protocol(rmat10):
    n, ro, ci, want, r = rmat10
    p = ga.C4Problem(instrument=True).init(n, ro, ci)
    first = _run(p)
    second = _run(p)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2]
    _same(first, want)
    assert second[3]["kernel_ms"] > 0 and second[3]["build_ms"] > 0 and second[3]["kernel_launches"] >= 1
    assert p.enact() > 0  # no reset between: Enact clears what the last one wrote
    third = p.extract() + (p.extract_edges(),)
    _same((third[0], third[2], third[1]), want, "a second enact without a reset")
    p.reset()
    for call in (p.extract, p.extract_edges):  # a reset leaves no result
        with pytest.raises(RuntimeError, match=NOT_READY):
            call()
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(n, ro, ci)
    assert p.set_option("no_such_option", 1) == 1
    for name, bad in (("strategy", 5), ("strategy", -1), ("lane_max_wedges", 33), ("lane_max_wedges", -1), ("table_slots", 32),
                      ("table_slots", 2048), ("table_slots", 96), ("block_slots", 128), ("block_slots", 16384), ("block_slots", 300),
                      ("scratch_mib", 0), ("edges", 2), ("edges", -1)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, bad)
    for name, good in (("lane_max_wedges", 0), ("lane_max_wedges", 32), ("table_slots", 64), ("block_slots", 256), ("scratch_mib", 1)):
        assert p.set_option(name, good) == 0
    _same(_run(p, lane_max_wedges=0), want, "no LANE regime")
    _same(_run(p, lane_max_wedges=32), want, "the largest LANE regime")
    p.close()
    p.close()  # twice is safe
    p = ga.C4Problem()
    for call in (p.reset, p.enact, p.extract, p.extract_edges, p.edges):  # before Init: an error code, nothing touched
        with pytest.raises(RuntimeError, match=NOT_READY):
            call()
    p.init(n, ro, ci)  # ... and the handle is still usable
    _same(_run(p), want, "behind refused calls")
    p.close()
    p = ga.C4Problem()
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that decrease
        p.init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.enact()
    p.close()
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.C4Problem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -1"):
        ga.C4Problem().init(0, np.array([0], np.int32), np.array([], np.int32))


def test_init_device_and_device_results():
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(10)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    h_ro, h_ci = ro.cpu().numpy(), ci.cpu().numpy()
    p = ga.C4Problem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    q = ga.C4Problem().init(n, h_ro, h_ci)
    got, host = _run(p, **LOW), _run(q, **LOW)
    d = p.device_results()
    M = p.simple_edges
    a, b = simple_edges(n, h_ro, h_ci)
    assert M == a.shape[0] == got[3]["simple_edges"]
    assert np.array_equal(devgraph.as_tensor(d["cycles"], n, "<i8").cpu().numpy(), got[0])
    assert np.array_equal(devgraph.as_tensor(d["edge_cycles"], M, "<i8").cpu().numpy(), got[1])
    assert np.array_equal(devgraph.as_tensor(d["src"], M, "<i4").cpu().numpy(), a) and np.array_equal(devgraph.as_tensor(d["dst"], M, "<i4").cpu().numpy(), b)
    _same(got, host[:3], "device against host")
    _same(got, k.dense(n, h_ro, h_ci), "device against the dense form")
    p.close()
    q.close()
