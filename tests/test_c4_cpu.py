"""4-cycle counting without a GPU: the two forms of tests/_c4_checker.py against each other, against literals computed once and against
the closed forms, so that the GPU tests compare the library with something that has been checked itself."""
import os
from math import comb

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _c4_checker as k
from _tc_checker import simple_edges


def _agree(n, ro, ci):
    cycles, edge, total = k.dense(n, ro, ci)
    r = k.ranked(n, ro, ci)
    assert np.array_equal(cycles, r["cycles"]) and np.array_equal(edge, r["edge_cycles"]) and total == r["total"]
    assert int(cycles.sum()) == int(edge.sum()) == 4 * total
    assert r["bound"] >= total and (not cycles.size or r["bound"] >= cycles.max()) and (not edge.size or r["bound"] >= edge.max())
    a, b = simple_edges(n, ro, ci)
    assert np.array_equal(r["src"], a) and np.array_equal(r["dst"], b)
    return cycles, edge, total, r


def test_chesapeake(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    cycles, edge, total, r = _agree(g.nodes, g.row_offsets, g.col_indices)
    assert (total, int(cycles.max()), int(edge.max()), r["wedges"]) == (1762, 944, 94, 692)


@pytest.mark.parametrize("seed", range(6))
def test_random_multigraphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 120))
    m = int(rng.integers(0, 6 * n))
    graph = (n, rng.integers(0, n, m), rng.integers(0, n, m))  # loops and duplicates included
    results = [_agree(n, ro, ci) for ro, ci in k.entry_forms(graph, rng).values()]
    for cycles, edge, total, _ in results[1:]:
        assert np.array_equal(cycles, results[0][0]) and np.array_equal(edge, results[0][1]) and total == results[0][2]


def _closed(graph, total, per_vertex=None, per_edge=None):
    n, ro, ci = k.mirrored(graph)
    cycles, edge, got, _ = _agree(n, ro, ci)
    assert got == total
    if per_vertex is not None:
        assert np.array_equal(cycles, per_vertex)
    if per_edge is not None:
        assert np.array_equal(edge, per_edge)


def test_closed_forms():
    for p, q in ((3, 5), (1, 7), (2, 2), (8, 8), (4, 9)):
        _closed(k.complete_bipartite(p, q), *k.complete_bipartite_counts(p, q))
    assert k.complete_bipartite_counts(3, 5)[0] == 30 and k.complete_bipartite_counts(1, 7)[0] == 0
    for n in (1, 2, 3, 4, 5, 6, 33, 65):
        _closed(k.complete(n), *k.complete_counts(n))
    assert k.complete_counts(4)[0] == 3 and k.complete_counts(6) [0] == 45
    for d in (1, 2, 3, 4, 6):
        _closed(k.hypercube(d), *k.hypercube_counts(d))
    assert k.hypercube_counts(4)[0] == 24
    for p, q in ((1, 9), (2, 2), (5, 7), (6, 3)):
        _closed(k.grid(p, q), k.grid_total(p, q))
    for t in (1, 2, 3, 17, 130):
        _closed(k.theta(t), k.theta_total(t))
        _closed(k.spider(t), 0)


def test_graphs_without_a_4_cycle():
    for graph in (k.cycle(5), k.cycle(3), k.cycle(7), k.petersen(), k.random_tree(200, 1), k.random_tree(17, 2), k.edgeless(9), k.edgeless(1)):
        n, ro, ci = k.mirrored(graph)
        cycles, edge, total, _ = _agree(n, ro, ci)
        assert total == 0 and not cycles.any() and not edge.any()
    _closed(k.cycle(4), 1, np.ones(4, np.int64), np.ones(4, np.int64))


def test_disjoint_unions_add():
    parts = [k.complete_bipartite(3, 5), k.petersen(), k.complete(6), k.theta(9), k.spider(9), k.hypercube(3)]
    totals = [30, 0, 45, 36, 0, 6]
    n, ro, ci = k.mirrored(k.union(*parts))
    cycles, edge, total, _ = _agree(n, ro, ci)
    assert total == sum(totals)
    at = 0
    for (size, _, _), want in zip(parts, totals):
        assert int(cycles[at:at + size].sum()) == 4 * want
        at += size


def test_theta_with_spider_has_the_hub_the_table_tests_need():
    """theta(t) + spider(t): the highest-ranked pole of the theta has W = t wedges into one end, the centre of the spider W = t wedges
    into t ends (its knees have degree 2 and rank below it for t >= 3)"""
    for t in (3, 4, 5, 31, 32, 33, 127, 128, 129):
        n, ro, ci = k.mirrored(k.union(k.theta(t), k.spider(t)))
        r = k.ranked(n, ro, ci)
        assert sorted(r["W"][r["W"] >= 2].tolist()) == [t, t] and r["total"] == comb(t, 2), t
        assert r["W"][1] == t and r["W"][2 + t] == t  # the second pole (equal degree, larger id) and the spider's centre


def test_exports():
    names = ("C4Problem", "C4Overflow", "gunrock_four_cycles", "gunrock_edge_four_cycles", "C4_AUTO", "C4_LANE", "C4_WAVE", "C4_BLOCK",
             "C4_GLOBAL", "C4_OVERFLOW")
    for name in names:
        assert name in ga.__all__ and hasattr(ga, name), name
    assert (ga.C4_AUTO, ga.C4_LANE, ga.C4_WAVE, ga.C4_BLOCK, ga.C4_GLOBAL, ga.C4_OVERFLOW) == (0, 1, 2, 3, 4, -7)
    assert issubclass(ga.C4Overflow, ArithmeticError)
