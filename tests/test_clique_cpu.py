"""The k-clique checker (tests/_clique_checker.py) on the CPU: its recursion agrees with its closed forms, with the triangle checker
for k = 3 and with the identities every count obeys; the package exports the family's names (no GPU needed)."""
import os
from math import comb

import numpy as np
import pytest

from oracle import gr_oracle as o

from _clique_checker import (bipartite_graph, complete_counts, complete_graph, count, elementary, grid_graph, multipartite_counts,
                             multipartite_graph, tree_graph, union, work_estimate)
from _tc_checker import csr_of, oriented

KS = (3, 4, 5, 6)


def _same(got, want):
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and got[1] == want[1]


@pytest.mark.parametrize("n", [1, 2, 5, 6, 9, 13])
def test_complete_graphs(n):
    ro, ci = complete_graph(n)
    for k in KS:
        _same(count(n, ro, ci, k), complete_counts(n, k))
        assert work_estimate(n, ro, ci, k) == sum(comb(n, j) for j in range(2, k))  # sum over r < n of C(r, j - 1)


@pytest.mark.parametrize("parts", [(1, 1, 1), (2, 3, 4), (3, 3, 3, 3), (1, 2, 3, 4, 5), (2, 2, 2, 2, 2, 2, 5)])
def test_complete_multipartite(parts):
    n, (ro, ci) = multipartite_graph(parts)
    assert elementary(parts, 1) == n and elementary(parts, len(parts) + 1) == 0
    for k in KS:
        got = count(n, ro, ci, k)
        _same(got, multipartite_counts(parts, k))
        assert int(got[0].sum()) == k * got[1]
        assert work_estimate(n, ro, ci, k) >= sum(elementary(parts, j) for j in range(2, k))  # the cliques the recursion walks


def test_disjoint_unions_add():
    pieces = [(7, complete_graph(7)), multipartite_graph((2, 3, 4)), grid_graph(3), (6, complete_graph(6))]
    n, (ro, ci) = union(pieces)
    for k in KS:
        want = [complete_counts(7, k), multipartite_counts((2, 3, 4), k), (np.zeros(9, np.int64), 0), complete_counts(6, k)]
        _same(count(n, ro, ci, k), (np.concatenate([w[0] for w in want]), sum(w[1] for w in want)))


def test_triangle_free_graphs_have_no_cliques():
    for n, (ro, ci) in (grid_graph(7), tree_graph(60, 3), bipartite_graph(9, 11, 0.5, 4)):
        for k in KS:
            got = count(n, ro, ci, k)
            assert not got[0].any() and got[1] == 0


def test_k3_is_the_triangle_checker(golden_dir):
    graphs = [o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True), o.rmat_seeded(8, 8 << 8),
              o.rmat_seeded(9, 4 << 9, undirected=False)]
    for g in graphs:
        tri, total, _, _, _ = oriented(g.nodes, g.row_offsets, g.col_indices)
        _same(count(g.nodes, g.row_offsets, g.col_indices, 3), (tri, total))
    # K_4 and a loose vertex from unsorted rows, duplicates, self-loops and one-way entries
    ro, ci = csr_of(5, [0, 0, 0, 1, 1, 2, 3, 3, 4], [3, 1, 1, 2, 1, 0, 2, 1, 4])
    tri, total, _, _, _ = oriented(5, ro, ci)
    _same(count(5, ro, ci, 3), (tri, total))
    assert total == 4 and count(5, ro, ci, 4)[0].tolist() == [1, 1, 1, 1, 0]


def test_chesapeake_literals(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    totals = []
    for k in KS:
        cl, total = count(g.nodes, g.row_offsets, g.col_indices, k)
        assert int(cl.sum()) == k * total
        totals.append(total)
    assert totals[0] == 194 and totals[1] > 0  # (194: tests/test_tc_cpu.py's literal)
    # a k-clique holds k (k - 1)-cliques, and a (k - 1)-clique lies in at most n - k + 1 k-cliques
    for i in range(1, len(totals)):
        assert KS[i] * totals[i] <= (g.nodes - KS[i] + 1) * totals[i - 1]


def test_names_are_exported():
    import gunrockinst_amd as ga
    for name in ("CliqueProblem", "gunrock_cliques", "CliqueOverflow", "CLIQUE_AUTO", "CLIQUE_BITMAP", "CLIQUE_LIST", "CLIQUE_OVERFLOW"):
        assert name in ga.__all__ and hasattr(ga, name), name
    assert (ga.CLIQUE_AUTO, ga.CLIQUE_BITMAP, ga.CLIQUE_LIST) == (0, 1, 2)
    assert issubclass(ga.CliqueOverflow, ArithmeticError) and issubclass(ga.CliqueProblem, ga.capi._Handle)
