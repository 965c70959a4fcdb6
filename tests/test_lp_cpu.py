"""The label-propagation checker (tests/_lp_checker.py) on the CPU: its two forms agree on every case, the hand cases come out as
stated, the summary agrees with networkx's modularity; the package exports the family's names (no GPU needed)."""
import os

import numpy as np
import pytest

from oracle import gr_oracle as o

import _lp_checker as k


def _pairs(n, ro, ci, w=None):
    return k.pairs_of(n, ro, ci, w)


def _communities(r):
    return k.community_of(r["labels"])[1]


def test_k33():
    ro, ci = k.complete_bipartite(3, 3)
    a, b, w = _pairs(6, ro, ci)
    r = k.solve(6, a, b, w, k.SYNC)
    assert (r["state"], r["rounds"], _communities(r)) == (k.PERIOD2, 3, 2)
    r = k.solve(6, a, b, w, k.CLASSES, classes=[0, 0, 0, 1, 1, 1])
    assert (r["state"], r["rounds"], _communities(r)) == (k.CONVERGED, 1, 1)


def test_star():
    ro, ci = k.star(64)
    a, b, w = _pairs(65, ro, ci)
    r = k.solve(65, a, b, w, k.SYNC)
    assert (r["state"], r["rounds"]) == (k.PERIOD2, 3)


@pytest.mark.parametrize("c,s", [(5, 4), (6, 8), (64, 5)])
def test_clique_rings(c, s):
    n = c * s
    ro, ci = k.clique_ring(c, s)
    a, b, w = _pairs(n, ro, ci)
    want = np.repeat(np.arange(c), s)
    sync = k.solve(n, a, b, w, k.SYNC)
    assert (sync["state"], sync["rounds"]) == (k.CONVERGED, 2)
    classes = k.greedy_classes(n, a, b)
    assert k.is_proper(a, b, classes)
    for r in (sync, k.solve(n, a, b, w, k.CLASSES, classes=classes)):
        assert r["state"] == k.CONVERGED
        community, count = k.community_of(r["labels"])
        assert count == c and np.array_equal(community, want)


def test_unit_path():
    n = 2001
    ro, ci, _ = k.path(n)
    a, b, w = _pairs(n, ro, ci)
    r = k.solve(n, a, b, w, k.SYNC)
    assert (r["state"], r["rounds"], r["entries_read"]) == (k.PERIOD2, 2001, 8004000)
    r = k.solve(n, a, b, w, k.CLASSES, classes=np.arange(n) % 2)
    assert (r["state"], r["rounds"], _communities(r), r["entries_read"]) == (k.CONVERGED, 1, 1000, 4000)
    capped = k.solve(n, a, b, w, k.SYNC, max_rounds=3, keep=True)
    assert (capped["state"], capped["rounds"]) == (k.CAPPED, 3) and np.array_equal(capped["labels"], capped["history"][2])


def test_rising_path_needs_a_round_per_pair():
    n = 2001
    ro, ci, w = k.path(n, np.arange(1, n))
    a, b, w = _pairs(n, ro, ci, w)
    r = k.solve(n, a, b, w, k.CLASSES, classes=np.arange(n) % 2)
    assert (r["state"], r["rounds"], _communities(r), r["entries_read"]) == (k.CONVERGED, 1000, 1, 2002999)


def test_goldens(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    a, b, w = _pairs(g.nodes, g.row_offsets, g.col_indices)
    r = k.solve(g.nodes, a, b, w, k.SYNC)
    assert (a.shape[0], r["state"], r["rounds"], _communities(r), r["entries_read"]) == (170, k.CONVERGED, 4, 1, 1363)
    g = o.build_market(os.path.join(golden_dir, "bips98_606.mtx"), undirected=True)
    a, b, w = _pairs(g.nodes, g.row_offsets, g.col_indices)
    r = k.solve(g.nodes, a, b, w, k.SYNC)
    assert (a.shape[0], r["state"], r["rounds"], _communities(r), r["entries_read"]) == (15190, k.PERIOD2, 20, 1679, 257350)


def test_rmat():
    g = o.rmat_seeded(12, 8 << 12)
    a, b, w = _pairs(g.nodes, g.row_offsets, g.col_indices)
    r = k.solve(g.nodes, a, b, w, k.SYNC)
    assert (a.shape[0], r["state"], r["rounds"], _communities(r), r["entries_read"]) == (27791, k.CONVERGED, 4, 982, 168981)


def test_tie_rule():
    # vertex 0 with neighbours 1, 2, 3: the current label tied with a smaller one keeps; absent, the smallest wins; weights overturn counts
    ro, ci = k.star(3)
    a, b, w = _pairs(4, ro, ci)
    assert k.solve(4, a, b, w, k.SYNC, start=[3, 3, 1, 2], max_rounds=1)["labels"][0] == 3   # 3, 1, 2 tied at 1: 3 is current
    assert k.solve(4, a, b, w, k.SYNC, start=[0, 3, 1, 2], max_rounds=1)["labels"][0] == 1   # 0 is absent: the smallest of 3, 1, 2
    ro, ci, w = k.csr_from_pairs(4, [0, 0, 0], [1, 2, 3], [1, 1, 3])
    a, b, w = _pairs(4, ro, ci, w)
    assert k.solve(4, a, b, w, k.SYNC, start=[0, 1, 1, 2], max_rounds=1)["labels"][0] == 2   # 1 + 1 against 3


def test_int64_scores():
    ro, ci, w = k.csr_from_pairs(5, [0, 0, 0, 0], [1, 2, 3, 4], [k.INT_MAX, k.INT_MAX, k.INT_MAX, k.INT_MAX])
    a, b, w = _pairs(5, ro, ci, w)
    # labels 4, 4, 4 carry 3 * INT_MAX (beyond int32 and uint32) against 1 * INT_MAX for label 1
    assert k.solve(5, a, b, w, k.SYNC, start=[0, 1, 4, 4, 4], max_rounds=1)["labels"][0] == 4


def test_summary_and_modularity(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    w = k.mod7_weights(g.nodes, g.row_offsets, g.col_indices)
    a, b, pw = _pairs(g.nodes, g.row_offsets, g.col_indices, w)
    classes = k.greedy_classes(g.nodes, a, b)
    assert k.is_proper(a, b, classes) and not k.is_proper(a, b, np.zeros(g.nodes, np.int32))
    for r in (k.solve(g.nodes, a, b, pw, k.CLASSES, classes=classes), k.solve(g.nodes, a, b, pw, k.SYNC, max_rounds=1)):
        s = k.summary_of(g.nodes, a, b, pw, r["labels"])
        assert int(s["size"].sum()) == g.nodes and int(s["volume"].sum()) == 2 * s["W"] and int(s["internal"].sum()) <= s["W"]
        assert abs(k.modularity(s) - k.networkx_modularity(g.nodes, a, b, pw, r["labels"])) < 1e-12


def test_names_are_exported():
    import gunrockinst_amd as ga
    names = ("LpProblem", "gunrock_label_propagation", "modularity_from_sums", "LP_SYNC", "LP_CLASSES", "LP_AUTO", "LP_LANE", "LP_WAVE",
             "LP_BLOCK", "LP_CONVERGED", "LP_PERIOD2", "LP_CAPPED", "LP_BAD_CLASSES")
    for name in names:
        assert name in ga.__all__ and hasattr(ga, name), name
    assert (ga.LP_SYNC, ga.LP_CLASSES) == (k.SYNC, k.CLASSES) and (ga.LP_CONVERGED, ga.LP_PERIOD2, ga.LP_CAPPED) == (k.CONVERGED, k.PERIOD2, k.CAPPED)
    assert (ga.LP_AUTO, ga.LP_LANE, ga.LP_WAVE, ga.LP_BLOCK) == (0, 1, 2, 3) and ga.LP_BAD_CLASSES == -8
    assert issubclass(ga.LpProblem, ga.capi._Handle)
    assert ga.modularity_from_sums([3, 3], [7, 7], 7) == pytest.approx(6 / 7 - 0.5)
