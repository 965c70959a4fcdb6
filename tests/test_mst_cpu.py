"""Minimum spanning forest without a GPU: the Kruskal checker (tests/_mst_checker.py) on hand-worked cases and against scipy,
and the grx_mst_* C ABI declared in the header, exported by libgunrock.so and bound by the Python package."""
import os
import re

import numpy as np
import pytest

import gunrockinst_amd as ga
from gunrockinst_amd import capi

from _mst_checker import components, kruskal, min_reduced_pairs, scipy_forest_weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr(nodes, triples):
    """entries in the order given, grouped by row (stable): the CSR index of each entry is predictable"""
    triples = sorted(triples, key=lambda t: t[0])
    ro = np.zeros(nodes + 1, np.int32)
    for u, _, _ in triples:
        ro[u + 1] += 1
    ro = np.cumsum(ro).astype(np.int32)
    ci = np.array([t[1] for t in triples], np.int32)
    w = np.array([t[2] for t in triples], np.int32)
    return ro, ci, w


def test_ties_take_the_lower_csr_index():
    # triangle, all weights 1, stored once each: entries 0:(0,1) 1:(0,2) 2:(1,2) -> the first two win
    ro, ci, w = _csr(3, [(0, 1, 1), (0, 2, 1), (1, 2, 1)])
    sel, total, count = kruskal(3, ro, ci, w)
    assert sel.tolist() == [1, 1, 0] and total == 2 and count == 2
    # mirrored with equal weights: the chosen copy of every forest edge is the u < v entry
    ro, ci, w = _csr(3, [(0, 1, 1), (0, 2, 1), (1, 0, 1), (1, 2, 1), (2, 0, 1), (2, 1, 1)])
    sel, _, count = kruskal(3, ro, ci, w)
    assert count == 2
    rows = np.repeat(np.arange(3), np.diff(ro))
    assert (rows[sel == 1] < ci[sel == 1]).all() and sel.tolist() == [1, 1, 0, 0, 0, 0]


def test_parallel_edges_and_self_loops():
    # two parallel copies of {0, 1} with weights 5 and 3 and a self-loop of weight -100: the lighter copy, no loop
    ro, ci, w = _csr(2, [(0, 1, 5), (0, 0, -100), (1, 0, 3)])
    sel, total, count = kruskal(2, ro, ci, w)
    assert sel.tolist() == [0, 0, 1] and total == 3 and count == 1
    # equal-weight duplicates: the earlier entry
    ro, ci, w = _csr(2, [(0, 1, 7), (0, 1, 7)])
    assert kruskal(2, ro, ci, w)[0].tolist() == [1, 0]


def test_negative_and_extreme_weights():
    imin, imax = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    # square 0-1-2-3-0 plus the diagonal 0-2
    ro, ci, w = _csr(4, [(0, 1, imax), (1, 2, -5), (2, 3, imin), (3, 0, 0), (0, 2, imax)])
    sel, total, count = kruskal(4, ro, ci, w)
    # rows: 0 -> entries 0:(0,1,max) 1:(0,2,max); 1 -> 2:(1,2,-5); 2 -> 3:(2,3,min); 3 -> 4:(3,0,0)
    # min, -5 and 0 already span the four vertices: neither INT_MAX entry is taken
    assert sel.tolist() == [0, 0, 1, 1, 1]
    assert total == imin - 5 + 0 and count == 3
    # without the 0 edge, the first INT_MAX entry (index 0) wins the tie with the diagonal
    ro, ci, w = _csr(4, [(0, 1, imax), (1, 2, -5), (2, 3, imin), (0, 2, imax)])
    sel, total, count = kruskal(4, ro, ci, w)
    assert sel.tolist() == [1, 0, 1, 1] and total == imax - 5 + imin and count == 3


def test_forest_with_isolated_vertices():
    # two components {0, 1, 2} and {4, 5}; vertices 3 and 6 isolated (3 has only a self-loop)
    ro, ci, w = _csr(7, [(0, 1, 4), (1, 2, 2), (2, 0, 3), (3, 3, 1), (4, 5, 9), (5, 4, 1)])
    sel, total, count = kruskal(7, ro, ci, w)
    assert count == 3 and total == 2 + 3 + 1
    assert 7 - count == components(7, [0, 1, 2, 4, 5], [1, 2, 0, 5, 4]) == 4


def test_empty_and_single_vertex():
    assert kruskal(1, [0, 0], [], [])[1:] == (0, 0)
    assert kruskal(5, [0] * 6, [], [])[1:] == (0, 0)
    assert components(5, [], []) == 5


@pytest.mark.parametrize("seed", range(6))
def test_checker_matches_scipy_total_weight(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 400))
    m = int(rng.integers(0, 4 * n))
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    ro = np.searchsorted(rows, np.arange(n + 1)).astype(np.int32)
    w = (rng.permutation(m) + 1).astype(np.int32)  # distinct, positive
    sel, total, count = kruskal(n, ro, cols, w)
    assert total == scipy_forest_weight(n, ro, cols, w)
    assert count == n - components(n, rows, cols)
    chosen = sel == 1
    assert components(n, rows[chosen], cols[chosen]) == n - count  # acyclic
    lo, hi, wmin = min_reduced_pairs(ro, cols, w)
    assert (lo < hi).all() and wmin.shape == lo.shape


def _declared_mst():
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(grx_mst_[a-z0-9_]+)\s*\(", text))


def test_mst_c_abi_declared_exported_and_bound():
    wanted = {"grx_mst_create", "grx_mst_init", "grx_mst_init_device", "grx_mst_reset", "grx_mst_enact", "grx_mst_stats",
              "grx_mst_extract", "grx_mst_device_results", "grx_mst_destroy"}
    assert wanted <= _declared_mst()
    L = ga.lib()
    for name in sorted(_declared_mst()):
        assert hasattr(L, name), name
        assert name in capi.exported_symbols(), name
    assert callable(ga.gunrock_mst) and hasattr(ga.MstProblem, "init_device")
    assert "gunrock_mst" in ga.__all__ and "MstProblem" in ga.__all__
    # MST stays out of the reference-equal gunrock.h
    assert "mst" not in open(os.path.join(ROOT, "include", "gunrock", "gunrock.h")).read().lower()
