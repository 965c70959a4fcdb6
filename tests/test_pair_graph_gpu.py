"""The build every undirected family shares (graphio/pair_graph.hpp), through what the Python API shows of it: truss, BCC, max-flow
and matching must return the same canonical pairs, equal to _bcc_checker.simple_edges, and the mirrored rows must carry the truss
supports and the contraction -- on the smallest shapes at which a step of the build can go wrong.  And one malformed CSR for all
nine families that validate their input the same way."""
import functools

import numpy as np
import pytest

import gunrockinst_amd as ga

import _bcc_checker as bk
import _matching_checker as hk
import _truss_checker as tk

pytestmark = pytest.mark.gpu

TILE = 4096  # graphio::kScanTile, and graphio::kSortTile: the elements one workgroup of the scan, and of the radix sort, takes


def _raw(n, rows, cols, shuffle=None):
    """the entries as they are: one-way, loops and duplicates kept"""
    ro, ci, _ = hk.csr_from_pairs(n, rows, cols, mirror=False, shuffle=shuffle)
    return n, ro, ci


def _boundary(n):
    """the last two vertices joined, in a graph of n: the key of (n - 2, n - 1) is the largest there is"""
    rows = np.array([n - 2, 0, 1, n - 1, 0])
    cols = np.array([n - 1, n - 1, n - 2, 1, 1])
    return _raw(n, rows, cols)


@functools.lru_cache(maxsize=None)
def _random_coo(entries):
    rng = np.random.default_rng(entries)
    n = 300
    return _raw(n, rng.integers(0, n, entries), rng.integers(0, n, entries), shuffle=rng)


def _twice_both_ways():
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, 40, 120), rng.integers(0, 40, 120)
    rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    return _raw(40, np.concatenate([rows, rows]), np.concatenate([cols, cols]))


def _unsorted_rows():
    rng = np.random.default_rng(6)
    return _raw(50, rng.integers(0, 50, 400), rng.integers(0, 50, 400), shuffle=rng)


CASES = {
    "one_vertex": lambda: (1, np.array([0, 0], np.int32), np.array([], np.int32)),
    "one_one_way_entry": lambda: _raw(2, [0], [1]),
    "one_one_way_entry_down": lambda: _raw(2, [1], [0]),
    "loops_only": lambda: _raw(3, [0, 1, 2, 1], [0, 1, 2, 1]),
    "loops_only_last_vertex_power_of_two": lambda: _raw(4, [3, 0, 3], [3, 0, 3]),  # (3 << 2 | 3) is the sentinel itself
    "loop_on_last_vertex_beside_edges": lambda: _raw(4, [0, 3, 2, 3], [1, 3, 3, 2]),
    "n64": lambda: _boundary(64),  # col_bits 6
    "n65": lambda: _boundary(65),  # col_bits 7
    "both_ways_and_duplicates": _twice_both_ways,
    "unsorted_rows": _unsorted_rows,
    "isolated_last_vertex": lambda: _raw(9, [0, 1, 2, 0, 7, 6], [1, 2, 0, 3, 6, 5]),
    "tile_minus_1": lambda: _random_coo(TILE - 1),
    "tile": lambda: _random_coo(TILE),
    "tile_plus_1": lambda: _random_coo(TILE + 1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_four_families_build_the_same_pairs_and_rows(name):
    n, ro, ci = CASES[name]()
    a, b = bk.simple_edges(n, ro, ci)
    M = a.shape[0]

    truss = ga.TrussProblem().init(n, ro, ci)
    bcc = ga.BccProblem().init(n, ro, ci)
    flow = ga.MaxflowProblem().init(n, ro, ci, np.ones(ci.shape[0], np.int32))
    if n >= 2:
        flow.reset(0, n - 1)
    match = ga.MatchingProblem().init(n, ro, ci)
    try:
        for what, (src, dst) in (("truss", truss.edges()), ("bcc", bcc.edges()), ("maxflow", flow.pairs()[:2]), ("matching", match.pairs()[:2])):
            assert src.dtype == np.int32 and np.array_equal(src, a) and np.array_equal(dst, b), what + ": the pairs differ from simple_edges"
        assert truss.stats()["simple_edges"] == truss.simple_edges == M
        assert bcc.stats()["simple_edges"] == bcc.simple_edges == M
        assert flow.stats()["pairs"] == flow.num_pairs == M
        assert match.stats()["pairs"] == M

        # the mirrored rows, through what reads them: the support pass and the contraction
        tri = tk.triangles(n, a.astype(np.int64), b.astype(np.int64))
        support, total = truss.support()
        assert np.array_equal(support, tk.support_of(M, tri)) and total == tri.shape[0], "the supports differ from the checker"

        _, _, pw, ref, _ = hk.solve(n, ro, ci, None, 0)
        match.reset()
        match.enact()
        assert np.array_equal(match.extract()["mate"], ref["mate"])
        want = hk.contract(n, a, b, pw, ref["mate"])
        nc, ne = match.contract()
        assert (nc, ne) == (want[1], want[3].shape[0]) and hk.same_coarse(match.coarse_extract(), want), "the coarse graph differs from the checker"
    finally:
        for p in (truss, bcc, flow, match):
            p.close()


FAMILIES = ("TcProblem", "KcoreProblem", "TrussProblem", "MisProblem", "MsbfsProblem", "SccProblem", "BccProblem", "MaxflowProblem",
            "MatchingProblem")


@pytest.mark.parametrize("family", FAMILIES)
def test_every_family_rejects_a_column_equal_to_nodes(family):
    good = (2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    p = getattr(ga, family)()
    try:
        with pytest.raises(RuntimeError, match="code -2"):
            p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 2], np.int32))
        with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
            p.init(*good)
    finally:
        p.close()
