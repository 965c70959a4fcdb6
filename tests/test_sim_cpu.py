"""Vertex similarity without a GPU: the two forms of tests/_sim_checker.py against each other, against networkx where it is installed,
against closed forms and against identities that tie the common-neighbour counts to the triangle supports, the triangles and the
4-cycles of the golden graphs, so that the GPU tests compare the library with something that has been checked itself."""
import os
from fractions import Fraction
from math import comb

import numpy as np
import pytest

from oracle import gr_oracle as o

import _c4_checker as ck
import _sim_checker as k
import _truss_checker as tk
from _tc_checker import oriented, simple_edges


def _agree(n, ro, ci, sources=None, ks=(1, 3, 64)):
    """both forms on all-pairs-of-a-sample and on the top-k of `sources` (default: all), every metric; returns them"""
    d, s = k.Dense(n, ro, ci), k.Sets(n, ro, ci)
    assert np.array_equal(d.wd, s.wd)
    rng = np.random.default_rng(n)
    u, v = rng.integers(0, n, 200), rng.integers(0, n, 200)
    a, b = simple_edges(n, ro, ci)
    u, v = np.concatenate([u, a, b, np.arange(n)]), np.concatenate([v, b, a, np.arange(n)])
    sources = np.arange(n) if sources is None else sources
    for metric in k.METRICS:
        assert k.same(d.pairs(u, v, metric), s.pairs(u, v, metric)) is None
        for skip in (False, True):
            for kk in ks:
                assert k.same(d.topk(sources, kk, metric, skip), s.topk(sources, kk, metric, skip)) is None, (metric, skip, kk)
    return d, s


def _golden(golden_dir, name):
    g = o.build_market(os.path.join(golden_dir, name + ".mtx"), undirected=True)
    return g.nodes, g.row_offsets, g.col_indices


@pytest.mark.parametrize("name", ["chesapeake", "test_bc"])
def test_forms_agree_on_small_goldens(golden_dir, name):
    _agree(*_golden(golden_dir, name))


@pytest.mark.parametrize("seed", range(4))
def test_random_multigraphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 90))
    m = int(rng.integers(0, 5 * n))
    graph = (n, rng.integers(0, n, m), rng.integers(0, n, m))  # loops and duplicates included
    firsts = []
    for ro, ci in ck.entry_forms(graph, rng).values():
        d, _ = _agree(n, ro, ci, ks=(2,))
        firsts.append(d.topk(np.arange(n), 5, k.JACCARD))
    for other in firsts[1:]:
        assert k.same(other, firsts[0]) is None


def test_networkx_is_a_third_witness(golden_dir):
    n, ro, ci = _golden(golden_dir, "chesapeake")
    u, v = np.divmod(np.arange(n * n), n)
    witness = k.nx_pairs(n, ro, ci, u, v)
    if witness is None:
        pytest.skip("networkx is not installed")
    d = k.Dense(n, ro, ci)
    assert d.pairs(u, v, k.COMMON)["common"].tolist() == witness[0]
    assert d.pairs(u, v, k.JACCARD)["score"].tolist() == witness[1]


def test_fraction_and_score():
    assert k.fraction(k.COMMON, 3, 5, 7) == (3, 1) and k.fraction(k.JACCARD, 3, 5, 7) == (3, 9)
    assert k.fraction(k.OVERLAP, 3, 5, 7) == (3, 5) and k.fraction(k.SORENSEN, 3, 5, 7) == (6, 12)
    assert k.fraction(k.JACCARD, 0, 0, 0) == (0, 0) and k.fraction(k.OVERLAP, 0, 0, 9) == (0, 0) and k.fraction(k.SORENSEN, 0, 0, 0) == (0, 0)
    assert k.fraction(k.JACCARD, 0, 0, 9) == (0, 9) and k.fraction(k.COMMON, 0, 0, 0) == (0, 1)
    assert k.score_of([1, 0, 2], [3, 0, 6]).tolist() == [1 / 3, 0.0, 2 / 6]


def _mirrored(graph):
    return ck.mirrored(graph)


def test_complete_graphs():
    for n in (2, 3, 5, 9):
        d, _ = _agree(*_mirrored(ck.complete(n)))
        u, v = np.nonzero(~np.eye(n, dtype=bool))
        p = d.pairs(u, v, k.JACCARD)
        assert (p["common"] == n - 2).all() and (p["num"] == n - 2).all() and (p["den"] == n).all()
        t = d.topk(np.arange(n), n, k.JACCARD)
        if n > 2:  # everything ties: the id order
            assert all(t["ids"][s, :n - 1].tolist() == [w for w in range(n) if w != s] and t["ids"][s, n - 1] == -1 for s in range(n))
            assert (t["count"] == n - 1).all() and (t["candidates"] == n - 1).all()
            assert (d.topk(np.arange(n), n, k.JACCARD, True)["count"] == 0).all()  # every candidate is a neighbour
        else:
            assert (t["count"] == 0).all()


def test_complete_bipartite_and_star():
    a, b = 3, 5
    d, _ = _agree(*_mirrored(ck.complete_bipartite(a, b)))
    left, right = np.arange(a), a + np.arange(b)
    p = d.pairs([0, 0, a, 0], [1, 2, a + 1, a], k.JACCARD)
    assert p["common"].tolist() == [b, b, a, 0] and p["score"].tolist() == [1.0, 1.0, 1.0, 0.0]
    t = d.topk(np.arange(a + b), 8, k.JACCARD)
    assert t["count"].tolist() == [a - 1] * a + [b - 1] * b
    assert t["ids"][0, :2].tolist() == [1, 2] and t["ids"][a, :4].tolist() == (right[1:]).tolist() and left[0] == 0
    m = 7  # star: the leaves are mutually Jaccard 1, the hub has no candidate
    d, _ = _agree(*_mirrored(k.star(m)))
    t = d.topk(np.arange(m + 1), 64, k.JACCARD)
    assert t["count"].tolist() == [0] + [m - 1] * m and (t["num"][1:, :m - 1] == t["den"][1:, :m - 1]).all()
    assert t["ids"][3, :m - 1].tolist() == [1, 2, 4, 5, 6, 7]


def test_paths_and_cycles():
    for n in (2, 3, 6):
        d, _ = _agree(*_mirrored(k.path(n)))
        t = d.topk(np.arange(n), 4, k.COMMON)
        assert t["ids"][:, :2].tolist() == [[w for w in (s - 2, s + 2) if 0 <= w < n] + [-1] * (2 - sum(0 <= w < n for w in (s - 2, s + 2)))
                                            for s in range(n)]
    for n in (5, 8):  # C_n, n > 4: the two vertices at distance 2 share one neighbour, nobody else does
        d, _ = _agree(*_mirrored(ck.cycle(n)))
        t = d.topk(np.arange(n), 4, k.JACCARD)
        assert (t["count"] == 2).all() and (t["num"][:, :2] == 1).all() and (t["den"][:, :2] == 3).all()
        assert all(sorted(t["ids"][s, :2].tolist()) == sorted([(s - 2) % n, (s + 2) % n]) for s in range(n))
    d, _ = _agree(*_mirrored(ck.cycle(4)))  # C_4: the opposite vertex shares both
    assert d.topk([0], 4, k.JACCARD)["ids"][0].tolist() == [2, -1, -1, -1] and d.pairs([0], [2], k.JACCARD)["score"].tolist() == [1.0]


def test_constructed_ties():
    (n, r, c), first, second = k.rational_tie()
    s = k.Sets(*_mirrored((n, r, c)))
    cand = s.candidates(0, k.JACCARD)
    assert [(w, num, den) for w, _, num, den in cand] == [(first, 2, 6), (second, 1, 3)] and first < second
    (n, r, c), first, second, m = k.near_tie()
    s = k.Sets(*_mirrored((n, r, c)))
    cand = s.candidates(0, k.JACCARD)
    assert [(w, num, den) for w, _, num, den in cand] == [(first, m, 2 * m + 1), (second, m - 1, 2 * m - 1)] and second < first
    assert Fraction(m, 2 * m + 1) > Fraction(m - 1, 2 * m - 1) and np.float32(m / (2 * m + 1)) == np.float32((m - 1) / (2 * m - 1))
    assert 3000 <= m < 12000 and s.wd[0] == 3 * m - 1


@pytest.mark.parametrize("name", ["chesapeake", "test_bc", "bips98_606"])
def test_identities_on_goldens(golden_dir, name):
    n, ro, ci = _golden(golden_dir, name)
    s = k.Sets(n, ro, ci)
    a, b, tri, support, _, _, _ = tk.peel(n, ro, ci)
    common = s.pairs(a, b, k.COMMON)["common"]
    assert np.array_equal(common, support)  # c over the canonical pairs is the triangle support of each edge
    assert int(common.sum()) == 3 * oriented(n, ro, ci)[1] == 3 * tri.shape[0]
    # with every candidate kept: the sum over unordered pairs of C(c, 2) is twice the 4-cycles (each has two diagonals)
    twice = sum(comb(c, 2) for u in range(n) for _, c, _, _ in s.candidates(u, k.COMMON))
    assert twice % 2 == 0 and twice // 2 == 2 * ck.ranked(n, ro, ci)["total"]
