"""The checker of subgraph matching (tests/_sm_checker.py) against closed forms, its two restatements -- plain backtracking and
networkx's GraphMatcher -- against each other on every case, and the inclusion theorem of the 4-vertex graphlets.  No GPU."""
import math
import os

import numpy as np
import pytest

import _sm_checker as k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHESAPEAKE = os.path.join(ROOT, "tests", "golden", "chesapeake.mtx")


def both(graph, name, induced=False, labels=None, plabels=None):
    """the occurrences of a named pattern, by both restatements, which have to agree on everything"""
    q, pairs = k.PATTERNS[name]
    a = k.count(graph, q, pairs, labels, plabels, induced)
    b = k.nx_count(graph, q, pairs, labels, plabels, induced)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (name, induced)
    assert int(a[0].sum()) == q * a[1]
    return a[1]


def test_automorphism_counts():
    for name, want in k.AUT.items():
        assert k.aut(*k.PATTERNS[name]) == want, name
    assert k.aut(3, k.PATTERNS["triangle"][1], [0, 0, 1]) == 2 and k.aut(3, k.PATTERNS["triangle"][1], [0, -1, 1]) == 1
    assert k.aut(3, k.PATTERNS["wedge"][1], [1, -1, 1]) == 2 and k.aut(3, k.PATTERNS["wedge"][1], [1, -1, -1]) == 1


@pytest.mark.parametrize("induced", [False, True])
def test_petersen(induced):
    g = k.petersen()
    assert both(g, "c5", induced) == 12
    assert both(g, "c4", induced) == 0 and both(g, "triangle", induced) == 0
    assert both(g, "wedge", induced) == 30 and both(g, "claw", induced) == 10  # (girth 5: every wedge and claw is induced)
    assert both(g, "c6", induced) == 10


def test_complete_bipartite_and_star():
    assert both(k.complete_bipartite(3, 5), "c4") == 30
    s = k.star(70)
    q, pairs = k.PATTERNS["wedge"]
    assert k.count(s, q, pairs)[1] == math.comb(70, 2) == 2415
    q, pairs = k.PATTERNS["claw"]
    got = k.count(s, q, pairs)
    assert got[1] == math.comb(70, 3) == 54740 and got[0][0] == 54740 and got[0][1] == math.comb(69, 2)
    small = k.star(9)
    assert both(small, "wedge") == 36 and both(small, "claw", True) == 84


@pytest.mark.parametrize("n", [6, 7])
def test_complete_graph(n):
    g = k.complete(n)
    for name in ("wedge", "triangle", "p4", "claw", "c4", "paw", "diamond", "k4", "c5", "house", "bull", "k5"):
        q, pairs = k.PATTERNS[name]
        falling = math.factorial(n) // math.factorial(n - q)
        use = both if n == 6 or q < 5 else (lambda g_, name_, induced=False: k.count(g_, *k.PATTERNS[name_], induced=induced)[1])
        assert use(g, name) == falling // k.aut(q, pairs), name
        complete = len(pairs) == q * (q - 1) // 2
        assert use(g, name, True) == (falling // k.aut(q, pairs) if complete else 0), name


def test_labels_and_wildcards_agree_with_networkx():
    g = k.gnp(16, 0.35, 5)
    for seed, name in enumerate(("wedge", "triangle", "p4", "paw", "diamond", "c5", "house")):
        labels, plabels = k.seeded_labels(g[0], k.PATTERNS[name][0], 100 + seed)
        for induced in (False, True):
            both(g, name, induced, labels, plabels)


def test_other_csr_forms_and_relabelled_patterns_count_the_same():
    g = k.gnp(14, 0.4, 9)
    rng = np.random.default_rng(3)
    for name in ("paw", "house"):
        q, pairs = k.PATTERNS[name]
        labels, plabels = k.seeded_labels(g[0], q, 7)
        want = k.count(g, q, pairs, labels, plabels, True)
        got = k.count(k.shuffled(g, 11), q, pairs, labels, plabels, True)
        assert np.array_equal(want[0], got[0]) and want[1:] == got[1:]
        perm = [int(x) for x in rng.permutation(q)]
        pairs2, plabels2 = k.relabelled(q, pairs, plabels, perm)
        got = k.count(g, q, pairs2, labels, plabels2, True)
        assert np.array_equal(want[0], got[0]) and want[1:] == got[1:]


@pytest.mark.parametrize("graph", ["chesapeake", "gnp"])
def test_inclusion_theorem_of_the_four_vertex_graphlets(graph):
    """not induced(H) = sum over the connected 4-vertex H' of (spanning copies of H in H') x induced(H'), per vertex too"""
    g = k.read_mtx(CHESAPEAKE) if graph == "chesapeake" else k.gnp(40, 0.2, 1)
    names = k.GRAPHLETS[4]
    induced = {name: k.count(g, *k.PATTERNS[name], induced=True) for name in names}
    multiplier = {(h, other): k.spanning_copies(4, k.PATTERNS[h][1], k.PATTERNS[other][1]) for h in names for other in names}
    assert multiplier[("p4", "k4")] == 12 and multiplier[("c4", "k4")] == 3 and multiplier[("claw", "k4")] == 4 and multiplier[("c4", "diamond")] == 1
    assert all(multiplier[(h, h)] == 1 for h in names) and multiplier[("k4", "diamond")] == 0
    for h in names:
        plain = k.count(g, *k.PATTERNS[h])
        assert plain[1] == sum(multiplier[(h, other)] * induced[other][1] for other in names), h
        assert np.array_equal(plain[0], sum(multiplier[(h, other)] * induced[other][0] for other in names)), h
    if graph == "chesapeake":
        assert g[0] == 39 and induced["k4"][1] > 0
