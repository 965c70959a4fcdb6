"""Subgraph matching on the GPU (gunrockinst_amd/sm.py) against the checker (tests/_sm_checker.py), bit for bit: closed forms, every
named pattern on chesapeake and on a seeded scale-7 R-MAT, induced and not, labelled and not; row lengths that cross the chunk sizes
of both group widths; options, CSR forms and pattern numberings that never change a result; the tree's own tc, clique and c4
families on a seeded scale-10 R-MAT; refusals; the graphlet census and the identities between the outputs."""
import functools
import math
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
import _sm_checker as k

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("wedge", "triangle", "p4", "claw", "c4", "paw", "diamond", "k4", "c5", "house", "bull", "k5")
SMALL = ("wedge", "triangle", "p4", "claw", "c4", "paw", "diamond", "k4")


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "chesapeake":
        return k.read_mtx(os.path.join(ROOT, "tests", "golden", "chesapeake.mtx"))
    if name == "rmat7":
        return k.rmat(7, 1024, 7)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def labels_of(graph_name, pattern):
    """seeded labels in {0, 1, 2} for the graph and in {-1, 0, 1, 2} for the pattern"""
    return k.seeded_labels(graph(graph_name)[0], k.PATTERNS[pattern][0], sum(map(ord, graph_name + pattern)))


@functools.lru_cache(maxsize=None)
def reference(graph_name, pattern, induced, labelled):
    labels, plabels = labels_of(graph_name, pattern) if labelled else (None, None)
    return k.count(graph(graph_name), *k.PATTERNS[pattern], labels, plabels, induced)


def enact(p, q, pairs, plabels=None, induced=False, per_vertex=True):
    """(count, occurrences, embeddings, aut) of one pattern on an initialised handle, the identities between them checked"""
    p.set_pattern(q, pairs, plabels, induced)
    p.enact()
    count, occurrences, embeddings = p.extract()
    info = p.pattern_info()
    assert count.dtype == np.int64 and count.shape == (p.nodes,)
    assert embeddings == info["aut"] * occurrences
    assert int(count.sum()) == (q * occurrences if per_vertex else 0)
    st = p.stats()
    assert st["occurrences"] == occurrences and st["embeddings"] == embeddings and st["items"] == st["group8_items"] + st["wave_items"]
    return count, occurrences, embeddings, info["aut"]


def solve(g, q, pairs, labels=None, plabels=None, induced=False, options=()):
    p = ga.SmProblem().init(*g, labels)
    try:
        for name, value in options:
            assert p.set_option(name, value) == 0, name
        return enact(p, q, pairs, plabels, induced, dict(options).get("per_vertex", 1) != 0)
    finally:
        p.close()


def same(got, want):
    return np.array_equal(got[0], want[0]) and got[1] == want[1] and got[3] == want[2]


def test_closed_forms():
    pet = k.petersen()
    for induced in (False, True):
        assert solve(pet, *k.PATTERNS["c5"], induced=induced)[1] == 12
        assert solve(pet, *k.PATTERNS["c4"], induced=induced)[1] == 0 and solve(pet, *k.PATTERNS["triangle"], induced=induced)[1] == 0
    got = solve(pet, *k.PATTERNS["wedge"])
    assert got[1] == 30 and got[0].tolist() == [9] * 10 and got[3] == 2
    assert solve(pet, *k.PATTERNS["claw"])[1] == 10 and solve(pet, *k.PATTERNS["c6"])[1] == 10
    got = solve(k.complete_bipartite(3, 5), *k.PATTERNS["c4"])
    assert got[1] == 30 and got[0].tolist() == [20] * 3 + [12] * 5
    s = k.star(70)
    assert solve(s, *k.PATTERNS["wedge"])[1] == math.comb(70, 2) == 2415
    got = solve(s, *k.PATTERNS["claw"])
    assert got[1] == math.comb(70, 3) == 54740 and got[0][0] == 54740 and got[0][1:].tolist() == [math.comb(69, 2)] * 70
    for name, want in k.AUT.items():
        p = ga.SmProblem()
        assert p.set_pattern(None, name).pattern_info()["aut"] == want, name
        p.close()


def test_complete_graph():
    n = 7
    p = ga.SmProblem().init(*k.complete(n))
    for name in ALL:
        q, pairs = k.PATTERNS[name]
        falling = math.factorial(n) // math.factorial(n - q)
        got = enact(p, q, pairs)
        assert got[1] == falling // got[3] and got[0].tolist() == [got[1] * q // n] * n, name
        assert enact(p, q, pairs, induced=True)[1] == (got[1] if len(pairs) == q * (q - 1) // 2 else 0), name
    p.close()


@pytest.mark.parametrize("pattern", ALL)
def test_chesapeake(pattern):
    g = graph("chesapeake")
    assert g[0] == 39
    for labelled in (False, True):
        labels, plabels = labels_of("chesapeake", pattern) if labelled else (None, None)
        p = ga.SmProblem().init(*g, labels)
        for induced in (False, True):
            assert same(enact(p, *k.PATTERNS[pattern], plabels, induced), reference("chesapeake", pattern, induced, labelled)), (labelled, induced)
        p.close()


@pytest.mark.parametrize("pattern", SMALL)
def test_rmat7(pattern):
    g = graph("rmat7")
    for labelled in (False, True):
        labels, plabels = labels_of("rmat7", pattern) if labelled else (None, None)
        p = ga.SmProblem().init(*g, labels)
        for induced in (False, True):
            assert same(enact(p, *k.PATTERNS[pattern], plabels, induced), reference("rmat7", pattern, induced, labelled)), (labelled, induced)
        p.close()


@pytest.mark.parametrize("degree", [7, 8, 9, 17, 63, 64, 65, 129])
def test_rows_that_cross_the_chunk_sizes(degree):
    """stars and double stars whose hub rows end before, on and behind a chunk of 8 and of 64, under both group widths"""
    for g in (k.star(degree), k.double_star(degree - 1)):  # (the double star's hubs have each other and degree - 1 leaves)
        want = {name: k.count(g, *k.PATTERNS[name]) for name in ("wedge", "p4", "claw", "paw", "c4")}
        for strategy in (ga.SM_AUTO, ga.SM_GROUP8, ga.SM_WAVE):
            p = ga.SmProblem().init(*g)
            assert p.set_option("strategy", strategy) == 0
            for name, ref in want.items():
                assert same(enact(p, *k.PATTERNS[name]), ref), (name, strategy)
            p.close()


def test_complete_graphs_beyond_a_wave():
    g = k.complete(66)
    for strategy in (ga.SM_GROUP8, ga.SM_WAVE):
        got = solve(g, *k.PATTERNS["triangle"], options=(("strategy", strategy),))
        assert got[1] == math.comb(66, 3) == 45760 and got[0].tolist() == [math.comb(65, 2)] * 66
        assert same(got, k.count(g, *k.PATTERNS["triangle"]))
        got = solve(g, *k.PATTERNS["k4"], options=(("strategy", strategy),))
        assert got[1] == math.comb(66, 4) and got[0].tolist() == [math.comb(65, 3)] * 66 and got[3] == 24
    g = k.complete_bipartite(9, 65)
    for strategy in (ga.SM_AUTO, ga.SM_GROUP8, ga.SM_WAVE):
        got = solve(g, *k.PATTERNS["c4"], options=(("strategy", strategy),))
        assert got[1] == math.comb(9, 2) * math.comb(65, 2) and same(got, k.count(g, *k.PATTERNS["c4"]))


OPTIONS = [(("symmetry", 0),), (("strategy", ga.SM_GROUP8),), (("strategy", ga.SM_WAVE),), (("group_max_row", 1),), (("group_max_row", 1024),),
           (("order", 1),), (("order", 2),), (("symmetry", 0), ("order", 1), ("strategy", ga.SM_WAVE)),
           (("symmetry", 0), ("order", 2), ("group_max_row", 4))]


@pytest.mark.parametrize("graph_name", ["chesapeake", "rmat7"])
@pytest.mark.parametrize("pattern", ["paw", "diamond", "c5", "house"])
def test_options_csr_forms_and_numberings_never_change_a_result(graph_name, pattern):
    g = graph(graph_name)
    q, pairs = k.PATTERNS[pattern]
    labels, plabels = labels_of(graph_name, pattern)
    for induced, labelled in ((False, False), (True, True)):
        lab, plab = (labels, plabels) if labelled else (None, None)
        base = solve(g, q, pairs, lab, plab, induced)
        assert same(base, reference(graph_name, pattern, induced, labelled))
        for options in OPTIONS:
            got = solve(g, q, pairs, lab, plab, induced, options)
            assert got[0].tobytes() == base[0].tobytes() and got[1:] == base[1:], options
        got = solve(g, q, pairs, lab, plab, induced, (("per_vertex", 0),))
        assert got[1:] == base[1:] and not got[0].any()
        got = solve(k.shuffled(g, 5), q, pairs, lab, plab, induced)
        assert got[0].tobytes() == base[0].tobytes() and got[1:] == base[1:]
        perm = [int(x) for x in np.random.default_rng(q).permutation(q)]
        pairs2, plab2 = k.relabelled(q, pairs, None if plab is None else plab.tolist(), perm)
        got = solve(g, q, pairs2, lab, plab2, induced)
        assert got[0].tobytes() == base[0].tobytes() and got[1:] == base[1:], perm


def test_two_patterns_on_one_handle_equal_two_fresh_handles():
    g = graph("chesapeake")
    p = ga.SmProblem().init(*g)
    first = enact(p, *k.PATTERNS["house"], induced=True)
    second = enact(p, *k.PATTERNS["paw"])
    again = enact(p, *k.PATTERNS["house"], induced=True)
    p.close()
    assert same(first, reference("chesapeake", "house", True, False)) and same(second, reference("chesapeake", "paw", False, False))
    assert first[0].tobytes() == again[0].tobytes() and first[1:] == again[1:]
    fresh = solve(g, *k.PATTERNS["paw"])
    assert fresh[0].tobytes() == second[0].tobytes() and fresh[1:] == second[1:]


def test_against_the_triangle_clique_and_four_cycle_families():
    from oracle import gr_oracle as o
    r = o.rmat_seeded(10, 8 << 10)
    g = (r.nodes, np.asarray(r.row_offsets), np.asarray(r.col_indices))
    p = ga.SmProblem().init(*g)  # (the default work_limit admits all four)
    tri, total = ga.gunrock_tc(*g)
    got = enact(p, *k.PATTERNS["triangle"])
    assert got[0].tobytes() == tri.astype(np.int64).tobytes() and got[1] == total > 0
    for name, size in (("k4", 4), ("k5", 5)):
        cliques, total = ga.gunrock_cliques(*g, size)
        got = enact(p, *k.PATTERNS[name])
        assert cliques.dtype == np.int64 and got[0].tobytes() == cliques.tobytes() and got[1] == total > 0, name
    cycles, total = ga.gunrock_four_cycles(*g)
    got = enact(p, *k.PATTERNS["c4"])
    assert got[0].tobytes() == cycles.tobytes() and got[1] == total > 0
    assert p.stats()["bound"] * 3 <= 2.0 ** 38
    p.close()


def test_refusals():
    g = graph("chesapeake")
    p = ga.SmProblem().init(*g)
    with pytest.raises(RuntimeError):
        p.enact()  # no pattern yet
    want = enact(p, *k.PATTERNS["paw"])
    bad = [(1, []), (7, [(i, i + 1) for i in range(6)]), (3, [(0, 1), (1, 3)]), (3, [(0, 1), (-1, 2)]), (3, [(0, 1), (1, 1), (1, 2)]),
           (4, [(0, 1), (2, 3)]), (2, [])]
    for q, pairs in bad:
        with pytest.raises(ValueError):
            p.set_pattern(q, pairs)
    with pytest.raises(ValueError):
        p.set_pattern(3, k.PATTERNS["wedge"][1], [0, -2, 0])
    with pytest.raises(ValueError):
        p.set_pattern(3, k.PATTERNS["wedge"][1], [0, 1])
    p.enact()  # nothing was installed: the paw is still in force
    got = p.extract()
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    for name, value in (("symmetry", 2), ("per_vertex", -1), ("strategy", 3), ("group_max_row", 0), ("work_limit", 0.5), ("order", 3)):
        with pytest.raises(RuntimeError):
            p.set_option(name, value)
    assert p.set_option("no such option", 1) == 1

    assert p.set_option("work_limit", 1) == 0
    with pytest.raises(ga.SmTooLarge):
        p.enact()
    with pytest.raises(RuntimeError):
        p.extract()  # a refused handle holds no result
    assert p.stats()["bound"] > 1
    assert p.set_option("work_limit", 2.0 ** 70) == 0  # capped at 2^62
    p.enact()
    got = p.extract()
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    p.close()

    n, ro, ci = g
    broken = ci.copy()
    broken[3] = n
    p = ga.SmProblem()
    with pytest.raises(RuntimeError, match=r"code -2\b"):
        p.init(n, ro, broken)
    p.close()
    p = ga.SmProblem()
    with pytest.raises(RuntimeError, match=r"code -2\b"):
        p.init(n, ro[::-1].copy(), ci)
    p.close()
    assert same(solve(g, *k.PATTERNS["paw"]), reference("chesapeake", "paw", False, False))


def test_empty_graphs_and_patterns_larger_than_the_graph():
    for g in ((0, np.zeros(1, np.int32), np.zeros(0, np.int32)), (5, np.zeros(6, np.int32), np.zeros(0, np.int32)),
              (3, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32))):  # no vertex; no entry; self-loops only
        for name in ("edge", "wedge", "k4"):
            got = solve(g, *k.PATTERNS.get(name, (2, [(0, 1)])))
            assert got[1] == 0 and got[2] == 0 and not got[0].any() and got[0].shape == (g[0],)
    tri = k.complete(3)
    assert solve(tri, 2, [(0, 1)])[1] == 3 and solve(tri, *k.PATTERNS["triangle"])[1] == 1
    for name in ("k4", "p4", "c5"):
        assert solve(tri, *k.PATTERNS[name])[1] == 0  # q > n


def test_edges_and_labelled_triangles():
    g = graph("chesapeake")
    got = solve(g, 2, [(0, 1)])
    want = k.count(g, 2, [(0, 1)])
    assert same(got, want) and got[1] == 170 and got[3] == 2
    labels = (np.arange(g[0]) % 3).astype(np.int32)
    for plabels in ([0, 1, 2], [0, 0, 1], [-1, 1, 1], [2, -1, -1]):
        assert same(solve(g, *k.PATTERNS["triangle"], labels, plabels), k.count(g, *k.PATTERNS["triangle"], labels, plabels)), plabels
    got = solve(g, 2, [(0, 1)], labels, [0, 1])
    assert same(got, k.count(g, 2, [(0, 1)], labels, [0, 1])) and got[3] == 1


@pytest.mark.parametrize("size", [3, 4])
def test_graphlets(size):
    g = graph("chesapeake")
    got = ga.gunrock_graphlets(*g, size)
    assert tuple(got) == k.GRAPHLETS[size]
    for name, (count, occurrences) in got.items():
        want = reference("chesapeake", name, True, False)
        assert np.array_equal(count, want[0]) and occurrences == want[1] and int(count.sum()) == size * occurrences, name
    count, occurrences, aut = ga.gunrock_subgraph_matching(*g, k.PATTERNS["diamond"][1], 4, induced=True)
    want = reference("chesapeake", "diamond", True, False)
    assert np.array_equal(count, want[0]) and (occurrences, aut) == want[1:]


def test_device_csr_and_device_labels():
    import torch
    g = graph("chesapeake")
    labels, plabels = labels_of("chesapeake", "paw")
    dev = [torch.as_tensor(np.ascontiguousarray(x), device="cuda") for x in (g[1], g[2], labels)]
    p = ga.SmProblem().init_device(g[0], int(g[2].shape[0]), *(t.data_ptr() for t in dev))
    assert same(enact(p, *k.PATTERNS["paw"], plabels, True), reference("chesapeake", "paw", True, True))
    d_count, d_deg = p.device_results()
    assert d_count and d_deg
    p.close()
