"""Label propagation on the GPU (grx_lp_*): labels, community, state, rounds, visits, entries_read and the summary arrays must
equal tests/_lp_checker.py's with np.array_equal in both modes under all four strategies -- goldens read directed and undirected with
three kinds of weights, the hand cases with their pinned values, rows at the regime boundaries, tables too small for a row's labels,
the tie rule in one round, raw CSRs of every awkward shape, the refusals, and R-MAT at scale 16 built on the device."""
import functools
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _lp_checker as k

pytestmark = pytest.mark.gpu

STRATEGIES = (ga.LP_AUTO, ga.LP_LANE, ga.LP_WAVE, ga.LP_BLOCK)
NOT_READY = "code 600"  # hipErrorNotReady
SMALL = 3000            # up to this many vertices the plain-Python form runs next to the numpy form


def _reference(n, a, b, pw, mode, classes, start, max_rounds):
    solve = k.solve if n <= SMALL else k.run_numpy
    return solve(n, a, b, pw, mode, classes, start, max_rounds if max_rounds else 10 ** 9)


def _compare(p, n, a, b, pw, ref, what):
    labels, community, communities = p.extract()
    st = p.stats()
    print(what, {name: st[name] for name in ("rounds", "state", "visits", "entries_read", "regime_rows", "fallback_rows", "readbacks")})
    assert labels.dtype == np.int32 and np.array_equal(labels, ref["labels"]), "labels differ from the checker: " + what
    want_community, want_count = k.community_of(ref["labels"])
    assert community.dtype == np.int32 and np.array_equal(community, want_community) and communities == want_count, what
    for name in k.FIELDS:
        assert st[name] == ref[name], "%s: %s is %s, the checker's %s" % (what, name, st[name], ref[name])
    assert st["pairs"] == a.shape[0] and st["readbacks"] <= st["rounds"] + 2, (what, st)
    got, want = p.summary(), k.summary_of(n, a, b, pw, ref["labels"])
    for name in ("size", "internal", "volume"):
        assert got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), "%s: summary %s differs" % (what, name)
    assert got["W"] == want["W"], what
    assert ga.modularity_from_sums(got["internal"], got["volume"], got["W"]) == k.modularity(want)
    visited, changed = p.round_trace()
    assert int(visited.sum()) == st["visits"] and int((changed > 0).sum()) == st["rounds"], what
    return st


def _check(n, ro, ci, w=None, mode=ga.LP_SYNC, classes=None, start=None, max_rounds=0, strategies=STRATEGIES, handle=None, **options):
    """the graph under every strategy on one handle, everything against the checker; returns the stats of the last run"""
    a, b, pw = k.pairs_of(n, ro, ci, w)
    ref = _reference(n, a, b, pw, mode, classes, start, max_rounds)
    p = handle if handle is not None else ga.LpProblem().init(n, ro, ci, w)
    assert p.set_option("mode", mode) == 0 and p.set_option("max_rounds", max_rounds) == 0
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    if classes is not None:
        assert p.set_classes(classes) == 0
    st = None
    for strategy in strategies:
        assert p.set_option("strategy", strategy) == 0
        p.reset(start)
        p.enact()
        st = _compare(p, n, a, b, pw, ref, "mode %d strategy %d %s" % (mode, strategy, options))
        if strategy != ga.LP_AUTO:
            assert sum(st["regime_rows"]) == st["regime_rows"][strategy - 1]
    if handle is None:
        p.close()
    return st


def _both_modes(n, ro, ci, w=None, coloured=True, **kw):
    """SYNC, CLASSES with the checker's id-order greedy colouring and, when coloured, CLASSES with gunrock_color's classes: one handle"""
    a, b, _ = k.pairs_of(n, ro, ci, w)
    p = ga.LpProblem().init(n, ro, ci, w)
    _check(n, ro, ci, w, ga.LP_SYNC, handle=p, **kw)
    greedy = k.greedy_classes(n, a, b)
    _check(n, ro, ci, w, ga.LP_CLASSES, classes=greedy, handle=p, **kw)
    if coloured:
        colours = ga.gunrock_color(n, ro, ci, seed=0)[0].astype(np.int32) - 1
        assert k.is_proper(a, b, colours)
        _check(n, ro, ci, w, ga.LP_CLASSES, classes=colours, handle=p, **kw)
    p.close()


def _degree_weights(n, ro, ci):
    deg = np.diff(np.asarray(ro, np.int64))
    rows = np.repeat(np.arange(n), deg)
    return (deg[rows] + deg[np.asarray(ci, np.int64)]).astype(np.int32)


GOLDENS = ("fixture7", "test_bc", "test_cc", "test_pr", "chesapeake", "bips98_606")  # test_matching_gpu.py's


@pytest.mark.parametrize("undirected", (True, False))
@pytest.mark.parametrize("name", GOLDENS)
def test_fixtures_and_goldens(name, undirected, golden, golden_dir):
    if name == "fixture7":
        f = golden["fixture7"]
        n, ro, ci = 7, np.array(f["row_offsets"], np.int32), np.array(f["col_indices"], np.int32)
        if undirected:
            rows = np.repeat(np.arange(7), np.diff(ro))
            ro, ci, _ = k.csr_from_pairs(7, rows, ci)
    else:
        g = o.build_market(os.path.join(golden_dir, name + ".mtx"), undirected=undirected)
        n, ro, ci = g.nodes, g.row_offsets, g.col_indices
    for w in (None, k.mod7_weights(n, ro, ci), _degree_weights(n, ro, ci)):
        _both_modes(n, ro, ci, w)


# ---------------- the hand cases and their pinned values ----------------

def _one_shot(n, ro, ci, w=None, mode=ga.LP_SYNC, labels=None, max_rounds=0):
    labels, community, communities, state, rounds = ga.gunrock_label_propagation(n, ro, ci, w, mode=mode, labels=labels, max_rounds=max_rounds)
    assert np.array_equal(community, k.community_of(labels)[0])
    return communities, state, rounds


def test_k33_and_star():
    ro, ci = k.complete_bipartite(3, 3)
    st = _check(6, ro, ci)
    assert (st["state"], st["rounds"]) == (ga.LP_PERIOD2, 3) and _one_shot(6, ro, ci) == (2, ga.LP_PERIOD2, 3)
    st = _check(6, ro, ci, mode=ga.LP_CLASSES, classes=[0, 0, 0, 1, 1, 1])
    assert (st["state"], st["rounds"]) == (ga.LP_CONVERGED, 1)
    assert _one_shot(6, ro, ci, mode=ga.LP_CLASSES)[:2] == (1, ga.LP_CONVERGED)
    ro, ci = k.star(64)
    st = _check(65, ro, ci)
    assert (st["state"], st["rounds"]) == (ga.LP_PERIOD2, 3) and _one_shot(65, ro, ci)[1:] == (ga.LP_PERIOD2, 3)


@pytest.mark.parametrize("c,s", [(5, 4), (6, 8), (64, 5)])
def test_clique_rings(c, s):
    n = c * s
    ro, ci = k.clique_ring(c, s)
    a, b, _ = k.pairs_of(n, ro, ci)
    a, b, pw = k.pairs_of(n, ro, ci)
    cliques = np.repeat(np.arange(c), s)
    st = _check(n, ro, ci)
    assert (st["state"], st["rounds"]) == (ga.LP_CONVERGED, 2)
    greedy = k.greedy_classes(n, a, b)
    _check(n, ro, ci, mode=ga.LP_CLASSES, classes=greedy)
    assert np.array_equal(k.community_of(k.solve(n, a, b, pw, k.CLASSES, greedy)["labels"])[0], cliques)
    labels, community, communities, state, rounds = ga.gunrock_label_propagation(n, ro, ci, mode=ga.LP_SYNC)
    assert (state, rounds, communities) == (ga.LP_CONVERGED, 2, c) and np.array_equal(community, cliques)
    # the one-shot's classes are gunrock_color's, and which fixed point the sweep reaches depends on the colouring: under the seeded
    # first-fit colours a clique of the (5, 4) and of the (64, 5) ring is taken over by its neighbour (both checker forms say so)
    colours = ga.gunrock_color(n, ro, ci, seed=0)[0].astype(np.int32) - 1
    ref = k.solve(n, a, b, pw, k.CLASSES, colours)
    labels, community, communities, state, rounds = ga.gunrock_label_propagation(n, ro, ci, mode=ga.LP_CLASSES)
    assert np.array_equal(labels, ref["labels"]) and (state, rounds) == (ga.LP_CONVERGED, ref["rounds"])
    assert communities in (c - 1, c) and (community[cliques == 0] == 0).all()


@functools.lru_cache(maxsize=None)
def _path2001(rising, mode, max_rounds=0):
    n = 2001
    ro, ci, w = k.path(n, np.arange(1, n) if rising else None)
    a, b, pw = k.pairs_of(n, ro, ci, w)
    ref = k.run_numpy(n, a, b, pw, mode, np.arange(n) % 2, None, max_rounds if max_rounds else 10 ** 9, keep=max_rounds > 0)
    return n, ro, ci, w, a, b, pw, ref


def _run_path(rising, mode, max_rounds=0):
    n, ro, ci, w, a, b, pw, ref = _path2001(rising, mode, max_rounds)
    p = ga.LpProblem().init(n, ro, ci, w)
    p.set_option("mode", mode)
    p.set_option("max_rounds", max_rounds if max_rounds else 4000)
    assert p.set_classes(np.arange(n) % 2) == 0
    p.reset()
    p.enact()
    st = _compare(p, n, a, b, pw, ref, "path rising=%s mode %d" % (rising, mode))
    communities = p.extract()[2]
    p.close()
    return st, communities, ref


def test_unit_path_sync():
    st, _, _ = _run_path(False, ga.LP_SYNC)
    assert (st["state"], st["rounds"], st["entries_read"]) == (ga.LP_PERIOD2, 2001, 8004000)


def test_unit_path_classes():
    st, communities, _ = _run_path(False, ga.LP_CLASSES)
    assert (st["state"], st["rounds"], communities, st["entries_read"]) == (ga.LP_CONVERGED, 1, 1000, 4000)


def test_rising_path_classes_and_its_readbacks():
    st, communities, _ = _run_path(True, ga.LP_CLASSES)
    assert (st["state"], st["rounds"], communities, st["entries_read"]) == (ga.LP_CONVERGED, 1000, 1, 2002999)
    assert st["readbacks"] <= st["rounds"] + 2 and st["kernel_launches"] == 2 * 1001, "one launch per sub-step, one read-back per round"


def test_max_rounds_caps():
    st, _, ref = _run_path(False, ga.LP_SYNC, max_rounds=3)
    assert (st["state"], st["rounds"]) == (ga.LP_CAPPED, 3) and np.array_equal(ref["labels"], ref["history"][2])


def test_pinned_goldens(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    st = _check(g.nodes, g.row_offsets, g.col_indices, strategies=(ga.LP_AUTO,))
    assert (st["pairs"], st["state"], st["rounds"], st["entries_read"]) == (170, ga.LP_CONVERGED, 4, 1363)
    assert _one_shot(g.nodes, g.row_offsets, g.col_indices) == (1, ga.LP_CONVERGED, 4)
    g = o.build_market(os.path.join(golden_dir, "bips98_606.mtx"), undirected=True)
    st = _check(g.nodes, g.row_offsets, g.col_indices, strategies=(ga.LP_AUTO,))
    assert (st["pairs"], st["state"], st["rounds"], st["entries_read"]) == (15190, ga.LP_PERIOD2, 20, 257350)
    assert _one_shot(g.nodes, g.row_offsets, g.col_indices) == (1679, ga.LP_PERIOD2, 20)
    g = o.rmat_seeded(12, 8 << 12)
    st = _check(g.nodes, g.row_offsets, g.col_indices, strategies=(ga.LP_AUTO,))
    assert (st["pairs"], st["state"], st["rounds"], st["entries_read"]) == (27791, ga.LP_CONVERGED, 4, 168981)
    assert _one_shot(g.nodes, g.row_offsets, g.col_indices) == (982, ga.LP_CONVERGED, 4)


# ---------------- regimes ----------------

def _hubs(degrees, rng, spread):
    """one hub per entry of `degrees`, each with leaves of its own; every leaf has one further neighbour among `spread` shared
    vertices, so that labels travel and hubs see many labels"""
    rows, cols, at = [], [], len(degrees) + spread
    for h, d in enumerate(degrees):
        leaves = np.arange(at, at + d)
        at += d
        rows += [np.full(d, h), leaves]
        cols += [leaves, len(degrees) + rng.integers(0, spread, d)]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return (at,) + k.csr_from_pairs(at, rows, cols, rng.integers(1, 4, rows.shape[0]))


@pytest.mark.parametrize("lane_max_row,wave_max_row", [(16, 512), (4, 40), (1, 70)])
def test_rows_at_the_regime_boundaries(lane_max_row, wave_max_row):
    rng = np.random.default_rng(lane_max_row)
    bounds = sorted({max(lane_max_row - 1, 1), max(lane_max_row, 1), lane_max_row + 1, wave_max_row - 1, wave_max_row, wave_max_row + 1})
    n, ro, ci, w = _hubs(bounds, rng, 7)
    deg = np.bincount(k.pairs_of(n, ro, ci)[0], minlength=n) + np.bincount(k.pairs_of(n, ro, ci)[1], minlength=n)
    assert deg[:len(bounds)].tolist() == bounds
    for mode, classes in ((ga.LP_SYNC, None), (ga.LP_CLASSES, k.greedy_classes(n, *k.pairs_of(n, ro, ci)[:2]))):
        st = _check(n, ro, ci, w, mode, classes, strategies=(ga.LP_AUTO,), lane_max_row=lane_max_row, wave_max_row=wave_max_row)
        assert all(x > 0 for x in st["regime_rows"]), "an AUTO run uses all three regimes: %s" % st["regime_rows"]


@pytest.mark.parametrize("n", (63, 64, 65, 1023, 1024, 1025))
def test_vertex_counts_around_the_wave_and_the_workgroup(n):
    rng = np.random.default_rng(n)
    rows, cols = rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)
    ro, ci, w = k.csr_from_pairs(n, rows, cols, rng.integers(1, 5, 3 * n))
    _both_modes(n, ro, ci, w, coloured=False, strategies=(ga.LP_AUTO, ga.LP_WAVE))


def _hub300(tied):
    """vertex 0 with neighbours 1 .. 300; the neighbours carry 300 distinct labels.  tied: unit weights, every label scores 1;
    else the weights differ and label 300 - 7 = 293's neighbour is the heaviest"""
    w = None if tied else ((np.arange(300) * 37) % 300 + 1)
    ro, ci, w = k.csr_from_pairs(301, np.zeros(300, np.int64), np.arange(1, 301), w)
    return ro, ci, w


@pytest.mark.parametrize("strategy", (ga.LP_AUTO, ga.LP_BLOCK))
def test_fallback_when_a_row_has_more_labels_than_slots(strategy):
    slots = 64  # (under LP_BLOCK a workgroup's table has 256 slots: still fewer than 300 labels)
    for tied in (False, True):
        ro, ci, w = _hub300(tied)
        a, b, pw = k.pairs_of(301, ro, ci, w)
        for hub_label in (0, 150, 300):  # absent from the neighbours; among them (keep-current wins a tie); the largest of them
            start = np.arange(301, dtype=np.int32)
            start[0] = hub_label
            ref = k.solve(301, a, b, pw, k.SYNC, None, start, 1)
            if tied:
                assert ref["labels"][0] == (hub_label if hub_label else 1), "keep-current among the tied, else the smallest"
            results = []
            for table_slots in (slots, 1024):
                p = ga.LpProblem().init(301, ro, ci, w)
                for name, value in (("mode", ga.LP_SYNC), ("strategy", strategy), ("table_slots", table_slots), ("max_rounds", 1)):
                    assert p.set_option(name, value) == 0
                p.reset(start)
                p.enact()
                st = _compare(p, 301, a, b, pw, ref, "hub300 tied=%s label %d slots %d" % (tied, hub_label, table_slots))
                assert (st["fallback_rows"] > 0) == (table_slots == slots), st
                results.append(p.extract()[0])
                p.close()
            assert np.array_equal(results[0], results[1]), "table_slots changes no result"


def test_tie_rule_in_one_round():
    ro, ci = k.star(3)
    for start, want in (([3, 3, 1, 2], 3), ([0, 3, 1, 2], 1)):  # the current label tied with smaller ones keeps; absent, the smallest wins
        st = _check(4, ro, ci, start=np.array(start, np.int32), max_rounds=1)
        labels = ga.gunrock_label_propagation(4, ro, ci, mode=ga.LP_SYNC, labels=np.array(start, np.int32), max_rounds=1)[0]
        assert labels[0] == want and st["state"] == ga.LP_CAPPED
    ro, ci, w = k.csr_from_pairs(4, [0, 0, 0], [1, 2, 3], [1, 1, 3])  # two neighbours of weight 1 against one of weight 3
    _check(4, ro, ci, w, start=np.array([0, 1, 1, 2], np.int32), max_rounds=1)
    assert ga.gunrock_label_propagation(4, ro, ci, w, mode=ga.LP_SYNC, labels=np.array([0, 1, 1, 2], np.int32), max_rounds=1)[0][0] == 2


# ---------------- awkward input ----------------

def test_unsorted_rows_duplicates_one_way_entries_and_self_loops():
    rng = np.random.default_rng(3)
    rows, cols = rng.integers(0, 300, 2000), rng.integers(0, 300, 2000)
    ro, ci, w = k.csr_from_pairs(300, rows, cols, rng.integers(1, 9, 2000), shuffle=rng)
    _both_modes(300, ro, ci, w, coloured=False, strategies=(ga.LP_AUTO,))
    _both_modes(300, ro, ci, None, strategies=(ga.LP_AUTO,))
    # pair {0, 1}: entries 3, 9 and 5 -> 9; pair {1, 2}: 4 and 6 -> 6; pair {2, 3}: 2 one way only; a heavy self-loop at 3: ignored
    rows, cols, w = [0, 0, 1, 1, 2, 2, 3], [1, 1, 0, 2, 1, 3, 3], [3, 9, 5, 4, 6, 2, k.INT_MAX]
    ro, ci, w = k.csr_from_pairs(4, rows, cols, w, mirror=False)
    assert k.pairs_of(4, ro, ci, w)[2].tolist() == [9, 6, 2]
    _both_modes(4, ro, ci, w)
    p = ga.LpProblem().init(4, ro, ci, w)  # vertex 1 between 0 (9, label 3) and 2 (6, label 2); vertex 2 between 1 (6) and 3 (2)
    p.set_option("mode", ga.LP_SYNC)
    p.set_option("max_rounds", 1)
    p.reset(np.array([3, 1, 2, 2], np.int32))
    p.enact()
    assert p.extract()[0].tolist() == [1, 3, 1, 2] and p.summary()["W"] == 17, "the largest entry of a pair decides"
    p.close()
    g = o.rmat_seeded(8, 8 << 8, undirected=False)
    rows = np.repeat(np.arange(g.nodes), np.diff(g.row_offsets))
    keep = rows < g.col_indices  # the upper triangle alone
    ro, ci, _ = k.csr_from_pairs(g.nodes, rows[keep], g.col_indices[keep], mirror=False)
    _both_modes(g.nodes, ro, ci, None, strategies=(ga.LP_AUTO,))


def test_isolated_vertices_and_no_edges():
    ro, ci, _ = k.csr_from_pairs(9, [1, 1, 4], [2, 4, 7])  # 0, 3, 5, 6, 8 are isolated
    _both_modes(9, ro, ci)
    for n, ro, ci in ((5, np.zeros(6, np.int32), np.array([], np.int32)), (1, np.array([0, 1], np.int32), np.array([0], np.int32))):
        for mode, classes in ((ga.LP_SYNC, None), (ga.LP_CLASSES, np.zeros(n, np.int32))):
            st = _check(n, ro, ci, mode=mode, classes=classes)
            assert (st["rounds"], st["state"], st["visits"], st["entries_read"]) == (0, ga.LP_CONVERGED, n, 0)
        assert ga.gunrock_label_propagation(n, ro, ci)[2:] == (n, ga.LP_CONVERGED, 0)


def test_int_max_weights_do_not_wrap():
    ro, ci, w = k.csr_from_pairs(5, [0, 0, 0, 0], [1, 2, 3, 4], [k.INT_MAX] * 4)
    st = _check(5, ro, ci, w, start=np.array([0, 1, 4, 4, 4], np.int32), max_rounds=1)  # 3 * INT_MAX for label 4 against INT_MAX for 1
    assert st["state"] == ga.LP_CAPPED
    assert ga.gunrock_label_propagation(5, ro, ci, w, mode=ga.LP_SYNC, labels=np.array([0, 1, 4, 4, 4], np.int32), max_rounds=1)[0][0] == 4


# ---------------- refusals ----------------

def test_refusals():
    ro, ci = np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32)
    for weight in (0, -3):
        with pytest.raises(RuntimeError, match="code -2"):
            ga.LpProblem().init(2, ro, ci, np.array([weight, weight], np.int32))
    ga.LpProblem().init(2, ro, ci, np.array([5, -3], np.int32)).close()  # (the pair's weight is the largest entry: 5)
    with pytest.raises(RuntimeError, match="code -1"):
        ga.LpProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.LpProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a decreasing offset
        ga.LpProblem().init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    p = ga.LpProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        p.init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, ro, ci)
    with pytest.raises(RuntimeError):  # and nothing runs on it
        p.reset()
    p.close()

    p = ga.LpProblem().init(2, ro, ci)
    with pytest.raises(RuntimeError, match="code -3"):  # a second init on a taken handle
        p.init(2, ro, ci)
    with pytest.raises(RuntimeError, match=NOT_READY):  # extract and summary before an Enact
        p.extract()
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.summary()
    with pytest.raises(RuntimeError, match="code -1"):  # a start label outside [0, nodes)
        p.reset(np.array([0, 2], np.int32))
    with pytest.raises(RuntimeError, match="code -1"):
        p.reset(np.array([-1, 0], np.int32))
    assert p.set_classes([0, 0]) == ga.LP_BAD_CLASSES  # improper: nothing is installed
    assert p.set_option("mode", ga.LP_CLASSES) == 0
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.enact()
    with pytest.raises(RuntimeError, match="code -1"):  # a class outside [0, num_classes)
        p.set_classes([0, 2], 2)
    assert p.set_classes([1, 0]) == 0
    p.enact()  # (an Enact without a Reset resets itself)
    assert p.extract()[0].tolist() == [0, 0]
    assert p.set_classes([1, 1]) == ga.LP_BAD_CLASSES  # and a refusal removes what was installed
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.enact()
    assert p.set_option("no_such_option", 1) == 1
    for name, value in (("mode", 2), ("mode", -1), ("strategy", 4), ("lane_max_row", -1), ("wave_max_row", -1), ("table_slots", 32),
                        ("table_slots", 96), ("table_slots", 2048), ("max_rounds", -1), ("max_rounds", float("nan"))):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    p.close()


# ---------------- options and scale ----------------

def test_options_change_no_result():
    g = o.rmat_seeded(12, 8 << 12)
    n, ro, ci = g.nodes, g.row_offsets, g.col_indices
    w = k.mod7_weights(n, ro, ci)
    a, b, _ = k.pairs_of(n, ro, ci, w)
    classes = k.greedy_classes(n, a, b)
    for options in ({"table_slots": 64}, {"lane_max_row": 0, "wave_max_row": 0}, {"lane_max_row": 2, "wave_max_row": 33, "table_slots": 128},
                    {"lane_max_row": 1 << 30}):
        _check(n, ro, ci, w, strategies=(ga.LP_AUTO,), **options)
        _check(n, ro, ci, w, ga.LP_CLASSES, classes, strategies=(ga.LP_AUTO,), **options)
    p = ga.LpProblem(instrument=True).init(n, ro, ci, w)
    p.set_option("mode", ga.LP_SYNC)
    p.reset()
    p.enact(max_grid_size=3)
    a, b, pw = k.pairs_of(n, ro, ci, w)
    st = _compare(p, n, a, b, pw, k.run_numpy(n, a, b, pw, k.SYNC), "instrumented, three workgroups")
    assert st["kernel_ms"] > 0 and st["build_ms"] > 0
    p.close()


def test_rmat16_device_built():
    """R-MAT at scale 16, built on the device, in both modes against the numpy form, which takes under a second per mode there."""
    import torch  # noqa: F401
    from gunrockinst_amd import devgraph
    d_ro, d_ci = devgraph.rmat_csr_device(16, 8)
    n, entries = 1 << 16, int(d_ci.shape[0])
    ro, ci = d_ro.cpu().numpy(), d_ci.cpu().numpy()
    a, b, pw = k.pairs_of(n, ro, ci)
    colours = ga.gunrock_color(n, ro, ci, seed=16)[0].astype(np.int32) - 1
    p = ga.LpProblem().init_device(n, entries, d_ro.data_ptr(), d_ci.data_ptr(), None)
    for mode, classes in ((ga.LP_SYNC, None), (ga.LP_CLASSES, colours)):
        ref = k.run_numpy(n, a, b, pw, mode, classes, None, 200)
        p.set_option("mode", mode)
        p.set_option("max_rounds", 200)
        if classes is not None:
            assert p.set_classes(classes) == 0
        p.reset()
        p.enact()
        st = _compare(p, n, a, b, pw, ref, "rmat16 mode %d" % mode)
        assert st["regime_rows"][1] > 0 and st["regime_rows"][2] > 0
    p.close()
