"""Heavy-edge matching and graph contraction on the GPU (grx_matching_*): in_matching, mate, medge and the summary must equal
tests/_matching_checker.py's with np.array_equal under all three schedules, the round count must equal the rounds form's, and the
coarse graph must equal both contraction forms of the checker -- goldens read directed and undirected with three kinds of weights
and three seeds, raw CSRs of every awkward shape, sizes at the lane, wave and workgroup boundaries, rows around wave_min_row with
neighbours that get matched elsewhere (the cursor and the wave reduction), hubs, the monotone path that needs a round per pair, and
R-MAT at scale 16 and, device-built, at scale 20."""
import functools
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _matching_checker as k

pytestmark = pytest.mark.gpu

SCHEDULES = (ga.MATCHING_AUTO, ga.MATCHING_ROUNDS, ga.MATCHING_DEVICE_LOOP)
INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1


def _check_contract(p, n, a, b, pw, ref, vertex_weights=None):
    want = k.contract(n, a, b, pw, ref["mate"], vertex_weights)
    assert k.same_coarse(want, k.contract_sparse(n, a, b, pw, ref["mate"], vertex_weights))
    nc, ne = p.contract(vertex_weights)
    got = p.coarse_extract()
    assert (nc, ne) == (want[1], want[3].shape[0]) and k.same_coarse(got, want), "the coarse graph differs from the checker"
    return got


def _check(n, ro, ci, w=None, seed=0, schedules=SCHEDULES, contract=True, solved=None, **options):
    """the graph under every schedule on one handle, everything against the checker; returns the stats of the last run"""
    a, b, pw, ref, count = solved if solved is not None else k.solve(n, ro, ci, w, seed)
    p = ga.MatchingProblem().init(n, ro, ci, w, seed)
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    st = None
    for schedule in schedules:
        assert p.set_option("schedule", schedule) == 0
        p.reset()
        p.enact()
        bad = k.mismatches(p, n, a, b, pw, ref)
        assert not bad, "differs from the checker under schedule %d %s: %s" % (schedule, options, bad)
        st = p.stats()
        assert st["pairs"] == a.shape[0] and st["rounds"] == count, (st, count)
        kind, ran, live, matched = p.round_trace()
        assert int(matched.sum()) == ref["summary"]["matched"] and int(ran.sum()) in (count, count + 1)
        if schedule == ga.MATCHING_ROUNDS:
            assert (kind == ga.MATCHING_STEP_WIDE).all() and st["loop_rounds"] == 0 and st["kernel_launches"] == 2 * int(ran.sum())
        if schedule == ga.MATCHING_DEVICE_LOOP:
            assert (kind == ga.MATCHING_STEP_LOOP).all() and st["loop_rounds"] == int(ran.sum())
    if contract:
        _check_contract(p, n, a, b, pw, ref)
        _check_contract(p, n, a, b, pw, ref, (np.arange(n) * 7 % 11 - 2).astype(np.int32))
    p.close()
    return st


def _degree_weights(n, ro, ci):
    deg = np.diff(np.asarray(ro, np.int64))
    rows = np.repeat(np.arange(n), deg)
    return (deg[rows] + deg[np.asarray(ci, np.int64)]).astype(np.int32)


GOLDENS = ("fixture7", "test_bc", "test_cc", "test_pr", "chesapeake", "bips98_606")


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
        for seed in (0, 1, 12345):
            _check(n, ro, ci, w, seed, contract=seed == 1)


def test_pinned_literals(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    src, dst, in_matching, mate, matched, weight = ga.gunrock_matching(g.nodes, g.row_offsets, g.col_indices, k.mod7_weights(g.nodes, g.row_offsets, g.col_indices))
    assert (src.shape[0], matched, weight) == (170, 18, 108) and int(in_matching.sum()) == 18 and int((mate >= 0).sum()) == 36
    g = o.rmat_seeded(12, 8 << 12)
    src, dst, in_matching, mate, matched, weight = ga.gunrock_matching(g.nodes, g.row_offsets, g.col_indices, seed=1)
    assert (src.shape[0], matched, weight) == (27791, 825, 825)
    assert np.array_equal(mate[src[in_matching == 1]], dst[in_matching == 1])


def test_unsorted_rows():
    rng = np.random.default_rng(3)
    rows, cols = rng.integers(0, 300, 2000), rng.integers(0, 300, 2000)
    ro, ci, w = k.csr_from_pairs(300, rows, cols, rng.integers(-5, 6, 2000), shuffle=rng)
    _check(300, ro, ci, w, 7)
    _check(300, ro, ci, None, 7)


def test_duplicates_with_different_weights_take_the_largest():
    # pair {0, 1}: entries 3, 9 and 5 -> 9; pair {1, 2}: -4 and -6 -> -4; pair {2, 3}: 9 one way only, and a heavy self-loop
    rows, cols, w = [0, 0, 1, 1, 2, 2, 3], [1, 1, 0, 2, 1, 3, 3], [3, 9, 5, -4, -6, 9, INT_MAX]
    ro, ci, w = k.csr_from_pairs(4, rows, cols, w, mirror=False)
    a, b, pw, ref, _ = k.solve(4, ro, ci, w, 0)
    assert pw.tolist() == [9, -4, 9]
    _check(4, ro, ci, w, 0)
    p = ga.MatchingProblem().init(4, ro, ci, w, 0)
    assert p.pairs()[2].tolist() == [9, -4, 9]
    p.close()


def test_one_way_entries_only():
    g = o.rmat_seeded(8, 8 << 8, undirected=False)
    rows = np.repeat(np.arange(g.nodes), np.diff(g.row_offsets))
    keep = rows < g.col_indices  # the upper triangle alone, then the lower alone
    for r, c in ((rows[keep], g.col_indices[keep]), (g.col_indices[keep], rows[keep])):
        ro, ci, _ = k.csr_from_pairs(g.nodes, r, c, mirror=False)
        _check(g.nodes, ro, ci, None, 2)


def test_degenerate_graphs():
    _check(3, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32), np.array([5, 6, 7], np.int32))  # self-loops only
    _check(1, np.array([0, 0], np.int32), np.array([], np.int32))                                             # one vertex
    _check(1, np.array([0, 1], np.int32), np.array([0], np.int32))
    _check(5, np.zeros(6, np.int32), np.array([], np.int32))                                                  # no edges
    st = _check(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    assert st["rounds"] == 1


@pytest.mark.parametrize("value", (INT_MIN, INT_MAX, 0, -1))
def test_extreme_and_equal_weights(value):
    g = o.rmat_seeded(9, 8 << 9)
    w = np.full(g.col_indices.shape[0], value, np.int32)
    _check(g.nodes, g.row_offsets, g.col_indices, w, 5, contract=False)
    rng = np.random.default_rng(9)
    mixed = rng.choice(np.array([INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 1, INT_MAX]), g.col_indices.shape[0]).astype(np.int32)
    _check(g.nodes, g.row_offsets, g.col_indices, mixed, 5, contract=False)


@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257, 1025))
def test_paths_and_cycles(n):
    rng = np.random.default_rng(n)
    for closed in (False, True):
        rows, cols = np.arange(n - 1 + closed), (np.arange(n - 1 + closed) + 1) % n
        for w in (None, rng.integers(1, 4, rows.shape[0]), np.arange(rows.shape[0])):
            ro, ci, we = k.csr_from_pairs(n, rows, cols, w)
            _check(n, ro, ci, we, n, contract=w is None)


def _broom(degree, rng):
    """a hub with `degree` leaves, each leaf with a partner of its own: most leaves are matched away from the hub, which then walks on"""
    leaves, partners = np.arange(1, degree + 1), np.arange(degree + 1, 2 * degree + 1)
    rows = np.concatenate([np.zeros(degree, np.int64), leaves])
    cols = np.concatenate([leaves, partners])
    w = np.concatenate([rng.integers(1, 6, degree), rng.integers(1, 10, degree)])
    return (2 * degree + 1,) + k.csr_from_pairs(2 * degree + 1, rows, cols, w)


@pytest.mark.parametrize("degree", (15, 16, 17, 63, 64, 65, 4097))
def test_rows_around_wave_min_row(degree):
    rng = np.random.default_rng(degree)
    n, ro, ci, w = _broom(degree, rng)
    solved = k.solve(n, ro, ci, w, 1)
    for wave_min_row in (16, 1, 64, 65, 1 << 30):
        _check(n, ro, ci, w, 1, solved=solved, contract=wave_min_row == 16, wave_min_row=wave_min_row)
    _check(n, ro, ci, None, 1)


def test_star_of_70000_leaves():
    n = 70001
    ro, ci, _ = k.csr_from_pairs(n, np.zeros(n - 1, np.int64), np.arange(1, n))
    st = _check(n, ro, ci, None, 3, schedules=(ga.MATCHING_AUTO, ga.MATCHING_ROUNDS))
    assert st["rounds"] == 1
    p = ga.MatchingProblem().init(n, ro, ci, None, 3)
    p.reset()
    p.enact()
    assert p.summary() == {"pairs": n - 1, "matched": 1, "weight": 1, "unmatched": n - 2, "unmatched_with_neighbours": n - 2}
    p.close()


def test_two_hubs_sharing_5000_leaves():
    leaves = np.arange(2, 5002)
    rows = np.concatenate([np.zeros(5000, np.int64), np.ones(5000, np.int64)])
    cols = np.concatenate([leaves, leaves])
    rng = np.random.default_rng(11)
    for w in (None, rng.integers(1, 3, 10000)):
        ro, ci, we = k.csr_from_pairs(5002, rows, cols, w)
        st = _check(5002, ro, ci, we, 4)
        assert st["pairs"] == 10000


@functools.lru_cache(maxsize=None)
def _monotone_path(n):
    ro, ci, w = k.path(n, np.arange(n - 1) + 1)
    solved = k.solve(n, ro, ci, w, 0)
    for x in (ro, ci, w) + solved[:3] + tuple(solved[3][name] for name in ("in_matching", "mate", "medge")):
        x.setflags(write=False)
    return ro, ci, w, solved


def test_monotone_path_of_20001_vertices():
    n = 20001
    ro, ci, w, solved = _monotone_path(n)
    assert solved[4] == 10000 and solved[3]["summary"]["matched"] == 10000
    p = ga.MatchingProblem().init(n, ro, ci, w, 0)
    for schedule in (ga.MATCHING_ROUNDS, ga.MATCHING_AUTO):
        p.set_option("schedule", schedule)
        p.reset()
        p.enact()
        assert not k.mismatches(p, n, *solved[:4])
        st = p.stats()
        assert st["rounds"] == 10000, "the round count is the rounds form's"
        if schedule == ga.MATCHING_ROUNDS:
            assert st["kernel_launches"] == 2 * 10001 and st["loop_rounds"] == 0, "a launch pair per round and the closing one"
        else:
            assert st["kernel_launches"] <= 4 and st["loop_rounds"] == 10001, "the device loop runs them all"
        assert st["polls"] > 0 and st["entries_read"] <= 4 * 2 * (n - 1), "waiting vertices poll: nobody walks a row again and again"
    p.close()


def test_max_rounds_gives_up_and_the_handle_goes_on():
    n = 2001
    ro, ci, w, solved = _monotone_path(n)
    p = ga.MatchingProblem().init(n, ro, ci, w, 0)
    for schedule in SCHEDULES:
        p.set_option("schedule", schedule)
        assert p.set_option("max_rounds", 1) == 0
        p.reset()
        with pytest.raises(ga.MatchingGaveUp, match="code -4"):
            p.enact()
        with pytest.raises(RuntimeError):  # no result to read
            p.extract()
        with pytest.raises(RuntimeError, match="code -1"):
            p.contract()
        assert p.set_option("max_rounds", 0) == 0  # the derived bound again: n / 2 + 1
        p.reset()
        p.enact()
        assert not k.mismatches(p, n, *solved[:4]) and p.stats()["rounds"] == 1000
    p.close()


@functools.lru_cache(maxsize=None)
def _rmat12():
    g = o.rmat_seeded(12, 8 << 12)
    return g.nodes, g.row_offsets, g.col_indices


def test_rmat16_device_built():
    import torch
    from gunrockinst_amd import devgraph
    d_ro, d_ci = devgraph.rmat_csr_device(16, 8)
    n, entries = 1 << 16, int(d_ci.shape[0])
    ro, ci = d_ro.cpu().numpy(), d_ci.cpu().numpy()
    d_w = torch.as_tensor(k.mod7_weights(n, ro, ci), device="cuda")
    for w, ptr in ((d_w.cpu().numpy(), d_w.data_ptr()),):  # (without weights: the scale-20 test below)
        a, b, pw, ref, count = k.solve(n, ro, ci, w, 16)
        p = ga.MatchingProblem().init_device(n, entries, d_ro.data_ptr(), d_ci.data_ptr(), ptr, seed=16)
        for schedule in SCHEDULES:
            p.set_option("schedule", schedule)
            p.reset()
            p.enact()
            assert not k.mismatches(p, n, a, b, pw, ref) and p.stats()["rounds"] == count
        _check_contract(p, n, a, b, pw, ref)
        p.close()


def test_rmat20_device_built_satisfies_the_equation():
    from gunrockinst_amd import devgraph
    d_ro, d_ci = devgraph.rmat_csr_device(20, 8)
    n = 1 << 20
    p = ga.MatchingProblem().init_device(n, int(d_ci.shape[0]), d_ro.data_ptr(), d_ci.data_ptr(), None, seed=20)
    p.reset()
    p.enact()
    a, b, pw = p.pairs()
    got, s = p.extract(), p.summary()
    assert (pw == 1).all() and (a < b).all() and s["pairs"] == a.shape[0] == p.stats()["pairs"]
    assert not k.verify(n, a, b, pw, 20, got["in_matching"], got["mate"], got["medge"])
    assert s["matched"] == int(got["in_matching"].sum()) == s["weight"] and s["unmatched"] == n - 2 * s["matched"]
    nc, ne = p.contract()
    assert nc == n - s["matched"]
    cmap, _, cro, cci, cw, vweight = p.coarse_extract()
    assert int(vweight.sum()) == n and int(vweight.max()) == 2 and cro[-1] == ne == cci.shape[0]
    inside = int((cmap[a] == cmap[b]).sum())
    assert inside == s["matched"] and int(cw.astype(np.int64).sum()) == 2 * (a.shape[0] - inside), "every fine pair lands on one coarse pair"
    p.close()


def test_three_levels_of_coarsening():
    n, ro, ci = _rmat12()
    w = k.mod7_weights(n, ro, ci)
    vw = (np.arange(n) % 3 + 1).astype(np.int32)
    levels = ga.gunrock_coarsen(n, ro, ci, w, vw, seed=2, levels=3)
    assert len(levels) == 3
    for cmap, nc, cro, cci, cw, vweight in levels:  # each level on its own: the checker on the level's input
        a, b, pw, ref, _ = k.solve(n, ro, ci, w, 2)
        want = k.contract(n, a, b, pw, ref["mate"], vw)
        assert k.same_coarse((cmap, nc, cro, cci, cw, vweight), want) and k.same_coarse(want, k.contract_sparse(n, a, b, pw, ref["mate"], vw))
        assert nc < n and int(vweight.sum()) == int(vw.sum())
        n, ro, ci, w, vw = nc, cro, cci, cw, vweight
    # a graph without edges matches nothing: one level, then it stops
    levels = ga.gunrock_coarsen(4, np.zeros(5, np.int32), np.array([], np.int32), levels=3)
    assert len(levels) == 1 and levels[0][1] == 4 and levels[0][0].tolist() == [0, 1, 2, 3] and levels[0][5].tolist() == [1, 1, 1, 1]


def test_contraction_overflow_and_order_of_calls():
    ro, ci, w = k.csr_from_pairs(3, [0, 0, 1], [1, 2, 2], [INT_MAX, 2 ** 30, 2 ** 30])
    p = ga.MatchingProblem().init(3, ro, ci, w, 0)
    with pytest.raises(RuntimeError, match="code -1"):  # before an Enact
        p.contract()
    p.reset()
    with pytest.raises(RuntimeError, match="code -1"):
        p.contract()
    p.enact()
    assert p.extract()["mate"].tolist() == [1, 0, -1]
    with pytest.raises(ga.MatchingOverflow, match="code -5"):  # 2^30 + 2^30 on the one coarse pair
        p.contract()
    with pytest.raises(RuntimeError):  # nothing is kept
        p.coarse_extract()
    with pytest.raises(ga.MatchingOverflow):
        p.contract(np.array([INT_MAX, 1, 0], np.int32))
    p.close()
    ro, ci, w = k.csr_from_pairs(3, [0, 0, 1], [1, 2, 2], [INT_MAX, 2 ** 30, 2 ** 30 - 1])
    p = ga.MatchingProblem().init(3, ro, ci, w, 0)
    p.reset()
    p.enact()
    with pytest.raises(ga.MatchingOverflow):  # the pair weights fit, the vertex weights do not
        p.contract(np.array([INT_MAX, 1, 0], np.int32))
    assert p.contract(np.array([INT_MAX, 0, INT_MIN], np.int32)) == (2, 2)
    cmap, nc, cro, cci, cw, vweight = p.coarse_extract()
    assert cmap.tolist() == [0, 0, 1] and cro.tolist() == [0, 1, 2] and cci.tolist() == [1, 0] and cw.tolist() == [INT_MAX, INT_MAX]
    assert vweight.tolist() == [INT_MAX, INT_MIN]
    p.close()


def test_rejects_bad_input():
    with pytest.raises(RuntimeError, match="code -1"):
        ga.MatchingProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.MatchingProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a decreasing offset
        ga.MatchingProblem().init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not end at `edges` (nothing else wrong)
        ga.MatchingProblem().init(2, np.array([0, 1, 1], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not start at 0 (nothing else wrong)
        ga.MatchingProblem().init(2, np.array([1, 1, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(ValueError):  # a weight per entry
        ga.MatchingProblem().init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1], np.int32))
    p = ga.MatchingProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        p.init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError):  # and nothing runs on it
        p.reset()
    p.close()
    p = ga.MatchingProblem().init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    assert p.set_option("no_such_option", 1) == 1
    for name, value in (("schedule", 3), ("schedule", -1), ("wave_min_row", 0), ("max_rounds", -1), ("loop_max_list", -1),
                        ("loop_max_entries", -1), ("max_rounds", float("nan"))):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    p.enact()  # (an Enact without a Reset resets itself)
    assert p.extract()["mate"].tolist() == [1, 0]
    p.close()


def test_options_change_no_result():
    n, ro, ci = _rmat12()
    w = k.mod7_weights(n, ro, ci)
    solved = k.solve(n, ro, ci, w, 1)
    for options in ({"loop_max_list": 0}, {"loop_max_entries": 0}, {"loop_max_list": 1 << 30, "loop_max_entries": 1 << 30},
                    {"loop_max_list": 64, "loop_max_entries": 1000, "wave_min_row": 2}):
        _check(n, ro, ci, w, 1, solved=solved, contract=False, **options)
    p = ga.MatchingProblem(instrument=True).init(n, ro, ci, w, 1)
    p.reset()
    p.enact(max_grid_size=3)
    assert not k.mismatches(p, n, *solved[:4]) and p.stats()["kernel_ms"] > 0 and p.stats()["build_ms"] > 0
    p.close()
