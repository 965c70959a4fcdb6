"""Maximal independent set and greedy colourings on the GPU (grx_mis_*): for every mode `ids` must equal the sequential greedy pass
of tests/_mis_checker.py bit for bit on every input -- fixtures, the golden MARKET files read undirected and directed, raw CSRs
of every awkward shape, caller priorities with ties, dependency chains as long as the graph, stars, R-MAT -- and the
device-built scale-22 R-MAT must satisfy the mode's equation at every vertex (the vectorised check; the solution is unique)."""
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

from _mis_checker import COLOR_FIRST_FIT, COLOR_ROUNDS, MODES, SET, greedy, higher, verify

pytestmark = pytest.mark.gpu


def _summary(mode, ids):
    return int(ids.sum()) if mode == SET else int(ids.max())


def _run_all(nodes, ro, ci, prio_or_seed):
    """{mode: (ids, summary, stats)} from one handle: Reset + Enact per mode"""
    seed = prio_or_seed if isinstance(prio_or_seed, (int, np.integer)) else 0
    prio = None if isinstance(prio_or_seed, (int, np.integer)) else prio_or_seed
    p = ga.MisProblem().init(nodes, ro, ci, prio, seed)
    out = {}
    for mode in MODES:
        p.reset()
        p.enact(mode)
        ids, summary = p.extract()
        out[mode] = (ids.copy(), summary, p.stats())
    p.close()
    return out


def _check(nodes, ro, ci, prio_or_seed):
    got = _run_all(nodes, ro, ci, prio_or_seed)
    for mode in MODES:
        ids, summary, _ = got[mode]
        ref = greedy(nodes, ro, ci, prio_or_seed, mode)
        assert ids.dtype == np.int32 and np.array_equal(ids, ref), "mode %d: ids differ from the greedy pass at %s" % (
            mode, np.flatnonzero(ids != ref)[:10])
        assert summary == _summary(mode, ref)
    return got


def test_fixture7(golden):
    f = golden["fixture7"]
    ro, ci = np.array(f["row_offsets"], np.int32), np.array(f["col_indices"], np.int32)
    got = _check(7, ro, ci, np.arange(7, dtype=np.int32))
    assert got[SET][0].tolist() == [0, 0, 1, 0, 0, 0, 1]
    assert got[COLOR_ROUNDS][0].tolist() == [6, 5, 4, 3, 3, 2, 1]
    assert got[COLOR_FIRST_FIT][0].tolist() == [4, 2, 1, 3, 3, 2, 1]
    for seed in (0, 1, 12345):
        _check(7, ro, ci, seed)


@pytest.mark.parametrize("name", ["bips98_606.mtx", "chesapeake.mtx", "test_bc.mtx", "test_cc.mtx", "test_pr.mtx"])
def test_market_files_undirected_and_directed(golden_dir, name):
    for und in (True, False):
        g = o.build_market(os.path.join(golden_dir, name), undirected=und)
        _check(g.nodes, g.row_offsets, g.col_indices, 0)
        _check(g.nodes, g.row_offsets, g.col_indices, 3)
        deg = np.diff(g.row_offsets).astype(np.int32)
        _check(g.nodes, g.row_offsets, g.col_indices, deg)  # largest degree first, ties by id


def test_raw_csrs():
    # unsorted rows and duplicates
    _check(4, np.array([0, 4, 6, 8, 9], np.int32), np.array([3, 1, 2, 1, 2, 0, 0, 1, 0], np.int32), 0)
    _check(4, np.array([0, 4, 6, 8, 9], np.int32), np.array([3, 1, 2, 1, 2, 0, 0, 1, 0], np.int32), np.array([1, 1, 0, 0], np.int32))
    # self-loops only, one vertex, no edges
    got = _check(3, np.array([0, 1, 3, 3], np.int32), np.array([0, 1, 1], np.int32), 0)
    assert got[SET][0].tolist() == [1, 1, 1] and got[COLOR_FIRST_FIT][0].tolist() == [1, 1, 1]
    _check(1, np.array([0, 1], np.int32), np.array([0], np.int32), 5)
    got = _check(1, np.array([0, 0], np.int32), np.array([], np.int32), 0)
    assert got[SET][0].tolist() == [1] and got[COLOR_ROUNDS][1] == 1
    got = _check(6, np.zeros(7, np.int32), np.array([], np.int32), 0)
    assert got[SET][1] == 6 and got[COLOR_ROUNDS][0].tolist() == [1] * 6
    # one-way edges only: the smallest case is {1 -> 0} (every unmirrored edge points from a higher to a lower id)
    for prio in (0, 1, 2, np.array([0, 0], np.int32), np.array([1, 0], np.int32)):
        got = _check(2, np.array([0, 0, 1], np.int32), np.array([0], np.int32), prio)
        assert sorted(got[SET][0].tolist()) == [0, 1] and sorted(got[COLOR_ROUNDS][0].tolist()) == [1, 2]
    _check(5, np.array([0, 0, 1, 2, 3, 4], np.int32), np.array([0, 1, 2, 3], np.int32), np.arange(5, dtype=np.int32))  # chain of one-way edges


def test_rejects_bad_input():
    with pytest.raises(RuntimeError, match="code -1"):
        ga.MisProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.MisProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a decreasing offset
        ga.MisProblem().init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not end at `edges` (nothing else wrong)
        ga.MisProblem().init(2, np.array([0, 1, 1], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not start at 0 (nothing else wrong)
        ga.MisProblem().init(2, np.array([1, 1, 1], np.int32), np.array([1], np.int32))
    p = ga.MisProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        p.init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    p.close()
    p = ga.MisProblem().init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    p.reset()
    with pytest.raises(RuntimeError, match="code -1"):  # not a mode
        p.enact(3)
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    p.close()


def _path(n, mirrored=True):
    if mirrored:
        rows = np.concatenate([np.arange(n - 1), np.arange(1, n)])
        cols = np.concatenate([np.arange(1, n), np.arange(n - 1)])
    else:
        rows, cols = np.arange(n - 1), np.arange(1, n)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    return np.searchsorted(rows, np.arange(n + 1)).astype(np.int32), cols.astype(np.int32)


def test_caller_priorities_equal_and_degree():
    g = o.rmat_seeded(12, 8 << 12, undirected=True)
    _check(g.nodes, g.row_offsets, g.col_indices, np.zeros(g.nodes, np.int32))                   # all equal: the id decides
    _check(g.nodes, g.row_offsets, g.col_indices, np.full(g.nodes, -(1 << 31), np.int32))
    _check(g.nodes, g.row_offsets, g.col_indices, np.diff(g.row_offsets).astype(np.int32))       # largest degree first
    _check(g.nodes, g.row_offsets, g.col_indices, (-np.diff(g.row_offsets)).astype(np.int32))    # smallest degree first
    rng = np.random.default_rng(5)
    _check(g.nodes, g.row_offsets, g.col_indices, rng.integers(-(1 << 31), 1 << 31, g.nodes, dtype=np.int64).astype(np.int32))


@pytest.mark.parametrize("mirrored", [True, False])
def test_path_with_a_dependency_chain_as_long_as_the_graph(mirrored):
    n = 20_000
    ro, ci = _path(n, mirrored)
    got = _check(n, ro, ci, np.arange(n, dtype=np.int32))  # prio = id: vertex v waits for v + 1
    assert got[COLOR_ROUNDS][0].tolist() == list(range(n, 0, -1))
    for mode in MODES:
        st = got[mode][2]
        print("path %d mode %d: %s" % (n, mode, st))
        # the chain must be walked on the device: a loop of one launch and one read-back per round would need ~n rounds
        assert st["rounds"] <= n // 16, st
    _check(n, ro, ci, 0)


def test_path_whose_chain_spans_several_tail_windows():
    n = 100_000  # prio = id: one chain through the whole list, longer than the window the device-side loop works on
    ro, ci = _path(n)
    got = _check(n, ro, ci, np.arange(n, dtype=np.int32))
    for mode in MODES:
        st = got[mode][2]
        print("path %d mode %d: %s" % (n, mode, st))
        assert st["rounds"] <= n // 16, st
        assert st["kernel_launches"] <= 4 * st["rounds"] + 64, st  # windows behind an unfinished one are not launched pass after pass


@pytest.mark.parametrize("mirrored", [True, False])
def test_star_with_100000_leaves_both_ways_round(mirrored):
    leaves = 100_000
    n = leaves + 1
    for centre in (0, n - 1):
        others = np.delete(np.arange(n), centre)
        rows = np.concatenate([others, np.full(leaves, centre)]) if mirrored else others
        cols = np.concatenate([np.full(leaves, centre), others]) if mirrored else np.full(leaves, centre)
        order = np.argsort(rows, kind="stable")
        rows, cols = rows[order], cols[order]
        ro = np.searchsorted(rows, np.arange(n + 1)).astype(np.int32)
        for first in (True, False):  # the centre has the largest key / the smallest key
            prio = np.zeros(n, np.int32)
            prio[centre] = 1 if first else -1
            got = _check(n, ro, cols.astype(np.int32), prio)
            assert got[SET][1] == (1 if first else leaves) and got[COLOR_FIRST_FIT][1] == 2
        _check(n, ro, cols.astype(np.int32), 9)


@pytest.mark.parametrize("undirected", [True, False])
def test_rmat16(undirected):
    g = o.rmat_seeded(16, 8 << 16, undirected=undirected)
    got = _check(g.nodes, g.row_offsets, g.col_indices, 0)
    for mode in MODES:
        print("rmat16 undirected=%s mode %d: summary %d %s" % (undirected, mode, got[mode][1], got[mode][2]))
    assert (got[COLOR_FIRST_FIT][0] <= got[COLOR_ROUNDS][0]).all()


def test_seeds_repeats_and_mode_switches():
    g = o.rmat_seeded(14, 8 << 14, undirected=True)
    a = _run_all(g.nodes, g.row_offsets, g.col_indices, 1)
    b = _run_all(g.nodes, g.row_offsets, g.col_indices, 2)
    assert not np.array_equal(a[SET][0], b[SET][0]), "two seeds gave the same set"
    p = ga.MisProblem(instrument=True).init(g.nodes, g.row_offsets, g.col_indices, None, 1)
    for mode in (SET, COLOR_FIRST_FIT, COLOR_ROUNDS, SET, COLOR_ROUNDS, COLOR_FIRST_FIT, COLOR_FIRST_FIT):  # one handle, any order
        p.reset()
        p.enact(mode)
        ids, summary = p.extract()
        assert ids.tobytes() == a[mode][0].tobytes() and summary == a[mode][1]
        trace = p.round_trace()
        st = p.stats()
        assert len(trace) == st["rounds"] and trace[0]["vertices"] == g.nodes and all(r["ms"] > 0 for r in trace)
        assert st["entries_read"] > 0 and st["kernel_launches"] >= st["rounds"]
    p.close()
    ids, size = ga.gunrock_mis(g.nodes, g.row_offsets, g.col_indices, seed=1)
    assert np.array_equal(ids, a[SET][0]) and size == a[SET][1]
    for first_fit, mode in ((True, COLOR_FIRST_FIT), (False, COLOR_ROUNDS)):
        ids, colours = ga.gunrock_color(g.nodes, g.row_offsets, g.col_indices, seed=1, first_fit=first_fit)
        assert np.array_equal(ids, a[mode][0]) and colours == a[mode][1]
    # the helper's priorities, passed back as the caller's, give the hashed order again when they are compared the same way:
    # (uint32 ^ 0x80000000) read as int32 keeps the unsigned order
    prio = (ga.mis_priorities(g.nodes, 1) ^ np.uint32(0x80000000)).view(np.int32)
    c = _run_all(g.nodes, g.row_offsets, g.col_indices, prio)
    for mode in MODES:
        assert np.array_equal(c[mode][0], a[mode][0])


def test_device_rmat22_init_device():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(22)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.MisProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    got = {}
    for mode in MODES:
        p.reset()
        p.enact(mode)
        ids, summary = p.extract()
        st = p.stats()
        p.reset()
        p.enact(mode)
        again, summary2 = p.extract()
        assert ids.tobytes() == again.tobytes() and summary == summary2
        got[mode] = (ids.copy(), summary)
        print("rmat22 mode %d: summary %d %s" % (mode, summary, st))
        assert st["entries_read"] >= m or mode == SET  # (a colouring reads every row entry; the set stops at a member)
    p.close()
    h_ro, h_ci = ro.cpu().numpy(), ci.cpu().numpy()
    del ro, ci
    graph = higher(n, h_ro, h_ci, 0)
    for mode in MODES:
        ids, summary = got[mode]
        assert verify(n, h_ro, h_ci, 0, mode, ids, graph=graph), "mode %d: the equation does not hold everywhere" % mode
        assert summary == _summary(mode, ids)
    assert (got[COLOR_FIRST_FIT][0] <= got[COLOR_ROUNDS][0]).all()
    assert got[COLOR_FIRST_FIT][1] <= int(np.diff(h_ro).max()) + 1
