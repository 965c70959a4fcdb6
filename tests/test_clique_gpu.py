"""k-clique counting on the GPU (grx_clique_*), k = 3 .. 6: `cliques` and `total` must equal tests/_clique_checker.py's recursion or
its closed forms, int64 against int64 with np.array_equal, and must not move under anything that is not the graph: the regime, the
bitmap budget, the rank that orients the build, the form the CSR comes in.

The regime test orients its graphs by a seeded random permutation.  Without a rank the longest out-rows of rmat(10, 8 << 10) and of
the multipartite graph (7, 9, 11, 13, 40) are 29 and 40 (computed on the CPU from the (d, id) order), so no automatic run at
bitmap_rows = 64 could fill both regimes; under the permutation their out-rows reach 187 and 66 with dozens at or below 32, and K_70
has one row of every length 0 .. 69 under any order.  That both regimes took rows is asserted from stats, as the rows' lengths
are."""
import os
from math import comb

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

from _clique_checker import (complete_counts, complete_graph, count, grid_graph, multipartite_counts, multipartite_graph,
                             tree_graph)
from _tc_checker import csr_of, simple_edges

pytestmark = pytest.mark.gpu

KS = (3, 4, 5, 6)
STRATEGIES = (ga.CLIQUE_AUTO, ga.CLIQUE_BITMAP, ga.CLIQUE_LIST)
NOT_READY = "code 600"  # hipErrorNotReady


def _run(p, k, **options):
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    p.reset()
    p.enact(k)
    cl, total = p.extract()
    assert cl.dtype == np.int64 and int(cl.sum()) == k * total
    assert p.extract(cliques=False) == (None, total)
    return cl.copy(), total, p.stats()


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), "%s: cliques differ at %s" % (what, np.flatnonzero(got[0] != want[0])[:10])
    assert got[1] == want[1], what


@pytest.fixture(scope="module")
def chesapeake(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    return g.nodes, g.row_offsets, g.col_indices


@pytest.fixture(scope="module")
def rmat10():
    g = o.rmat_seeded(10, 8 << 10)
    return g.nodes, g.row_offsets, g.col_indices, {k: count(g.nodes, g.row_offsets, g.col_indices, k) for k in (4, 5)}


def test_chesapeake(chesapeake):
    n, ro, ci = chesapeake
    p = ga.CliqueProblem().init(n, ro, ci)
    for k in KS:
        ref = count(n, ro, ci, k)
        for strategy in STRATEGIES:
            got = _run(p, k, strategy=strategy)
            _same(got, ref, "k %d strategy %d" % (k, strategy))
        _same(ga.gunrock_cliques(n, ro, ci, k), ref)
    tri, total = ga.gunrock_tc(n, ro, ci)
    cl, got_total, _ = _run(p, 3, strategy=ga.CLIQUE_AUTO)
    p.close()
    assert cl.tobytes() == tri.tobytes() and got_total == total == 194


@pytest.mark.parametrize("n", [1, 2, 5, 6, 33, 34, 65, 66, 70])
def test_word_borders(n):
    """K_n: out-rows of every length 0 .. n - 1, across the 32- and 64-bit borders of a bit row; k > n gives zeros"""
    ro, ci = complete_graph(n)
    p = ga.CliqueProblem().init(n, ro, ci)
    for k in KS:
        got = _run(p, k)
        _same(got, complete_counts(n, k), "K_%d k %d" % (n, k))
        if k > n:
            assert got[1] == 0 and not got[0].any()
        assert got[2]["max_out_row"] == n - 1 and got[2]["list_rows"] == 0
        assert got[2]["bound"] == comb(n, k)
    p.close()


def _regimes_agree(n, ro, ci, refs, label):
    rank = np.random.default_rng(1).permutation(n).astype(np.int32)
    p = ga.CliqueProblem().init(n, ro, ci, rank)
    for k in (4, 5):
        for rows in (32, 64, 512):
            for strategy in STRATEGIES:
                got = _run(p, k, strategy=strategy, bitmap_rows=rows)
                _same(got, refs[k], "%s k %d bitmap_rows %d strategy %d" % (label, k, rows, strategy))
                st = got[2]
                assert 0 < st["bitmap_edges"] + st["list_edges"] <= st["oriented_edges"]  # (rows below k - 1 entries are left out)
                if strategy == ga.CLIQUE_AUTO and rows < 512:
                    assert st["bitmap_rows"] > 0 and st["list_rows"] > 0 and st["bit_ands"] > 0 and st["list_lookups"] > 0, st
                    assert rows < st["max_out_row"]
                if strategy == ga.CLIQUE_LIST:
                    assert st["bitmap_rows"] == 0 and st["bit_ands"] == 0 and st["list_lookups"] > 0, st
                if strategy == ga.CLIQUE_BITMAP:
                    assert st["list_rows"] == 0 and st["list_lookups"] == 0, st
    p.close()


def test_regimes_agree_rmat(rmat10):
    n, ro, ci, refs = rmat10
    _regimes_agree(n, ro, ci, refs, "rmat10")


def test_regimes_agree_multipartite():
    parts = (7, 9, 11, 13, 40)
    n, (ro, ci) = multipartite_graph(parts)
    _regimes_agree(n, ro, ci, {k: multipartite_counts(parts, k) for k in (4, 5)}, "multipartite")


def test_regimes_agree_k70():
    ro, ci = complete_graph(70)
    _regimes_agree(70, ro, ci, {k: complete_counts(70, k) for k in (4, 5)}, "K_70")


def test_orientation_changes_nothing(rmat10, chesapeake):
    for n, ro, ci in (rmat10[:3], chesapeake):
        core, _ = ga.gunrock_kcore(n, ro, ci)
        ranks = {"none": None, "core": core, "permutation": np.random.default_rng(5).permutation(n).astype(np.int32),
                 "negative": np.full(n, -7, np.int32)}
        results = {}
        for name, rank in ranks.items():
            p = ga.CliqueProblem().init(n, ro, ci, rank)
            results[name] = {k: _run(p, k) for k in (3, 4, 5)}
            p.close()
        ref = {k: count(n, ro, ci, k) for k in (3, 4, 5)}
        for name in ranks:
            for k in (3, 4, 5):
                _same(results[name][k], ref[k], "rank %s k %d" % (name, k))
        m = simple_edges(n, ro, ci)[0].shape[0]
        for name in ("none", "negative"):  # all equal: TC's order and its bound
            assert results[name][4][2]["max_out_row"] ** 2 <= 2 * m
        assert results["none"][4][2]["max_out_row"] == results["negative"][4][2]["max_out_row"]
        assert all(results[name][4][2]["oriented_edges"] == m for name in ranks)


def test_core_rank_keeps_out_rows_within_the_degeneracy(rmat10, chesapeake):
    """With core numbers as the rank, stats' longest out-row is at most the degeneracy.

    (core, d, id) alone does not give that -- 29 against 24 on rmat(10, 8 << 10), 8 against 6 on chesapeake -- so the build breaks the
    rank's ties by a peel.  A tree and a grid peel over many rounds inside one shell; in K_70 and the multipartite graph every
    vertex of a shell leaves at once."""
    tree, grid = tree_graph(600, 3), grid_graph(23)
    parts = multipartite_graph((7, 9, 11, 13, 40))
    graphs = [rmat10[:3], chesapeake, (tree[0],) + tuple(tree[1]), (grid[0],) + tuple(grid[1]), (70,) + tuple(complete_graph(70)),
              (parts[0],) + tuple(parts[1])]
    figures = []
    for n, ro, ci in graphs:
        core, degeneracy = ga.gunrock_kcore(n, ro, ci)
        p = ga.CliqueProblem().init(n, ro, ci, core)
        figures.append((p.stats()["max_out_row"], degeneracy))
        _same(_run(p, 4)[:2], ga.gunrock_cliques(n, ro, ci, 4))
        p.close()
    print("longest out-row under core numbers, degeneracy:", figures)
    assert [d for _, d in figures][2:] == [1, 2, 69, 40]
    for longest, degeneracy in figures:
        assert longest <= degeneracy, figures


def test_input_forms():
    rng = np.random.default_rng(11)
    n = 150  # G(n, 0.25) on the first 140 vertices; the last 10 are isolated
    a, b = np.nonzero(np.triu(rng.random((140, 140)) < 0.25, 1))
    both_r, both_c = np.concatenate([a, b]), np.concatenate([b, a])
    shuffle = rng.permutation(both_r.shape[0])
    dup = rng.integers(0, a.shape[0], 300)
    loops = rng.integers(0, n, 40)
    one_way = rng.random(a.shape[0]) < 0.5
    forms = {
        "mirrored": csr_of(n, both_r, both_c),
        "upper": csr_of(n, a, b),
        "one-way": csr_of(n, np.where(one_way, a, b), np.where(one_way, b, a)),
        "shuffled": csr_of(n, both_r[shuffle], both_c[shuffle]),
        "duplicates": csr_of(n, np.concatenate([both_r, a[dup], b[dup]]), np.concatenate([both_c, b[dup], a[dup]])),
        "loops": csr_of(n, np.concatenate([loops, a, loops]), np.concatenate([loops, b, loops])),
    }
    for k in (3, 4, 5):
        ref = count(n, *forms["mirrored"], k)
        assert ref[1] > 0 and not ref[0][140:].any()
        for name, (ro, ci) in forms.items():
            _same(ga.gunrock_cliques(n, ro, ci, k), ref, "%s k %d" % (name, k))
    for k in KS:
        cl, total = ga.gunrock_cliques(1, np.array([0, 0], np.int32), np.array([], np.int32), k)
        assert cl.tolist() == [0] and total == 0
        cl, total = ga.gunrock_cliques(3, np.array([0, 1, 3, 3], np.int32), np.array([0, 1, 1], np.int32), k)  # only self-loops
        assert cl.tolist() == [0, 0, 0] and total == 0


def test_large_lds():
    """K_1000 forced into the bitmap regime: a 1000-row matrix, about 125 KiB, beyond what a launch gets unasked"""
    n = 1000
    ro, ci = complete_graph(n)
    p = ga.CliqueProblem().init(n, ro, ci)
    for k in (3, 4):
        got = _run(p, k, strategy=ga.CLIQUE_BITMAP, bitmap_rows=1024)
        _same(got, complete_counts(n, k), "K_1000 k %d" % k)
        assert got[2]["list_rows"] == 0 and got[2]["bitmap_rows"] == n - (k - 1) and got[2]["max_out_row"] == n - 1
    p.close()


def test_forced_bitmap_leaves_rows_beyond_1024_to_the_list_regime():
    n = 1100  # K_n: one out-row of every length 0 .. 1099, 75 of them beyond 1024
    ro, ci = complete_graph(n)
    p = ga.CliqueProblem().init(n, ro, ci)
    got = _run(p, 3, strategy=ga.CLIQUE_BITMAP, bitmap_rows=32)
    p.close()
    _same(got, complete_counts(n, 3), "K_1100")
    assert got[2]["list_rows"] == 75 and got[2]["bitmap_rows"] == 1023 and got[2]["list_lookups"] > 0


def test_overflow_is_refused():
    ro, ci = complete_graph(70)
    p = ga.CliqueProblem().init(70, ro, ci)
    assert p.set_option("count_limit", 1e6) == 0
    p.reset()
    with pytest.raises(ga.CliqueOverflow):
        p.enact(5)
    assert p.stats()["bound"] == comb(70, 5) == 12_103_014
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.extract()
    _same(_run(p, 3), complete_counts(70, 3))  # C(70, 3) = 54 740 is below the limit
    assert p.stats()["bound"] == 54_740
    with pytest.raises(ga.CliqueOverflow):  # refused again, and without a reset: the k = 3 result is gone
        p.enact(5)
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.extract()
    assert p.set_option("count_limit", 2.0 ** 62) == 0  # the default
    p.enact(5)  # the same handle takes the next Enact
    _same(p.extract(), complete_counts(70, 5))
    assert p.extract()[1] == 12_103_014
    for bad in (0, -1, 2.0 ** 63):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option("count_limit", bad)
    p.close()


def test_handle_protocol(rmat10):
    n, ro, ci, refs = rmat10
    p = ga.CliqueProblem(instrument=True).init(n, ro, ci)
    first = _run(p, 4)
    second = _run(p, 4)
    assert first[0].tobytes() == second[0].tobytes() and first[1] == second[1]
    _same(first, refs[4])
    assert second[2]["kernel_ms"] > 0 and second[2]["build_ms"] > 0 and second[2]["kernel_launches"] >= 2
    assert p.enact(5) > 0  # no reset between: Enact clears what the last one wrote
    _same(p.extract(), refs[5])
    assert p.enact(4) > 0
    _same(p.extract(), refs[4])
    p.reset()
    with pytest.raises(RuntimeError, match=NOT_READY):  # a reset leaves no result
        p.extract()
    for k in (2, 7, 0, -3):
        with pytest.raises(RuntimeError, match="code -1"):
            p.enact(k)
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(n, ro, ci)
    assert p.set_option("no_such_option", 1) == 1
    for name, bad in (("bitmap_rows", 16), ("bitmap_rows", 2048), ("strategy", 3), ("strategy", -1)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, bad)
    assert p.set_option("bitmap_rows", 32) == 0 and p.set_option("bitmap_rows", 1024) == 0
    p.close()
    p = ga.CliqueProblem()
    for call in (p.reset, lambda: p.enact(4), p.extract):  # before Init: an error code, nothing touched
        with pytest.raises(RuntimeError, match=NOT_READY):
            call()
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that decrease
        p.init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.enact(3)
    p.close()
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.CliqueProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -1"):
        ga.CliqueProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    with pytest.raises(ValueError):  # a rank for every vertex
        ga.CliqueProblem().init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.zeros(3, np.int32))


def test_init_device_and_device_results():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(10)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    h_ro, h_ci = ro.cpu().numpy(), ci.cpu().numpy()
    rank = np.random.default_rng(3).permutation(n).astype(np.int32)
    d_rank = torch.from_numpy(rank).cuda()
    torch.cuda.synchronize()
    for h_rank, dev_rank in ((None, None), (rank, d_rank.data_ptr())):
        p = ga.CliqueProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr(), dev_rank)
        q = ga.CliqueProblem().init(n, h_ro, h_ci, h_rank)
        for k in (3, 4):
            got, host = _run(p, k), _run(q, k)
            d_cl, d_deg = p.device_results()
            on_device = devgraph.as_tensor(d_cl, n, "<i8").cpu().numpy()
            degrees = devgraph.as_tensor(d_deg, n, "<i4").cpu().numpy()
            assert on_device.dtype == np.int64 and np.array_equal(on_device, got[0])
            _same(got, host[:2], "device against host, k %d" % k)
            assert got[2]["max_out_row"] == host[2]["max_out_row"]
            a, b = simple_edges(n, h_ro, h_ci)
            assert np.array_equal(degrees.astype(np.int64), np.bincount(a, minlength=n) + np.bincount(b, minlength=n))
        _same(got, count(n, h_ro, h_ci, 4))
        p.close()
        q.close()
