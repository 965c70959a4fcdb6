"""Triangle counting and clustering coefficients on the GPU (grx_tc_*): `triangles` must equal the numpy restatement of
tests/_tc_checker.py on every input, int64 against int64 with np.array_equal -- goldens read undirected and directed, raw CSRs of
every awkward shape, R-MAT, complete graphs whose total exceeds 2^32, every strategy and a tiny staging budget -- and the
device-built scale-22 R-MAT, too large for a CPU count, must satisfy invariants a wrong kernel breaks."""
import math
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

from _tc_checker import clustering, complete, hub_and_cliques, local_count, oriented, simple_edges

pytestmark = pytest.mark.gpu

STRATEGIES = (ga.TC_AUTO, ga.TC_LANE, ga.TC_LDS, ga.TC_GLOBAL)
# (total, max per vertex): computed on the CPU by both checker forms; the same read undirected and directed
LITERALS = {"chesapeake.mtx": (194, 71), "bips98_606.mtx": (10743, 52), "test_bc.mtx": (7, 5), "test_cc.mtx": (9, 5),
            "test_pr.mtx": (4, 3)}


def _run(p, **options):
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    p.reset()
    p.enact()
    tri, total = p.extract()
    assert tri.dtype == np.int64
    return tri.copy(), total, p.stats()


def _bound(st):
    assert st["max_out_row"] <= math.isqrt(2 * st["oriented_edges"]), st


def _check(nodes, ro, ci, **options):
    """one run against the checker: counts, total, the largest out-row and its bound, coefficients"""
    p = ga.TcProblem().init(nodes, ro, ci)
    tri, total, st = _run(p, **options)
    coeff, trans = p.clustering()
    only_total = p.extract(triangles=False)
    only_trans = p.clustering(coefficients=False)
    p.close()
    ref, ref_total, d, longest, _ = oriented(nodes, ro, ci)
    assert np.array_equal(tri, ref), "triangles differ from the checker at %s" % np.flatnonzero(tri != ref)[:10]
    assert total == ref_total and int(tri.sum()) == 3 * total
    assert st["oriented_edges"] == simple_edges(nodes, ro, ci)[0].shape[0] and st["max_out_row"] == longest
    _bound(st)
    ref_coeff, ref_trans = clustering(ref, d, ref_total)
    assert coeff.dtype == np.float64 and coeff.tobytes() == ref_coeff.tobytes() and trans == ref_trans
    assert only_total == (None, total) and only_trans == (None, trans)
    return tri, total, st


@pytest.mark.parametrize("name", sorted(LITERALS))
def test_goldens_undirected_and_directed(golden_dir, name):
    for und in (True, False):
        g = o.build_market(os.path.join(golden_dir, name), undirected=und)
        tri, total, _ = _check(g.nodes, g.row_offsets, g.col_indices)
        assert (total, int(tri.max())) == LITERALS[name]
        for strategy in STRATEGIES[1:]:
            other, _, _ = _check(g.nodes, g.row_offsets, g.col_indices, strategy=strategy, lds_entries=5)
            assert other.tobytes() == tri.tobytes()


@pytest.mark.parametrize("scale,total,most,longest", [(12, 123380, 14060, 48), (16, 2947873, 186415, 129)])
def test_rmat_literals(scale, total, most, longest):
    for und in (True, False):
        g = o.rmat_seeded(scale, 8 << scale, undirected=und)
        tri, got, st = _check(g.nodes, g.row_offsets, g.col_indices)
        assert (got, int(tri.max()), st["max_out_row"]) == (total, most, longest)
        print("rmat%d undirected=%s: %s" % (scale, und, st))


def test_raw_csrs():
    # unsorted rows and duplicates
    tri, total, _ = _check(4, np.array([0, 4, 6, 8, 9], np.int32), np.array([3, 1, 2, 1, 2, 0, 0, 1, 0], np.int32))
    assert tri.tolist() == [1, 1, 1, 0] and total == 1
    # only self-loops, one vertex, no edges
    tri, total, st = _check(3, np.array([0, 1, 3, 3], np.int32), np.array([0, 1, 1], np.int32))
    assert tri.tolist() == [0, 0, 0] and total == 0 and st["oriented_edges"] == 0
    _check(1, np.array([0, 1], np.int32), np.array([0], np.int32))
    tri, total, _ = _check(1, np.array([0, 0], np.int32), np.array([], np.int32))
    assert tri.tolist() == [0] and total == 0
    tri, total, _ = _check(6, np.zeros(7, np.int32), np.array([], np.int32))
    assert tri.tolist() == [0] * 6 and total == 0
    # one-way edges only
    _check(2, np.array([0, 0, 1], np.int32), np.array([0], np.int32))
    _check(5, np.array([0, 0, 1, 2, 3, 4], np.int32), np.array([0, 1, 2, 3], np.int32))
    # a triangle given by three one-way edges
    for strategy in STRATEGIES:
        tri, total, _ = _check(3, np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32), strategy=strategy)
        assert tri.tolist() == [1, 1, 1] and total == 1


def test_complete_graphs_beyond_32_bits():
    n = 3000
    ro, ci = complete(n)
    p = ga.TcProblem().init(n, ro, ci)
    tri, total, st = _run(p)
    coeff, trans = p.clustering()
    p.close()
    assert total == 4_495_501_000 and total > 1 << 32
    assert np.array_equal(tri, np.full(n, 4_495_501, np.int64))
    assert (coeff == 1.0).all() and trans == 1.0
    assert st["max_out_row"] == n - 1
    _bound(st)
    n = 2048
    ro, ci = complete(n)
    p = ga.TcProblem().init(n, ro, ci)
    for strategy in STRATEGIES:
        for lds in (8192, 100):
            tri, total, st = _run(p, strategy=strategy, lds_entries=lds)
            assert total == n * (n - 1) * (n - 2) // 6
            assert np.array_equal(tri, np.full(n, (n - 1) * (n - 2) // 2, np.int64)), (strategy, lds)
            print("K_%d strategy %d lds_entries %d: %s" % (n, strategy, lds, st))
    p.close()


def _strategies_agree(p, label):
    """every strategy, and a tiny staging budget, byte for byte; the automatic run uses more than one regime"""
    auto, total, st = _run(p, strategy=ga.TC_AUTO, lds_entries=4096, lane_max_row=32)
    print("%s auto: total %d %s" % (label, total, st))
    assert sum(1 for k in ("lane_rows", "lds_rows", "global_rows") if st[k] > 0) > 1, st
    assert st["entries_probed"] > 0 and st["kernel_launches"] >= 3
    _bound(st)
    for options in ({"strategy": ga.TC_LANE}, {"strategy": ga.TC_LDS}, {"strategy": ga.TC_GLOBAL}, {"strategy": ga.TC_LDS, "lds_entries": 3},
                    {"strategy": ga.TC_AUTO, "lds_entries": 40}, {"strategy": ga.TC_AUTO, "lds_entries": 8, "lane_max_row": 4},
                    {"strategy": ga.TC_AUTO, "lds_entries": 8192, "lane_max_row": 0}):
        tri, other_total, other = _run(p, **options)
        assert tri.tobytes() == auto.tobytes() and other_total == total, options
        if options.get("lds_entries", 4096) < st["max_out_row"] and options["strategy"] != ga.TC_LANE:
            assert other["global_rows"] > 0, (options, other)  # the path beyond the LDS budget ran
    return auto, total


def test_every_strategy_on_rmat16():
    g = o.rmat_seeded(16, 8 << 16)
    p = ga.TcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    auto, total = _strategies_agree(p, "rmat16")
    p.close()
    assert total == 2947873
    assert np.array_equal(auto, oriented(g.nodes, g.row_offsets, g.col_indices)[0])


def test_every_strategy_on_hub_and_cliques():
    n, ro, ci = hub_and_cliques()
    p = ga.TcProblem(instrument=True).init(n, ro, ci)
    auto, total = _strategies_agree(p, "hub and cliques")
    assert p.stats()["kernel_ms"] > 0
    p.close()
    ref, ref_total, _, _, _ = oriented(n, ro, ci)
    assert np.array_equal(auto, ref) and total == ref_total


def test_rejects_bad_input():
    with pytest.raises(RuntimeError, match="code -1"):
        ga.TcProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.TcProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a decreasing offset
        ga.TcProblem().init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not end at `edges` (nothing else wrong)
        ga.TcProblem().init(2, np.array([0, 1, 1], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not start at 0 (nothing else wrong)
        ga.TcProblem().init(2, np.array([1, 1, 1], np.int32), np.array([1], np.int32))
    p = ga.TcProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        p.init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError):  # nothing to run on
        p.enact()
    p.close()
    p = ga.TcProblem()
    for call in (p.reset, p.enact, p.extract, p.clustering):  # before Init: an error code, nothing touched
        with pytest.raises(RuntimeError, match="failed"):
            call()
    assert p.set_option("no_such_option", 1) == 1
    assert p.set_option("strategy", 2) == 0 and p.set_option("strategy", 0) == 0
    with pytest.raises(RuntimeError, match="code -1"):  # not a strategy
        p.set_option("strategy", 4)
    with pytest.raises(RuntimeError, match="code -1"):
        p.set_option("lds_entries", 0)
    p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    p.close()


def test_reset_and_enact_twice_and_one_shots():
    g = o.rmat_seeded(14, 8 << 14)
    p = ga.TcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    a, total_a, _ = _run(p)
    b, total_b, _ = _run(p)
    assert a.tobytes() == b.tobytes() and total_a == total_b
    p.enact()  # without Reset the counts add up: Reset is what zeroes them
    c, total_c = p.extract()
    assert np.array_equal(c, 2 * a) and total_c == 2 * total_a
    d, total_d, _ = _run(p)
    assert d.tobytes() == a.tobytes() and total_d == total_a
    coeff, trans = p.clustering()
    p.close()
    tri, total = ga.gunrock_tc(g.nodes, g.row_offsets, g.col_indices)
    assert np.array_equal(tri, a) and total == total_a
    coeff2, trans2 = ga.gunrock_clustering(g.nodes, g.row_offsets, g.col_indices)
    assert coeff2.tobytes() == coeff.tobytes() and trans2 == trans


def test_clustering_is_bit_equal_to_numpy(golden_dir):
    # d < 2 vertices (chesapeake has none; the R-MAT graph has isolated and degree-1 vertices) and the edgeless graph
    g = o.rmat_seeded(12, 8 << 12)
    p = ga.TcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    tri, total, _ = _run(p)
    coeff, trans = p.clustering()
    p.close()
    d = np.diff(g.row_offsets).astype(np.int64)  # (the oracle's mirrored graph is simple: a row is the neighbourhood)
    assert (d < 2).any()
    want = np.where(d >= 2, 2.0 * tri.astype(np.float64) / np.maximum(d * (d - 1), 1).astype(np.float64), 0.0)
    assert coeff.tobytes() == want.astype(np.float64).tobytes()
    assert trans == np.float64(3 * total) / np.float64((d * (d - 1) // 2).sum())
    assert not coeff[d < 2].any() and 0.0 < trans < 1.0
    p = ga.TcProblem().init(5, np.zeros(6, np.int32), np.array([], np.int32))
    p.reset()
    p.enact()
    coeff, trans = p.clustering()
    p.close()
    assert coeff.tolist() == [0.0] * 5 and trans == 0.0


def test_init_device_and_device_results():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(16)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.TcProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    tri, total, st = _run(p)
    d_tri, d_deg = p.device_results()
    on_device = devgraph.as_tensor(d_tri, n, "<i8").cpu().numpy()
    degrees = devgraph.as_tensor(d_deg, n, "<i4").cpu().numpy()
    p.close()
    h_ro, h_ci = ro.cpu().numpy(), ci.cpu().numpy()
    ref, ref_total, d, longest, _ = oriented(n, h_ro, h_ci)
    assert on_device.dtype == np.int64 and np.array_equal(on_device, tri) and np.array_equal(tri, ref) and total == ref_total == 2947873
    assert np.array_equal(degrees.astype(np.int64), d) and st["max_out_row"] == longest == 129


def test_device_rmat22_invariants():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(22)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.TcProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    tri, total, st = _run(p)
    print("rmat22 auto: total %d %s" % (total, st))
    for options in ({"strategy": ga.TC_LANE}, {"strategy": ga.TC_LDS}, {"strategy": ga.TC_GLOBAL}, {"strategy": ga.TC_AUTO, "lds_entries": 64}):
        other, other_total, other_st = _run(p, **options)
        assert other.tobytes() == tri.tobytes() and other_total == total, options  # (this is what checks the largest-degree vertex)
        print("rmat22 %s: %s" % (options, other_st))
    d_tri, d_deg = p.device_results()
    d = devgraph.as_tensor(d_deg, n, "<i4").cpu().numpy().astype(np.int64)
    p.close()
    _bound(st)
    h_ro, h_ci = ro.cpu().numpy().astype(np.int64), ci.cpu().numpy().astype(np.int64)
    del ro, ci
    # the device-built mirrored graph is simple (Csr::FromCoo drops self-loops and duplicates): a row is the neighbourhood
    assert np.array_equal(d, np.diff(h_ro)) and st["oriented_edges"] * 2 == m
    assert total > 0 and int(tri.sum()) == 3 * total
    assert (tri >= 0).all() and (tri <= d * (d - 1) // 2).all() and not tri[d < 2].any()
    eligible = np.flatnonzero((d >= 2) & (d <= 4096))  # (the cap only bounds host time)
    sample = np.random.default_rng(22).choice(eligible, 256, replace=False)
    mark = np.zeros(n, dtype=bool)
    for v in sample:
        assert local_count(h_ro, h_ci, int(v), mark) == tri[v], "vertex %d of degree %d" % (v, d[v])
