"""Betweenness centrality on the GPU against the oracle's Brandes pass (doubles).

Tolerance: the GPU accumulates float32 with atomicAdd in arbitrary order, the oracle sums doubles in BFS order; the
reference's own check for floats is 5 % relative / 0.05 absolute below 0.01 (test_utils.cuh:360-405).  Used here:
|gpu - ref| <= 1e-3 * |ref| + 1e-3 -- two orders tighter, still far above float32 summation noise on these graphs.
Path counts (sigma) are small integers in float32 here, so they must match exactly."""
import os
import re

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-3, 1e-3


def _close(got, ref):
    return np.all(np.abs(got.astype(np.float64) - ref) <= RTOL * np.abs(ref) + ATOL)


def test_reference_known_answer_all_sources(golden, capfd):
    f = golden["bc_undirected7"]
    ro, ci = np.array(f["row_offsets"], np.int32), np.array(f["col_indices"], np.int32)
    bc, ebc = ga.gunrock_bc(7, ro, ci, src=-1)                      # shared_lib_tests/test_bc.c: src_node = -1, manually
    out = capfd.readouterr().out
    assert "GPU Betweeness Centrality finished in" in out           # bc_app.cu:128 (spelling as in the reference)
    line = "Node_ID [0] : BC[%f]" % bc[0]
    assert re.search(r"Node_ID.*0.*: BC.*0.500000", line)            # CMakeLists.txt:219-221
    ref, _ = o.bc(o.Csr(7, ro, ci), -1)
    assert _close(bc, ref)
    assert ebc.shape == (26,) and not ebc.any()                      # the reference never accumulates edge centralities


def test_unsupported_value_type_prints_reference_message(golden, capfd):
    f = golden["bc_undirected7"]
    ro, ci = np.array(f["row_offsets"], np.int32), np.array(f["col_indices"], np.int32)
    import ctypes as C
    from gunrockinst_amd import capi
    gin, gout, cfg = capi._graph_struct(7, ro, ci), ga.GunrockGraph(), ga.GunrockConfig()
    ga.lib().gunrock_bc_func(C.byref(gout), C.byref(gin), cfg, ga.GunrockDataType(ga.VTXID_INT, ga.SIZET_INT, ga.VALUE_INT))
    assert "Not Yet Support This DataType Combination." in capfd.readouterr().out
    assert not gout.node_values


@pytest.mark.parametrize("src", [0, 3, 6])
def test_single_source_sigma_and_dependencies(golden, src):
    f = golden["fixture7"]                                            # the directed 7-vertex fixture
    g = o.Csr(7, f["row_offsets"], f["col_indices"])
    p = ga.BcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    p.run(src)
    sig, bc = p.extract()
    p.close()
    ref, ref_sig = o.bc(g, src)
    assert np.array_equal(sig.astype(np.float64), ref_sig)
    assert _close(bc, ref)


def test_bips98_606_largest_degree_and_rerun(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "bips98_606.mtx"), undirected=True)
    src, _ = o.highest_degree_node(g)
    p = ga.BcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    ref, ref_sig = o.bc(g, src)
    for _ in range(2):                                                # a second run must not accumulate onto the first
        p.run(src)
        sig, bc = p.extract()
        assert np.array_equal(sig.astype(np.float64), ref_sig)
        assert _close(bc, ref)
    p.close()


def test_all_sources_small_graphs(golden_dir):
    for name in ("test_cc.mtx", "chesapeake.mtx"):
        g = o.build_market(os.path.join(golden_dir, name), undirected=True)
        p = ga.BcProblem().init(g.nodes, g.row_offsets, g.col_indices)
        p.run(-1)
        _, bc = p.extract()
        p.close()
        ref, _ = o.bc(g, -1)
        assert _close(bc, ref)


@pytest.mark.parametrize("scale,ef", [(10, 8), (14, 8)])
def test_rmat_single_source(scale, ef):
    g = o.rmat_seeded(scale, ef << scale)
    src, _ = o.highest_degree_node(g)
    p = ga.BcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    p.run(src)
    sig, bc = p.extract()
    p.close()
    ref, ref_sig = o.bc(g, src)
    # path counts grow fast on R-MAT: compare them relatively (float32 holds 24 bits)
    assert np.all(np.abs(sig.astype(np.float64) - ref_sig) <= 1e-5 * ref_sig)
    assert _close(bc, ref)


def test_edge_cases():
    # single vertex, isolated source, two components
    p = ga.BcProblem().init(1, [0, 0], [])
    p.run(0)
    assert p.extract()[1].tolist() == [0.0]
    p.close()
    g = o.Csr(5, [0, 1, 2, 2, 3, 4], [1, 0, 4, 3])                     # 0-1, 3-4, vertex 2 isolated
    p = ga.BcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    for src in (2, -1):
        p.run(src)
        _, bc = p.extract()
        assert _close(bc, o.bc(g, src)[0])
    p.close()


def test_directed_graphs_with_sinks():
    # Vertices without out-edges are never enqueued, so the deepest RECORDED frontier can still have children: 0 -> 1 -> {2, 3}
    # gives vertex 1 the pairs (0, 2) and (0, 3).  (Found by tools/fuzz_others.py: the backward phase used to skip that level.)
    g = o.Csr(4, [0, 1, 3, 3, 3], [1, 2, 3])
    p = ga.BcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    p.run(0)
    _, bc = p.extract()
    ref, _ = o.bc(g, 0)
    assert ref.tolist() == [0.0, 1.0, 0.0, 0.0]                        # (halved like the reference's drivers)
    assert _close(bc, ref)
    p.close()
    for scale, ef in [(6, 20), (10, 4), (13, 8)]:                      # directed R-MAT: many sinks on every level
        g = o.rmat_seeded(scale, ef << scale, undirected=False)
        deg = np.diff(g.row_offsets)
        p = ga.BcProblem().init(g.nodes, g.row_offsets, g.col_indices)
        for src in [int(np.argmax(deg)), 5, int(np.nonzero(deg > 0)[0][-1])]:
            p.run(src)
            _, bc = p.extract()
            assert _close(bc, o.bc(g, src)[0])
        p.close()


# ---- held to tests/_bc_checker.py: Brandes in float64 with a DERIVED relative error bound per vertex (no absolute term), exact zeros,
# exact path counts below 2^24 -- and, on the families whose answers are dyadic, bit-exact results.  (The comparisons above keep their
# 1e-3 + 1e-3: one edge's contribution on an R-MAT level is often below that, so they cannot see a dropped or doubled one.) ----
import _bc_checker as k  # noqa: E402

TILE = k.advance_tile()  # AdvancePolicy::TILE: edge slots per tile of the advance BCEnactor runs


def _note(family, ratio):
    print("BC error/bound  %-28s %.3f" % (family, ratio))  # (pytest -s shows the figures)


def _run(n, ro, ci, src, **kw):
    p = ga.BcProblem().init(n, ro, ci)
    p.run(src, **kw)
    sig, bc = p.extract()
    p.close()
    return sig, bc


EXACT = {
    # 2999 levels; every vertex has out-edges, so at queue_sizing 1.0 the queue holds exactly `nodes` entries
    "path from 0": lambda: k.path(3000, 0), "path from 1500": lambda: k.path(3000, 1500),
    # the hub sits on level 1 and sums one row that ends on, before and after a wave (64) and a tile boundary
    **{"star %d" % d: (lambda d=d: k.star(d)) for d in (63, 64, 65, TILE - 1, TILE, TILE + 1)},
    "broom": lambda: k.broom(5, TILE + 1),                                           # a long hub row below a chain
    "cycle 1000": lambda: k.cycle(1000), "cycle 1001": lambda: k.cycle(1001),       # two shortest paths meeting; the odd case without
    "tree from root": lambda: k.binary_tree(10, 0), "tree from leaf": lambda: k.binary_tree(10, 2046),
    # all dyadic; sigma = 2^k passes 2^24 at k = 25, and at k = 126 the stored 1 / sigma is the smallest normal float
    **{"diamonds %d" % c: (lambda c=c: k.diamond_chain(c)) for c in (24, 25, 126)},
}


@pytest.mark.parametrize("family", list(EXACT))
def test_exact_families(family):
    n, ro, ci, src, want_sigma, want_bc = EXACT[family]()
    sig, bc = _run(n, ro, ci, src)
    assert np.array_equal(sig, want_sigma), np.flatnonzero(sig != want_sigma)[:8]
    assert np.array_equal(bc, want_bc), np.flatnonzero(bc != want_bc)[:8]


def _hub_in_the_middle(d):
    return k.hub_in_the_middle(d, np.random.default_rng(d))


BOUNDED = {
    "grid 13x13": lambda: k.grid(13, 13) + ([0],),                                   # binomial path counts below 2^24: exact
    "layered 65x6 directed": lambda: k.layered(65, 6, False) + ([0],),              # in-degree 65 crosses a wave; 65^5 > 2^24
    "layered 65x6 mirrored": lambda: k.layered(65, 6, True) + ([0],),
    **{"hub in the middle %d" % d: (lambda d=d: _hub_in_the_middle(d) + ([0],)) for d in (TILE - 1, TILE + 1, 5000)},
}


def _three_sources(g):
    deg = np.diff(g.row_offsets)  # the hub, a median-degree vertex, the last vertex with out-edges
    return [int(np.argmax(deg)), int(np.argsort(deg, kind="stable")[g.nodes // 2]), int(np.flatnonzero(deg)[-1])]


def _rmat(scale, undirected):
    g = o.rmat_seeded(scale, 8 << scale, undirected=undirected)
    return g.nodes, g.row_offsets, g.col_indices, _three_sources(g)


for _scale, _und in ((10, True), (14, True), (13, False)):
    BOUNDED["rmat %d %s" % (_scale, "mirrored" if _und else "directed")] = lambda s=_scale, u=_und: _rmat(s, u)


@pytest.mark.parametrize("family", list(BOUNDED))
def test_bounded_families(family):
    n, ro, ci, sources = BOUNDED[family]()
    p = ga.BcProblem().init(n, ro, ci)
    for src in sources:
        ref = k.brandes(n, ro, ci, src)
        assert (ref.bc > 0).any()
        p.run(src)
        _note("%s src %d" % (family, src), k.assert_bc(*p.extract(), ref))
    p.close()


def test_bips98_606_three_sources(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "bips98_606.mtx"), undirected=True)
    p = ga.BcProblem().init(g.nodes, g.row_offsets, g.col_indices)
    for src in _three_sources(g):
        p.run(src)
        _note("bips98_606 src %d" % src, k.assert_bc(*p.extract(), k.brandes(g.nodes, g.row_offsets, g.col_indices, src)))
    p.close()


ALL_SOURCES = {
    "rmat 8 mirrored": lambda: _rmat(8, True)[:3], "rmat 8 directed": lambda: _rmat(8, False)[:3],
    "grid 16x16": lambda: k.grid(16, 16),
    "two components": lambda: k.two_components(np.random.default_rng(2)),            # + 30 isolated vertices, 300 in all
}


@pytest.mark.parametrize("family", list(ALL_SOURCES))
def test_all_sources(family):
    n, ro, ci = ALL_SOURCES[family]()
    ref = k.brandes_all(n, ro, ci)
    assert (ref.bc > 0).any()
    _note("all sources, " + family, k.assert_bc(*_run(n, ro, ci, -1), ref))  # (the path counts are the last source's)


_cache = {}


def _rmat12():
    if "rmat12" not in _cache:
        n, ro, ci, sources = _rmat(12, True)
        _cache["rmat12"] = (n, ro, ci, sources[1], k.brandes(n, ro, ci, sources[1]))
    return _cache["rmat12"]


def test_init_device_gives_the_same_arrays_as_init():
    import torch
    n, ro, ci, src, ref = _rmat12()
    d_ro, d_ci = torch.from_numpy(ro).cuda(), torch.from_numpy(ci).cuda()
    torch.cuda.synchronize()
    p = ga.BcProblem().init_device(n, int(ci.shape[0]), d_ro.data_ptr(), d_ci.data_ptr())
    p.run(src)
    sig, bc = p.extract()
    p.close()
    _note("init_device rmat 12", k.assert_bc(sig, bc, ref))
    host_sig, host_bc = _run(n, ro, ci, src)
    assert np.array_equal(sig, host_sig)  # (integers; the centralities are float sums in no fixed order: both are inside the bound)
    k.assert_bc(host_sig, host_bc, ref)
    assert np.array_equal(d_ro.cpu().numpy(), ro) and np.array_equal(d_ci.cpu().numpy(), ci)  # the borrowed graph is not written


@pytest.mark.parametrize("max_grid_size", [1, 3])
def test_max_grid_size(max_grid_size):
    n, ro, ci, src, ref = _rmat12()
    _note("max_grid_size %d rmat 12" % max_grid_size, k.assert_bc(*_run(n, ro, ci, src, max_grid_size=max_grid_size), ref))
    n, ro, ci, src, want_sigma, want_bc = k.path(3000, 0)
    sig, bc = _run(n, ro, ci, src, max_grid_size=max_grid_size)
    assert np.array_equal(sig, want_sigma) and np.array_equal(bc, want_bc)


def test_queue_sizing_below_one_is_clamped():
    n, ro, ci, src, want_sigma, want_bc = k.path(3000, 1500)  # fills the queue: any capacity below `nodes` would overflow it
    sig, bc = _run(n, ro, ci, src, queue_sizing=0.1)
    assert np.array_equal(sig, want_sigma) and np.array_equal(bc, want_bc)
    n, ro, ci, src, ref = _rmat12()
    k.assert_bc(*_run(n, ro, ci, src, queue_sizing=0.1), ref)


def test_one_shot_call_against_the_checker():
    n, ro, ci, src, ref = _rmat12()
    bc, ebc = ga.gunrock_bc(n, ro, ci, src=src)
    _note("gunrock_bc rmat 12", k.assert_bc(None, bc, ref))
    assert ebc.shape == (ci.shape[0],) and not ebc.any()  # still never accumulated


def test_one_handle_deep_then_shallow_then_all_sources():
    n, ro, ci = k.path(3000, 0)[:3]
    p = ga.BcProblem().init(n, ro, ci)
    for src in (0, 2999, 1500, 1500, 0):  # 2999 levels, the same from the other end, 1500 levels, and back: nothing may linger
        p.run(src)
        sig, bc = p.extract()
        _, _, _, _, want_sigma, want_bc = k.path(3000, src)
        assert np.array_equal(sig, want_sigma) and np.array_equal(bc, want_bc), src
    sn, sro, sci = k.two_components(np.random.default_rng(2))
    q = ga.BcProblem().init(sn, sro, sci)  # a second handle while the first is alive
    q.run(-1)
    ref = k.brandes_all(sn, sro, sci)
    k.assert_bc(*q.extract(), ref)
    p.run(7)  # and the first handle has not noticed
    sig, bc = p.extract()
    assert np.array_equal(bc, k.path(3000, 7)[5])
    q.run(-1)
    k.assert_bc(*q.extract(), ref)
    p.close()
    q.close()


def test_raw_csr_with_self_loops_and_parallel_entries():
    n, ro, ci = k.messy(np.random.default_rng(5))  # parallel entries are parallel edges, self loops carry nothing (test_bc_cpu.py)
    src = int(np.argmax(np.diff(ro)))
    _note("raw csr src %d" % src, k.assert_bc(*_run(n, ro, ci, src), k.brandes(n, ro, ci, src)))
    _note("raw csr all sources", k.assert_bc(*_run(n, ro, ci, -1), k.brandes_all(n, ro, ci)))
    sig, bc = _run(3, [0, 2, 3, 3], [1, 1, 2], 0)  # 0 => 1 twice, 1 -> 2
    assert sig.tolist() == [1, 2, 2] and bc.tolist() == [0, 0.5, 0]


def test_source_without_out_edges():
    n, ro, ci = k.layered(65, 3, False)  # directed: the last layer has no out-edges
    sig, bc = _run(n, ro, ci, n - 1)
    assert sig.tolist() == [0.0] * (n - 1) + [1.0] and not bc.any()


# ---- path counts are float32: a search whose counts leave it is refused (GRX_BC_OVERFLOW), not answered with 0s or NaNs ----

def test_path_count_overflow_is_reported():
    n, ro, ci = k.diamond_chain(130)[:3]  # 2^130 shortest paths to the far end
    p = ga.BcProblem().init(n, ro, ci)
    for _ in range(2):
        with pytest.raises(ga.BcOverflow, match="code -6"):
            p.run(0)
        assert not p.extract()[1].any()  # bc_values are left cleared
        # the handle stays usable: from the joint after 100 diamonds the largest count is 2^100
        _, _, _, src, want_sigma, want_bc = k.diamond_chain(130, 100)
        p.run(src)
        sig, bc = p.extract()
        assert np.array_equal(sig, want_sigma) and np.array_equal(bc, want_bc)
    with pytest.raises(ga.BcOverflow):  # every vertex in turn: stops at vertex 0
        p.run(-1)
    assert not p.extract()[1].any()
    p.close()
    assert issubclass(ga.BcOverflow, ArithmeticError) and ga.BC_OVERFLOW == -6
    # all sources where a LATER source overflows: what the earlier ones added is cleared too
    n, ro, ci = k.diamond_chain(130, 100)[:3]
    order = np.concatenate([np.arange(150, 153), np.arange(150), np.arange(153, n)])  # renumbered: three vertices of the middle first
    inv = np.empty(n, np.int64)
    inv[order] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(ro))
    n, ro, ci = k.csr_from_edges(n, inv[rows], inv[ci])
    p = ga.BcProblem().init(n, ro, ci)
    p.run(0)
    assert p.extract()[1].any()
    with pytest.raises(ga.BcOverflow):
        p.run(-1)
    assert not p.extract()[1].any()
    p.close()


def test_one_shot_call_reports_overflow_by_returning_nothing(capfd):
    n, ro, ci = k.diamond_chain(130)[:3]
    with pytest.raises(RuntimeError, match="no node_values"):
        ga.gunrock_bc(n, ro, ci, src=0)
    assert "gunrock_bc_func failed (-6)" in capfd.readouterr().err


def test_path_counts_at_the_edge_of_float32():
    """2^126 is the last count whose reciprocal is a normal float: exact (test_exact_families).  2^127 is a float but 1 / 2^127 is
    subnormal: the search must either be refused or be exact -- never silently different.  (The threshold refuses it.)"""
    n, ro, ci, src, want_sigma, want_bc = k.diamond_chain(127)
    p = ga.BcProblem().init(n, ro, ci)
    try:
        p.run(src)
    except ga.BcOverflow:
        assert not p.extract()[1].any()
    else:
        sig, bc = p.extract()
        assert np.array_equal(sig, want_sigma) and np.array_equal(bc, want_bc)
    p.close()
