"""Per-edge triangle support and the k-truss decomposition on the GPU (grx_truss_*): `support` and `truss` must equal the numpy
peel of tests/_truss_checker.py on every input, int32 against int32 with np.array_equal -- goldens read undirected and directed,
raw CSRs of every awkward shape, closed forms that stress one mechanism each (the tie rule, the put-back, a charge nobody makes,
a triangle charged twice, the wave regime), R-MAT, both schedules crossed with the row threshold, limited runs -- and the
device-built scale-20 R-MAT, too slow for the checker inside a test, must satisfy invariants a wrong kernel breaks.

`rounds` is the number of sub-rounds (under both schedules those of the synchronous peel: the scans of levels nobody is at are
not counted), `levels` the number of non-empty levels."""
import functools
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

from _truss_checker import (classes, clique_ladder, clique_with_pendant, complete, complete_bipartite, diamond, grid, hub_and_cliques,
                            members, path, peel, star, vertex_triangles, vertex_truss)

pytestmark = pytest.mark.gpu

SCHEDULES = (ga.TRUSS_AUTO, ga.TRUSS_ROUNDS)
# (n, M, triangles, max support, max truss, sum(truss), distinct truss values, top class: edges, vertices, levels, sub-rounds of the
# synchronous peel): computed on the CPU by the numpy peel, cross-checked by the sequential algorithm and nx.k_truss
LITERALS = {
    "chesapeake.mtx": (39, 170, 194, 10, 5, 682, 4, 43, 12, 4, 12),
    "bips98_606.mtx": (7135, 15190, 10743, 26, 6, 57406, 5, 1817, 626, 5, 11),
    "test_bc.mtx": (7, 13, 7, 2, 3, 39, 1, 13, 7, 1, 3),
    "test_cc.mtx": (11, 18, 9, 2, 3, 54, 1, 18, 11, 1, 3),
    "test_pr.mtx": (4, 6, 4, 2, 4, 24, 1, 6, 4, 1, 1),
}
RMAT = {
    10: (1024, 6283, 23149, 139, 16, 48061, 15, 516, 38, 15, 83),
    12: (4096, 27791, 123380, 286, 23, 233921, 22, 1760, 73, 22, 169),
    14: (16384, 118049, 626628, 645, 37, 1110395, 35, 3695, 102, 35, 273),
    16: (65536, 490084, 2947873, 1330, 60, 4954774, 47, 7062, 137, 47, 494),
}
CLASSES = {
    "chesapeake.mtx": [0, 0, 7, 27, 93, 43],
    "bips98_606.mtx": [0, 0, 3340, 971, 8399, 663, 1817],
}
RMAT16_CLASSES = [0, 0, 99150, 63058, 45116, 34014, 27055, 24104]


def _freeze(res):
    for x in res[:5]:
        x.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    """(nodes, row_offsets, col_indices, the checker's result): computed once, shared, never written"""
    g = o.rmat_seeded(scale, 8 << scale)
    return g.nodes, g.row_offsets, g.col_indices, _freeze(peel(g.nodes, g.row_offsets, g.col_indices))


@functools.lru_cache(maxsize=None)
def _hub():
    n, ro, ci = hub_and_cliques(6, 12, 400)
    return n, ro, ci, _freeze(peel(n, ro, ci))


def _run(p, k_limit=-1, **options):
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    p.reset()
    p.enact(k_limit)
    truss, top = p.extract()
    assert truss.dtype == np.int32
    return truss.copy(), top, p.stats()


def _check(nodes, ro, ci, ref=None, every_k=True, **options):
    """one full run against the checker: edges, support, truss, max_truss, stats, classes, the trace, members(k), vertex_truss"""
    if ref is None:
        ref = peel(nodes, ro, ci)
    a, b, tri, support, want, levels, sub_rounds = ref
    m = a.shape[0]
    p = ga.TrussProblem()
    for key, value in options.items():  # (before Init: the row threshold then holds for the support pass too)
        assert p.set_option(key, value) == 0, key
    p.init(nodes, ro, ci)
    src, dst = p.edges()
    assert src.dtype == dst.dtype == np.int32 and np.array_equal(src, a) and np.array_equal(dst, b)
    sup, total = p.support()  # valid before any Enact
    assert sup.dtype == np.int32 and np.array_equal(sup, support), np.flatnonzero(sup != support)[:10]
    assert total == tri.shape[0]
    truss, top, st = _run(p)
    assert np.array_equal(truss, want), "truss numbers differ from the checker at %s" % np.flatnonzero(truss != want)[:10]
    assert top == (int(want.max()) if m else 0)
    assert (st["simple_edges"], st["triangles"], st["max_support"]) == (m, tri.shape[0], int(support.max()) if m else 0), st
    assert (st["edges_peeled"], st["levels"], st["rounds"]) == (m, levels, sub_rounds), (st, levels, sub_rounds)
    assert p.extract(truss=False) == (None, top)
    cl = p.classes()
    assert cl.dtype == np.int64 and np.array_equal(cl, classes(want))
    k, edges, ms = p.level_trace()
    assert np.array_equal(k, np.unique(want)) and np.array_equal(edges, cl[k]) and (ms >= 0).all()
    for kk in (range(top + 2) if every_k else (0, 2, 3, top, top + 1)):
        mask, ne, nv = p.members(kk)
        ref_mask, ref_ne, ref_nv = members(nodes, want, a, b, kk)
        assert mask.dtype == np.uint8 and np.array_equal(mask, ref_mask) and (ne, nv) == (ref_ne, ref_nv), kk
        assert p.members(kk, mask=False) == (None, ne, nv)
    assert p.members(top + 1)[1:] == (0, 0)
    vt = p.vertex_truss()
    assert vt.dtype == np.int32 and np.array_equal(vt, vertex_truss(nodes, want, a, b))
    p.close()
    return truss, st


def _summary(nodes, ref, truss, st):
    a, b = ref[0], ref[1]
    top = int(truss.max()) if truss.shape[0] else 0
    _, edges, vertices = members(nodes, truss, a, b, top)
    return (int(nodes), st["simple_edges"], st["triangles"], st["max_support"], top, int(truss.sum()), int(np.unique(truss).shape[0]),
            edges, vertices, st["levels"], st["rounds"])


@pytest.mark.parametrize("name", sorted(LITERALS))
def test_goldens_undirected_and_directed(golden_dir, name):
    for und in (True, False):
        g = o.build_market(os.path.join(golden_dir, name), undirected=und)
        ref = peel(g.nodes, g.row_offsets, g.col_indices)
        truss, st = _check(g.nodes, g.row_offsets, g.col_indices, ref=ref)
        assert _summary(g.nodes, ref, truss, st) == LITERALS[name]
        if name in CLASSES:
            assert classes(truss).tolist() == CLASSES[name]
        other, other_st = _check(g.nodes, g.row_offsets, g.col_indices, ref=ref, every_k=False, schedule=ga.TRUSS_ROUNDS, wave_min_row=3)
        assert other.tobytes() == truss.tobytes() and _summary(g.nodes, ref, other, other_st) == LITERALS[name]


@pytest.mark.parametrize("scale", [10, 12, 14])
def test_rmat_against_the_checker(scale):
    n, ro, ci, ref = _rmat(scale)
    truss, st = _check(n, ro, ci, ref=ref, every_k=scale == 10)
    assert _summary(n, ref, truss, st) == RMAT[scale]
    print("rmat%d: %s" % (scale, st))


def test_rmat16_literals():
    # the checker takes seconds at this scale: pinned by literals, and the two schedules byte for byte
    g = o.rmat_seeded(16, 8 << 16)
    want = RMAT[16]
    p = ga.TrussProblem().init(g.nodes, g.row_offsets, g.col_indices)
    results = {}
    for schedule in SCHEDULES:
        truss, top, st = _run(p, schedule=schedule)
        cl = p.classes()
        _, edges, vertices = p.members(top, mask=False)
        got = (g.nodes, st["simple_edges"], st["triangles"], st["max_support"], top, int(truss.sum(dtype=np.int64)),
               int(np.unique(truss).shape[0]), edges, vertices, st["levels"], st["rounds"])
        assert got == want, (schedule, got)
        assert cl[:8].tolist() == RMAT16_CLASSES and int(cl.sum()) == want[1]
        results[schedule] = truss
        print("rmat16 schedule %d: %s" % (schedule, st))
    sup, total = p.support()
    p.close()
    assert results[ga.TRUSS_AUTO].tobytes() == results[ga.TRUSS_ROUNDS].tobytes()
    assert int(sup.sum(dtype=np.int64)) == 3 * total == 3 * want[2] and (results[ga.TRUSS_AUTO] <= sup + 2).all()


def test_raw_csrs():
    # unsorted rows and duplicates: a triangle and a pendant edge
    truss, _ = _check(4, np.array([0, 4, 6, 8, 9], np.int32), np.array([3, 1, 2, 1, 2, 0, 0, 1, 0], np.int32))
    assert truss.tolist() == [3, 3, 2, 3]
    # only self-loops; one vertex with and without a loop; six vertices with no edges: M = 0, every array empty
    for n, ro, ci in ((3, [0, 1, 3, 3], [0, 1, 1]), (1, [0, 1], [0]), (1, [0, 0], []), (6, [0] * 7, [])):
        truss, st = _check(n, np.array(ro, np.int32), np.array(ci, np.int32))
        assert truss.shape == (0,) and (st["simple_edges"], st["levels"], st["rounds"], st["triangles"]) == (0, 0, 0, 0)
        p = ga.TrussProblem().init(n, np.array(ro, np.int32), np.array(ci, np.int32))
        p.enact()
        assert p.extract()[1] == 0 and p.classes().tolist() == [0] and p.vertex_truss().tolist() == [0] * n
        assert p.edges()[0].shape == (0,) and p.support()[0].shape == (0,) and p.members(0)[0].shape == (0,)
        p.close()
    # one-way edges only
    truss, _ = _check(2, np.array([0, 0, 1], np.int32), np.array([0], np.int32))
    assert truss.tolist() == [2]
    truss, _ = _check(5, np.array([0, 0, 1, 2, 3, 4], np.int32), np.array([0, 1, 2, 3], np.int32))
    assert truss.tolist() == [2] * 4
    # a triangle given by three one-way edges
    for schedule in SCHEDULES:
        truss, _ = _check(3, np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32), schedule=schedule)
        assert truss.tolist() == [3, 3, 3]


def test_closed_forms():
    for schedule in SCHEDULES:
        for wave_min_row in (1, 32):
            opts = dict(schedule=schedule, wave_min_row=wave_min_row)
            for n, ro, ci in (grid(5, 7), path(50), star(40), complete_bipartite(5, 6)):  # no triangle anywhere
                truss, st = _check(n, ro, ci, **opts)
                assert (truss == 2).all() and (st["levels"], st["rounds"], st["triangles"]) == (1, 1, 0)
            ro, ci = complete(7)  # all three edges of every triangle in the frontier at once
            truss, st = _check(7, ro, ci, **opts)
            assert (truss == 7).all() and (st["levels"], st["rounds"], st["max_support"]) == (1, 1, 5)
            truss, _ = _check(*diamond(), **opts)  # the tie rule and the put-back
            assert truss.tolist() == [3] * 5
            for q in (4, 5):  # a charge that nobody makes (4), a triangle charged twice (5)
                n, ro, ci = clique_with_pendant(q)
                truss, st = _check(n, ro, ci, **opts)
                assert sorted(truss.tolist()) == [3, 3] + [q] * (q * (q - 1) // 2) and st["levels"] == 2
            n, ro, ci = clique_ladder(9)
            truss, st = _check(n, ro, ci, **opts)
            assert st["simple_edges"] == 127 and classes(truss).tolist() == [0, 0, 8, 3, 6, 10, 15, 21, 28, 36] and st["levels"] == 8


@pytest.mark.parametrize("wave_min_row", [3, 1024])
def test_hub_and_cliques(wave_min_row):
    # a 400-entry row: with the threshold at 3 every intersection of more than two entries goes through the wave regime
    n, ro, ci, ref = _hub()
    for schedule in SCHEDULES:
        truss, st = _check(n, ro, ci, ref=ref, every_k=False, schedule=schedule, wave_min_row=wave_min_row)
        cl = classes(truss)
        assert (n, st["simple_edges"], st["triangles"], int(truss.max()), int(truss.sum())) == (465, 2632, 3217, 13, 12525)
        assert int((truss >= 4).sum()) == 812 and (cl[4], cl[5], cl[13]) == (333, 11, 468)


@pytest.mark.parametrize("which", ["rmat12", "hub"])
def test_every_schedule_and_threshold_agrees(which):
    n, ro, ci, ref = _rmat(12) if which == "rmat12" else _hub()
    want, levels, sub_rounds = ref[4], ref[5], ref[6]
    p = ga.TrussProblem().init(n, ro, ci)
    launches = {}
    for schedule in SCHEDULES:
        for wave_min_row in (1, 3, 16, 1024):
            for loop_max_entries in (8192, 64):
                truss, _, st = _run(p, schedule=schedule, wave_min_row=wave_min_row, loop_max_entries=loop_max_entries)
                assert truss.tobytes() == want.tobytes(), (which, schedule, wave_min_row, loop_max_entries)
                assert (st["edges_peeled"], st["levels"], st["rounds"]) == (want.shape[0], levels, sub_rounds), st
                launches[(schedule, wave_min_row, loop_max_entries)] = (st["kernel_launches"], st["readbacks"])
    p.close()
    print("%s (launches, read-backs): %s" % (which, launches))
    assert launches[(ga.TRUSS_AUTO, 16, 8192)][1] < launches[(ga.TRUSS_ROUNDS, 16, 8192)][1]


def test_limited_runs(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    cases = [(g.nodes, g.row_offsets, g.col_indices, peel(g.nodes, g.row_offsets, g.col_indices)), _rmat(12)]
    for n, ro, ci, ref in cases:
        a, b, want = ref[0], ref[1], ref[4]
        top = int(want.max())
        p = ga.TrussProblem().init(n, ro, ci)
        for K in (2, 3, (top + 2) // 2, top, top + 1):
            for schedule in SCHEDULES:
                truss, got_top, st = _run(p, k_limit=K, schedule=schedule)
                assert np.array_equal(truss, np.minimum(want, K)), (K, schedule)
                assert got_top == min(top, K)
                assert st["edges_peeled"] == int((want < K).sum()), (K, schedule, st)
                assert st["levels"] == int(np.unique(want[want < K]).shape[0]), (K, schedule, st)
            mask, ne, nv = p.members(K)  # of the limited run: min(truss, K) >= K where truss >= K
            full = members(n, want, a, b, K)
            assert np.array_equal(mask, full[0]) and (ne, nv) == full[1:]
            src, dst, kmask, kne, knv = ga.gunrock_ktruss(n, ro, ci, K)
            assert np.array_equal(src, a) and np.array_equal(dst, b) and np.array_equal(kmask, full[0]) and (kne, knv) == full[1:], K
        p.close()
        src, dst, truss, got_top = ga.gunrock_truss(n, ro, ci)
        assert np.array_equal(src, a) and np.array_equal(dst, b) and np.array_equal(truss, want) and got_top == top
        src, dst, sup, total = ga.gunrock_edge_support(n, ro, ci)
        assert np.array_equal(src, a) and np.array_equal(dst, b) and np.array_equal(sup, ref[3]) and total == ref[2].shape[0]


def test_handle_rules_and_lifecycle():
    with pytest.raises(RuntimeError, match="code -1"):
        ga.TrussProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.TrussProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a decreasing offset
        ga.TrussProblem().init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not end at `edges`
        ga.TrussProblem().init(2, np.array([0, 1, 1], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(ValueError):  # a wrong offsets length
        ga.TrussProblem().init(3, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    p = ga.TrussProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        p.init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError):  # nothing to run on
        p.enact()
    p.close()
    p = ga.TrussProblem()
    for call in (p.reset, p.enact, p.extract, p.support, p.classes, p.vertex_truss, lambda: p.members(2)):  # before Init
        with pytest.raises(RuntimeError, match="failed"):
            call()
    assert p.set_option("no_such_option", 1) == 1
    assert p.set_option("schedule", 1) == 0 and p.set_option("schedule", 0) == 0
    for name, value in (("schedule", 2), ("schedule", -1), ("wave_min_row", 0), ("loop_max_entries", -1)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    n, ro, ci, ref = _rmat(12)
    p.init(n, ro, ci)
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(n, ro, ci)
    sup, total = p.support()  # before any Enact
    assert np.array_equal(sup, ref[3]) and total == ref[2].shape[0]
    with pytest.raises(RuntimeError, match="failed"):  # no result yet
        p.extract()
    p.enact()  # without Reset: it makes its own
    first, top_first = p.extract()
    p.enact()  # and again, on the used state
    second, top_second = p.extract()
    a, top_a, _ = _run(p)
    b, top_b, _ = _run(p)
    assert first.tobytes() == second.tobytes() == a.tobytes() == b.tobytes() == ref[4].tobytes()
    assert top_first == top_second == top_a == top_b == int(ref[4].max())
    assert np.array_equal(p.support()[0], ref[3])  # the peel works on a copy
    p.close()


def test_init_device_and_device_results():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(12)
    n, entries = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.TrussProblem().init_device(n, entries, ro.data_ptr(), ci.data_ptr())
    truss, top, st = _run(p)
    m = st["simple_edges"]
    on_device = [devgraph.as_tensor(ptr, m, "<i4").cpu().numpy() for ptr in p.device_results()]
    sup = p.support()[0]
    src, dst = p.edges()
    p.close()
    ref = peel(n, ro.cpu().numpy(), ci.cpu().numpy())
    assert np.array_equal(truss, ref[4]) and np.array_equal(sup, ref[3]) and top == int(ref[4].max())
    for got, want in zip(on_device, (truss, sup, src, dst)):
        assert got.dtype == np.int32 and np.array_equal(got, want)


def test_device_rmat20_invariants():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(20)
    n, entries = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.TrussProblem().init_device(n, entries, ro.data_ptr(), ci.data_ptr())
    truss, top, st = _run(p)
    print("rmat20 auto: max truss %d %s" % (top, st))
    m = st["simple_edges"]
    sup, total = p.support()
    src, dst = p.edges()
    cl = p.classes()
    mask, top_edges, top_vertices = p.members(top)
    other, other_top, other_st = _run(p, schedule=ga.TRUSS_ROUNDS)
    print("rmat20 rounds: %s" % other_st)
    p.close()
    assert other.tobytes() == truss.tobytes() and other_top == top
    assert (other_st["levels"], other_st["rounds"]) == (st["levels"], st["rounds"])
    assert (src < dst).all() and int(sup.sum(dtype=np.int64)) == 3 * total == 3 * st["triangles"]
    t = ga.TcProblem().init_device(n, entries, ro.data_ptr(), ci.data_ptr())
    t.reset()
    t.enact()
    tri, tc_total = t.extract()
    t.close()
    assert tc_total == total and np.array_equal(vertex_triangles(n, sup, src, dst), tri)
    assert (truss >= 2).all() and (truss <= sup + 2).all()
    k = ga.KcoreProblem().init_device(n, entries, ro.data_ptr(), ci.data_ptr())
    k.reset()
    k.enact()
    core, _ = k.extract()
    k.close()
    assert (truss <= np.minimum(core[src], core[dst]) + 1).all()
    assert int(cl.sum()) == m and cl.shape[0] == top + 1 and cl[top] == top_edges and st["levels"] == int((cl > 0).sum())
    # the top class: every edge has at least max_truss - 2 triangles inside the mask (a small subgraph: on the CPU)
    keep = mask.astype(bool)
    sa, sb = src[keep].astype(np.int64), dst[keep].astype(np.int64)
    ids, inv = np.unique(np.concatenate([sa, sb]), return_inverse=True)
    assert ids.shape[0] == top_vertices
    adj = np.zeros((ids.shape[0], ids.shape[0]), dtype=np.int64)
    x, y = inv[:sa.shape[0]], inv[sa.shape[0]:]
    adj[x, y] = adj[y, x] = 1
    inside = (adj @ adj)[x, y]
    assert (inside >= top - 2).all(), int(inside.min())
