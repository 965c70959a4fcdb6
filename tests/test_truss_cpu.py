"""The k-truss checker (tests/_truss_checker.py) on the CPU: its forms agree on the goldens, raw CSRs, closed forms and R-MAT and
reproduce the literals, and the header declares grx_truss_* with capi binding them (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from oracle import gr_oracle as o

from _truss_checker import (by_networkx, classes, clique_ladder, clique_with_pendant, complete, complete_bipartite, diamond, grid,
                            hub_and_cliques, members, path, peel, sequential, star, vertex_triangles, vertex_truss)
from _tc_checker import oriented

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, M, triangles, max support, max truss, sum(truss), distinct truss values, top class: edges, vertices, levels, sub-rounds of the
# synchronous peel); the numpy peel and the sequential algorithm agree on them; the same read undirected and directed
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

RAW = [
    (4, [0, 4, 6, 8, 9], [3, 1, 2, 1, 2, 0, 0, 1, 0], [3, 3, 2, 3]),  # unsorted rows and duplicates: a triangle and a pendant
    (3, [0, 1, 3, 3], [0, 1, 1], []),                                 # only self-loops
    (1, [0, 1], [0], []),                                             # one vertex
    (1, [0, 0], [], []),
    (6, [0] * 7, [], []),                                             # no edges
    (5, [0, 0, 1, 2, 3, 4], [0, 1, 2, 3], [2] * 4),                   # one-way edges only: a path
    (3, [0, 1, 2, 3], [1, 2, 0], [3, 3, 3]),                          # a triangle given by three one-way edges
]


def summary(nodes, res):
    a, b, tri, support, truss, levels, sub_rounds = res
    top = int(truss.max()) if truss.shape[0] else 0
    _, edges, vertices = members(nodes, truss, a, b, top)
    return (int(nodes), int(a.shape[0]), int(tri.shape[0]), int(support.max()) if support.shape[0] else 0, top, int(truss.sum()),
            int(np.unique(truss).shape[0]), edges, vertices, levels, sub_rounds)


def _all(nodes, ro, ci, python_loop=True, nx_ks=()):
    res = peel(nodes, ro, ci)
    a, b, tri, support, truss, levels, sub_rounds = res
    m = a.shape[0]
    assert support.dtype == np.int32 and truss.dtype == np.int32
    assert int(support.sum()) == 3 * tri.shape[0] and (truss >= 2).all() and (truss <= support + 2).all()
    assert levels == np.unique(truss).shape[0] and sub_rounds >= levels
    tc_tri, tc_total = oriented(nodes, ro, ci)[:2]
    assert tc_total == tri.shape[0] and np.array_equal(vertex_triangles(nodes, support, a, b), tc_tri)
    if python_loop:
        assert np.array_equal(truss, sequential(nodes, ro, ci))
    counts = by_networkx(nodes, ro, ci, nx_ks)
    if counts is not None:
        for k, edges in counts.items():
            assert edges == int((truss >= k).sum()), k
    cl = classes(truss)
    assert cl.dtype == np.int64 and int(cl.sum()) == m and cl[:2].sum() == 0
    if m:
        assert cl.shape[0] == int(truss.max()) + 1 and cl[-1] > 0
    return res


@pytest.mark.parametrize("name", sorted(LITERALS))
def test_forms_agree_on_goldens(golden_dir, name):
    for und in (True, False):
        g = o.build_market(os.path.join(golden_dir, name), undirected=und)
        res = _all(g.nodes, g.row_offsets, g.col_indices, nx_ks=range(2, LITERALS[name][4] + 2))
        assert summary(g.nodes, res) == LITERALS[name]
        if name in CLASSES:
            assert classes(res[4]).tolist() == CLASSES[name]


@pytest.mark.parametrize("scale", [10, 12])
def test_forms_agree_on_rmat(scale):
    g = o.rmat_seeded(scale, 8 << scale)
    res = _all(g.nodes, g.row_offsets, g.col_indices, nx_ks=(3, 10, 23, 24) if scale == 12 else (3, 16, 17))
    assert summary(g.nodes, res) == RMAT[scale]


@pytest.mark.parametrize("scale", [14, 16])
def test_peel_reproduces_the_large_literals(scale):
    g = o.rmat_seeded(scale, 8 << scale)
    res = _all(g.nodes, g.row_offsets, g.col_indices, python_loop=False)
    assert summary(g.nodes, res) == RMAT[scale]
    if scale == 16:
        assert classes(res[4])[:8].tolist() == RMAT16_CLASSES


def test_forms_agree_on_raw_csrs():
    for n, ro, ci, want in RAW:
        res = _all(n, np.array(ro, np.int32), np.array(ci, np.int32), nx_ks=(2, 3, 4))
        assert res[4].tolist() == want
        if not want:
            assert res[5:] == (0, 0) and classes(res[4]).tolist() == [0]


def test_closed_forms():
    for n, ro, ci in (grid(5, 7), path(50), star(40), complete_bipartite(5, 6)):
        res = _all(n, ro, ci)
        assert (res[4] == 2).all() and (res[3] == 0).all() and res[5:] == (1, 1)
    ro, ci = complete(7)
    res = _all(7, ro, ci)
    assert (res[4] == 7).all() and (res[3] == 5).all() and res[5:] == (1, 1)
    res = _all(*diamond())
    assert res[4].tolist() == [3] * 5 and res[3].tolist() == [2, 1, 1, 1, 1]
    for q in (4, 5):
        n, ro, ci = clique_with_pendant(q)
        res = _all(n, ro, ci)
        a, b, truss = res[0], res[1], res[4]
        assert np.array_equal(truss, np.where(b == q, 3, q)) and res[5] == 2
    n, ro, ci = clique_ladder(9)
    res = _all(n, ro, ci)
    assert res[0].shape[0] == 127 and classes(res[4]).tolist() == [0, 0, 8, 3, 6, 10, 15, 21, 28, 36] and res[5] == 8


def test_hub_and_cliques_shape():
    n, ro, ci = hub_and_cliques(6, 12, 400)
    res = _all(n, ro, ci)
    a, b, tri, support, truss = res[:5]
    assert (n, a.shape[0], tri.shape[0], int(truss.max()), int(truss.sum())) == (465, 2632, 3217, 13, 12525)
    cl = classes(truss)
    assert int((truss >= 4).sum()) == 812 and (cl[4], cl[5], cl[13]) == (333, 11, 468)
    d = np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    assert d[0] >= 400  # the hub's row: every intersection with it walks the other end's


def test_members_and_vertex_truss():
    n, ro, ci = clique_ladder(6)
    a, b, _, _, truss, _, _ = peel(n, ro, ci)
    assert members(n, truss, a, b, 0)[1:] == (a.shape[0], n)
    assert members(n, truss, a, b, 6)[1:] == (15, 6)      # K_6 alone
    assert members(n, truss, a, b, 5)[1:] == (25, 11)     # K_5 and K_6: the bridge between them is in no triangle
    assert members(n, truss, a, b, 7)[1:] == (0, 0)
    assert members(n, truss, a, b, 5)[0].dtype == np.uint8
    vt = vertex_truss(n, truss, a, b)
    assert vt.dtype == np.int32 and vt.tolist() == sum(([j] * j for j in range(2, 7)), [])
    assert vertex_truss(3, np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64)).tolist() == [0, 0, 0]


def test_header_declares_truss_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    assert "no\n * app/truss" in text or "no app/truss" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_truss_[a-z0-9_]+)\s*\(", text))
    want = {"grx_truss_" + x for x in ("create", "init", "init_device", "set_option", "reset", "enact", "stats", "level_trace", "edges",
                                       "support", "extract", "classes", "members", "vertex_truss", "device_results", "destroy")}
    assert want <= declared, want - declared
    from gunrockinst_amd import capi
    import gunrockinst_amd as ga
    assert declared <= set(capi.exported_symbols()), declared - set(capi.exported_symbols())
    for name in ("TrussProblem", "gunrock_truss", "gunrock_edge_support", "gunrock_ktruss"):
        assert hasattr(ga, name), name
    assert (ga.TRUSS_AUTO, ga.TRUSS_ROUNDS) == (0, 1)
    for method in ("init", "init_device", "set_option", "reset", "enact", "stats", "level_trace", "edges", "support", "extract", "classes",
                   "members", "vertex_truss", "device_results", "close"):
        assert callable(getattr(ga.TrussProblem, method)), method
    legacy = open(os.path.join(ROOT, "include", "gunrock", "gunrock.h")).read()
    assert "grx_truss" not in legacy and "gunrock_truss" not in legacy
