"""The triangle-counting checker (tests/_tc_checker.py) on the CPU: its two forms agree on the goldens, raw CSRs and R-MAT,
closed forms hold, and the header declares grx_tc_* with capi binding them (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from oracle import gr_oracle as o

from _tc_checker import by_matrix, clustering, complete, csr_of, hub_and_cliques, local_count, neighbour_csr, oriented, simple_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# computed by both checker forms; the same read undirected and directed
LITERALS = {"chesapeake.mtx": (194, 71), "bips98_606.mtx": (10743, 52), "test_bc.mtx": (7, 5), "test_cc.mtx": (9, 5),
            "test_pr.mtx": (4, 3)}

RAW = [
    (4, [0, 4, 6, 8, 9], [3, 1, 2, 1, 2, 0, 0, 1, 0]),  # unsorted rows and duplicates
    (3, [0, 1, 3, 3], [0, 1, 1]),                       # only self-loops
    (1, [0, 1], [0]),                                   # one vertex
    (1, [0, 0], []),
    (6, [0] * 7, []),                                   # no edges
    (5, [0, 0, 1, 2, 3, 4], [0, 1, 2, 3]),              # one-way edges only
    (3, [0, 1, 2, 3], [1, 2, 0]),                       # a triangle given by three one-way edges
]


def _both(nodes, ro, ci):
    tri, total, d, longest, _ = oriented(nodes, ro, ci)
    assert tri.dtype == np.int64 and int(tri.sum()) == 3 * total
    m = simple_edges(nodes, ro, ci)[0].shape[0]
    assert longest <= int(np.sqrt(2 * m))
    other = by_matrix(nodes, ro, ci)
    if other is not None:
        assert np.array_equal(tri, other[0]) and total == other[1]
    return tri, total, d


@pytest.mark.parametrize("name", sorted(LITERALS))
def test_forms_agree_on_goldens(golden_dir, name):
    for und in (True, False):
        g = o.build_market(os.path.join(golden_dir, name), undirected=und)
        tri, total, _ = _both(g.nodes, g.row_offsets, g.col_indices)
        assert (total, int(tri.max())) == LITERALS[name]


def test_forms_agree_on_raw_csrs():
    expect = [1, 0, 0, 0, 0, 0, 1]
    for (n, ro, ci), want in zip(RAW, expect):
        tri, total, _ = _both(n, np.array(ro, np.int32), np.array(ci, np.int32))
        assert total == want
    tri, total, _ = _both(3, np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32))
    assert tri.tolist() == [1, 1, 1]


def test_forms_agree_on_rmat12():
    for und in (True, False):
        g = o.rmat_seeded(12, 8 << 12, undirected=und)
        tri, total, d = _both(g.nodes, g.row_offsets, g.col_indices)
        assert (total, int(tri.max())) == (123380, 14060)
        assert oriented(g.nodes, g.row_offsets, g.col_indices)[3] == 48
    a, b = simple_edges(g.nodes, g.row_offsets, g.col_indices)
    nro, nci = neighbour_csr(g.nodes, a, b)
    mark = np.zeros(g.nodes, dtype=bool)
    for v in (0, 1, 17, int(np.argmax(tri))):
        assert local_count(nro, nci, v, mark) == tri[v]


def _grid(w, h):
    v = np.arange(w * h).reshape(h, w)
    r = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    c = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return csr_of(w * h, np.concatenate([r, c]), np.concatenate([c, r]))


def test_closed_forms():
    for n in (3, 4, 9, 33):
        ro, ci = complete(n)
        tri, total, d = _both(n, ro, ci)
        assert (tri == (n - 1) * (n - 2) // 2).all() and total == n * (n - 1) * (n - 2) // 6
        coeff, trans = clustering(tri, d, total)
        assert (coeff == 1.0).all() and trans == 1.0
    # K_{a,b}, a star, a path, a grid: no triangle
    a, b = 5, 7
    r, c = np.repeat(np.arange(a), b), a + np.tile(np.arange(b), a)
    for n, (ro, ci) in ((a + b, csr_of(a + b, np.concatenate([r, c]), np.concatenate([c, r]))),
                        (50, csr_of(50, np.zeros(49, np.int64), np.arange(1, 50))),
                        (50, csr_of(50, np.arange(49), np.arange(1, 50))),
                        (12 * 9, _grid(12, 9))):
        tri, total, d = _both(n, ro, ci)
        assert total == 0 and not tri.any()
        coeff, trans = clustering(tri, d, total)
        assert not coeff.any() and trans == 0.0
    # wheels: a hub and a rim cycle of k >= 4 vertices
    for k in (4, 5, 12, 101):
        rim = 1 + np.arange(k)
        r = np.concatenate([np.zeros(k, np.int64), rim])
        c = np.concatenate([rim, 1 + (np.arange(k) + 1) % k])
        ro, ci = csr_of(k + 1, r, c)  # one-way
        tri, total, d = _both(k + 1, ro, ci)
        assert tri[0] == k and (tri[1:] == 2).all() and total == k
        coeff, trans = clustering(tri, d, total)
        assert coeff[0] == 2.0 * k / (k * (k - 1)) and (coeff[1:] == 2.0 * 2 / 6).all()
        assert trans == 3.0 * k / (k * (k - 1) // 2 + 3 * k)


def test_hub_and_cliques_shape():
    n, ro, ci = hub_and_cliques()
    tri, total, d = _both(n, ro, ci)
    assert d[0] >= 6000 and total >= 24 * (40 * 39 * 38 // 6)
    assert oriented(n, ro, ci)[3] >= 33  # beyond the lane regime's default rows: the automatic run uses more than one regime


def test_header_declares_tc_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_tc_[a-z0-9_]+)\s*\(", text))
    want = {"grx_tc_create", "grx_tc_init", "grx_tc_init_device", "grx_tc_reset", "grx_tc_enact", "grx_tc_stats", "grx_tc_extract",
            "grx_tc_clustering", "grx_tc_device_results", "grx_tc_set_option", "grx_tc_destroy"}
    assert want <= declared, want - declared
    from gunrockinst_amd import capi
    import gunrockinst_amd as ga
    assert declared <= set(capi.exported_symbols()), declared - set(capi.exported_symbols())
    for name in ("TcProblem", "gunrock_tc", "gunrock_clustering"):
        assert hasattr(ga, name), name
    for method in ("init", "init_device", "reset", "enact", "extract", "clustering", "stats", "set_option", "close"):
        assert callable(getattr(ga.TcProblem, method)), method
    legacy = open(os.path.join(ROOT, "include", "gunrock", "gunrock.h")).read()
    assert "grx_tc" not in legacy and "gunrock_tc" not in legacy
