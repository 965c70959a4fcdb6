"""The k-core checker (tests/_kcore_checker.py) on the CPU: its forms agree on the goldens, raw CSRs, closed forms and R-MAT and
reproduce the literals, and the header declares grx_kcore_* with capi binding them (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from oracle import gr_oracle as o

from _kcore_checker import (buckets, by_networkx, clique_ladder, complete, complete_bipartite, cycle, grid, hub_and_cliques, ladder_cores,
                            members, path, peel, shells, simple_edges, star)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, simple edges, degeneracy, sum(core), distinct core values, top core: vertices, edges inside); the numpy peel and
# networkx.core_number agree on them; the same read undirected and directed
LITERALS = {
    "chesapeake.mtx": (39, 170, 6, 207, 4, 26, 119),
    "bips98_606.mtx": (7135, 15190, 7, 21418, 7, 18, 65),
    "test_bc.mtx": (7, 13, 3, 21, 1, 7, 13),
    "test_cc.mtx": (11, 18, 3, 29, 2, 7, 13),
    "test_pr.mtx": (4, 6, 3, 12, 1, 4, 6),
}
RMAT = {12: (4096, 27791, 38, 29261, 37, 72, 1734), 16: (65536, 490084, 109, 516212, 74, 661, 53039)}
RMAT_PEEL = {12: (111, 873), 16: (231, 6050)}  # sub-rounds of the synchronous peel, the largest degree

RAW = [
    (4, [0, 4, 6, 8, 9], [3, 1, 2, 1, 2, 0, 0, 1, 0], [2, 2, 2, 1]),  # unsorted rows and duplicates
    (3, [0, 1, 3, 3], [0, 1, 1], [0, 0, 0]),                          # only self-loops
    (1, [0, 1], [0], [0]),                                            # one vertex
    (1, [0, 0], [], [0]),
    (6, [0] * 7, [], [0] * 6),                                        # no edges
    (5, [0, 0, 1, 2, 3, 4], [0, 1, 2, 3], [1] * 5),                   # one-way edges only: a path
    (3, [0, 1, 2, 3], [1, 2, 0], [2, 2, 2]),                          # a triangle given by three one-way edges
]


def summary(nodes, ro, ci, core):
    a, b = simple_edges(nodes, ro, ci)
    top = int(core.max())
    _, vertices, edges = members(core, a, b, top)
    return (int(nodes), int(a.shape[0]), top, int(core.sum()), int(np.unique(core).shape[0]), vertices, edges)


def _all(nodes, ro, ci, python_loop=True):
    core, d, levels, sub_rounds = peel(nodes, ro, ci)
    assert core.dtype == np.int32 and (core <= d).all() and ((core == 0) == (d == 0)).all()
    assert levels == np.unique(core).shape[0] and sub_rounds >= levels
    if python_loop:
        assert np.array_equal(core, buckets(nodes, ro, ci))
    other = by_networkx(nodes, ro, ci)
    if other is not None:
        assert np.array_equal(core, other)
    sh = shells(core)
    assert sh.dtype == np.int64 and int(sh.sum()) == nodes and sh.shape[0] == int(core.max()) + 1 and sh[-1] > 0
    return core, d, levels, sub_rounds


@pytest.mark.parametrize("name", sorted(LITERALS))
def test_forms_agree_on_goldens(golden_dir, name):
    for und in (True, False):
        g = o.build_market(os.path.join(golden_dir, name), undirected=und)
        core, _, _, _ = _all(g.nodes, g.row_offsets, g.col_indices)
        assert summary(g.nodes, g.row_offsets, g.col_indices, core) == LITERALS[name]


@pytest.mark.parametrize("scale", [12, 16])
def test_forms_agree_on_rmat(scale):
    g = o.rmat_seeded(scale, 8 << scale)
    core, d, levels, sub_rounds = _all(g.nodes, g.row_offsets, g.col_indices)
    assert summary(g.nodes, g.row_offsets, g.col_indices, core) == RMAT[scale]
    assert (sub_rounds, int(d.max())) == RMAT_PEEL[scale]
    assert levels == RMAT[scale][4] and (core == 0).any()  # (level 0, the vertices without a neighbour, is one of them)


def test_forms_agree_on_raw_csrs():
    for n, ro, ci, want in RAW:
        core, _, _, _ = _all(n, np.array(ro, np.int32), np.array(ci, np.int32))
        assert core.tolist() == want


def test_closed_forms():
    for n in (2, 3, 9, 65):
        ro, ci = complete(n)
        assert (_all(n, ro, ci)[0] == n - 1).all()
    for (n, ro, ci), want in ((path(51), 1), (cycle(50), 2), (star(40), 1), (grid(9, 12), 2), (complete_bipartite(3, 17), 3),
                              (complete_bipartite(5, 5), 5)):
        core, _, levels, _ = _all(n, ro, ci)
        assert (core == want).all() and levels == 1
    # a path of N vertices leaves from both ends: ceil(N / 2) sub-rounds in its one level
    for n_path in (2, 7, 10, 51):
        n, ro, ci = path(n_path)
        assert peel(n, ro, ci)[3] == (n_path + 1) // 2
    for q in (2, 3, 8, 20):
        n, ro, ci = clique_ladder(q)
        core, _, levels, _ = _all(n, ro, ci)
        assert n == q * (q + 1) // 2 - 1 and np.array_equal(core, ladder_cores(q)) and levels == q - 1
        assert shells(core).tolist() == [0] + list(range(2, q + 1))


def test_hub_and_cliques_shape():
    n, ro, ci = hub_and_cliques()
    core, d, _, _ = _all(n, ro, ci, python_loop=False)
    assert d[0] >= 6000 and int(core.max()) >= 39 and core[0] >= 39  # the hub sits in the cliques' core, far below its degree


def test_members_and_shells():
    n, ro, ci = clique_ladder(6)
    core = peel(n, ro, ci)[0]
    a, b = simple_edges(n, ro, ci)
    assert members(core, a, b, 0)[1:] == (n, a.shape[0])
    assert members(core, a, b, 5)[1:] == (6, 15)      # K_6 alone
    assert members(core, a, b, 4)[1:] == (11, 26)     # K_5, K_6 and the bridge between them
    assert members(core, a, b, 6)[1:] == (0, 0)
    assert members(core, a, b, 5)[0].dtype == np.uint8


def test_header_declares_kcore_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_kcore_[a-z0-9_]+)\s*\(", text))
    want = {"grx_kcore_create", "grx_kcore_init", "grx_kcore_init_device", "grx_kcore_set_option", "grx_kcore_reset", "grx_kcore_enact",
            "grx_kcore_stats", "grx_kcore_level_trace", "grx_kcore_extract", "grx_kcore_shells", "grx_kcore_members",
            "grx_kcore_device_results", "grx_kcore_destroy"}
    assert want <= declared, want - declared
    from gunrockinst_amd import capi
    import gunrockinst_amd as ga
    assert declared <= set(capi.exported_symbols()), declared - set(capi.exported_symbols())
    for name in ("KcoreProblem", "gunrock_kcore", "gunrock_kcore_members"):
        assert hasattr(ga, name), name
    assert (ga.KCORE_AUTO, ga.KCORE_ROUNDS, ga.KCORE_DEVICE_LOOP) == (0, 1, 2)
    for method in ("init", "init_device", "set_option", "reset", "enact", "stats", "level_trace", "extract", "shells", "members",
                   "device_results", "close"):
        assert callable(getattr(ga.KcoreProblem, method)), method
    legacy = open(os.path.join(ROOT, "include", "gunrock", "gunrock.h")).read()
    assert "grx_kcore" not in legacy and "gunrock_kcore" not in legacy
