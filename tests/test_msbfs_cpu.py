"""The MS-BFS checker (tests/_msbfs_checker.py) on the CPU: its three forms (the frontier-matrix BFS in numpy, scipy, networkx) agree
with each other and with the oracle's single-source BFS row by row on the goldens read directed and undirected, on the generators
and on R-MAT, and reproduce the literals; closeness in the one formula is networkx's; the header declares grx_msbfs_* and capi binds
them (no GPU needed).  On bips98_606 (7135 vertices) every source goes through the numpy form and the oracle, in chunks; scipy and
networkx take seeded samples of the sources there (64 per chunk of 512, and 24): all of them would be 15 s and minutes."""
import os
import re

import numpy as np
import pytest

from oracle import gr_oracle as o

import _msbfs_checker as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, entries, reachable ordered pairs excluding self, sum of all finite distances, largest eccentricity) over all sources, keyed by
# (file, read undirected): computed here by the checker
LITERALS = {
    ("bips98_606.mtx", False): (7135, 27838, 39993104, 762297910, 73),
    ("bips98_606.mtx", True): (7135, 30380, 43474242, 482590034, 33),
    ("chesapeake.mtx", False): (39, 170, 300, 501, 5),
    ("chesapeake.mtx", True): (39, 340, 1482, 2720, 3),
    ("test_bc.mtx", False): (7, 15, 23, 31, 2),
    ("test_bc.mtx", True): (7, 26, 42, 58, 2),
    ("test_cc.mtx", False): (11, 20, 28, 36, 2),
    ("test_cc.mtx", True): (11, 36, 54, 72, 2),
    ("test_pr.mtx", False): (4, 8, 12, 16, 2),
    ("test_pr.mtx", True): (4, 12, 12, 12, 1),
}
RMAT12 = {False: (4096, 29522, 7125167, 22185364, 8), True: (4096, 55582, 9700110, 27774510, 7)}


def _agree(nodes, ro, ci, sources, scipy_rows=None, networkx_rows=None):
    """the numpy form against the oracle on every row, against scipy and networkx on every row or on the rows given"""
    sources = np.asarray(sources)
    d = mk.depths(nodes, ro, ci, sources)
    assert d.dtype == np.int32 and d.shape == (sources.shape[0], nodes)
    g = o.Csr(nodes, ro, ci)
    for row in range(sources.shape[0]):
        assert np.array_equal(d[row], o.bfs(g, int(sources[row]))[0]), "row %d" % row
    rows = np.arange(sources.shape[0]) if scipy_rows is None else np.asarray(scipy_rows)
    assert np.array_equal(d[rows], mk.by_scipy(nodes, ro, ci, sources[rows]))
    rows = np.arange(sources.shape[0]) if networkx_rows is None else np.asarray(networkx_rows)
    assert np.array_equal(d[rows], mk.by_networkx(nodes, ro, ci, sources[rows]))
    return d


@pytest.mark.parametrize("name,undirected", sorted(LITERALS))
def test_forms_agree_on_goldens(golden_dir, name, undirected):
    g = o.build_market(os.path.join(golden_dir, name), undirected=undirected)
    n = g.nodes
    pairs = total = largest = 0
    for first in range(0, n, 512):  # (the literal is summed from the same rows: the numpy form runs once per chunk)
        sources = np.arange(first, min(first + 512, n))
        sample = None if n < 200 else np.random.default_rng(first).choice(sources.shape[0], 64, replace=False)
        d = _agree(n, g.row_offsets, g.col_indices, sources, sample, None if n < 200 else sample[:24 if first == 0 else 0])
        reached, dist_sum, ecc = mk.source_summary(d)
        pairs, total, largest = pairs + int(reached.sum()) - sources.shape[0], total + int(dist_sum.sum()), max(largest, int(ecc.max()))
    assert (n, g.edges, pairs, total, largest) == LITERALS[(name, undirected)]
    if n < 200:
        assert mk.literal(n, g.row_offsets, g.col_indices) == LITERALS[(name, undirected)]


@pytest.mark.parametrize("undirected", [False, True])
def test_forms_agree_on_rmat12(undirected):
    g = o.rmat_seeded(12, 8 << 12, undirected=undirected)
    sources = np.random.default_rng(12).integers(0, g.nodes, 130)
    _agree(g.nodes, g.row_offsets, g.col_indices, sources, None, np.arange(0, 130, 5))
    assert mk.literal(g.nodes, g.row_offsets, g.col_indices) == RMAT12[undirected]


def test_generators_and_closed_forms():
    for n in (1, 2, 3, 64, 65):
        d = _agree(*mk.path(n), np.arange(n))
        assert np.array_equal(d, np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]))
        d = _agree(*mk.dipath(n), np.arange(n))
        assert np.array_equal(d[n - 1], np.where(np.arange(n) == n - 1, 0, -1))  # the far end reaches nobody
        assert mk.source_summary(d)[0].tolist() == list(range(n, 0, -1))
        d = _agree(*mk.cycle(n), np.arange(n))
        assert int(d.max()) == n // 2
        d = _agree(*mk.dicycle(n), np.arange(n))
        assert np.array_equal(d, (np.arange(n)[None, :] - np.arange(n)[:, None]) % n)
        d = _agree(*mk.complete(n), np.arange(n))
        assert np.array_equal(d, 1 - np.eye(n, dtype=np.int32))
    d = _agree(*mk.star(65), np.arange(66))
    assert mk.source_summary(d)[2].tolist() == [1] + [2] * 65
    d = _agree(*mk.two_components(5, 7), np.arange(12))
    assert (d[:5, 5:] == -1).all() and (d[5:, :5] == -1).all() and mk.source_summary(d)[0].tolist() == [5] * 5 + [7] * 7
    n, ro, ci = mk.bowtie(4, 3, 5)
    d = _agree(n, ro, ci, np.arange(n))
    reached, dist_sum, ecc = mk.source_summary(d)
    assert reached.tolist() == [9] * 4 + [8] * 3 + [1] * 5 and ecc[7:].tolist() == [0] * 5
    reaching, in_dist_sum = mk.vertex_summary(d)
    assert reaching.tolist() == [1] * 4 + [7] * 3 + [8] * 5
    assert int(in_dist_sum.sum()) == int(dist_sum.sum())


def test_duplicate_sources_and_summaries():
    n, ro, ci = mk.path(6)
    sources = np.array([0, 5, 0, 3])
    d = _agree(n, ro, ci, sources)
    assert np.array_equal(d[0], d[2])
    reached, dist_sum, ecc = mk.source_summary(d)
    assert reached.dtype == np.int64 and dist_sum.dtype == np.int64 and ecc.dtype == np.int32
    assert reached.tolist() == [6] * 4 and dist_sum.tolist() == [15, 15, 15, 9] and ecc.tolist() == [5, 5, 5, 3]
    reaching, in_dist_sum = mk.vertex_summary(d)
    assert reaching.dtype == np.int32 and in_dist_sum.dtype == np.int64
    assert reaching.tolist() == [4] * 6 and in_dist_sum.tolist() == [8, 8, 8, 8, 10, 12]


def _nx_closeness(nodes, ro, ci, wf_improved):
    import networkx as nx
    g = nx.DiGraph()
    g.add_nodes_from(range(nodes))
    g.add_edges_from(zip(np.repeat(np.arange(nodes), np.diff(ro)).tolist(), np.asarray(ci).tolist()))
    c = nx.closeness_centrality(g, wf_improved=wf_improved)
    return np.array([c[v] for v in range(nodes)])


def test_closeness_is_networkx(golden_dir):
    c = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    rng = np.random.default_rng(130)
    digraph = mk.from_edges(130, rng.integers(0, 130, 400), rng.integers(0, 130, 400))
    bow = mk.bowtie(4, 3, 5)
    for nodes, ro, ci in ((c.nodes, c.row_offsets, c.col_indices), digraph, bow):
        _, _, _, reaching, in_dist_sum = mk.all_sources(nodes, ro, ci)
        for wf_improved in (True, False):
            mine = mk.closeness(nodes, np.arange(nodes), reaching, in_dist_sum, wf_improved)
            assert mine.dtype == np.float64 and np.abs(mine - _nx_closeness(nodes, ro, ci, wf_improved)).max() <= 1e-12


def test_header_declares_msbfs_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_msbfs_[a-z0-9_]+)\s*\(", text))
    want = {"grx_msbfs_create", "grx_msbfs_init", "grx_msbfs_init_device", "grx_msbfs_set_option", "grx_msbfs_reset", "grx_msbfs_enact",
            "grx_msbfs_stats", "grx_msbfs_level_trace", "grx_msbfs_extract_depths", "grx_msbfs_source_summary", "grx_msbfs_vertex_summary",
            "grx_msbfs_device_results", "grx_msbfs_destroy"}
    assert want == declared, want ^ declared
    from gunrockinst_amd import capi
    import gunrockinst_amd as ga
    assert declared <= set(capi.exported_symbols()), declared - set(capi.exported_symbols())
    for name in ("MsbfsProblem", "gunrock_msbfs", "gunrock_closeness", "gunrock_eccentricity"):
        assert hasattr(ga, name), name
    assert (ga.MSBFS_AUTO, ga.MSBFS_PUSH, ga.MSBFS_PULL, ga.MSBFS_ALTERNATE) == (0, 1, 2, 3)
    for method in ("init", "init_device", "set_option", "reset", "enact", "stats", "level_trace", "depths", "source_summary", "vertex_summary",
                   "device_results", "close"):
        assert callable(getattr(ga.MsbfsProblem, method)), method
    # the binding's closeness is the checker's formula, bit for bit
    reaching, in_dist_sum = np.array([3, 1, 2, 0], np.int32), np.array([7, 0, 3, 0], np.int64)
    for wf_improved in (True, False):
        assert ga.closeness_from_sums(4, [0, 1, 2, 3], reaching, in_dist_sum, wf_improved).tobytes() == \
            mk.closeness(4, [0, 1, 2, 3], reaching, in_dist_sum, wf_improved).tobytes()
    legacy = open(os.path.join(ROOT, "include", "gunrock", "gunrock.h")).read()
    assert "grx_msbfs" not in legacy and "gunrock_msbfs" not in legacy
