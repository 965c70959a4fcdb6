"""The BCC checker (tests/_bcc_checker.py) on the CPU: its three forms (the Tarjan-Vishkin rules over a breadth-first and over a
non-BFS spanning forest, the depth-first search with an edge stack, networkx) agree on the goldens read directed and undirected, on
the generators, on seeded random graphs and on R-MAT, and reproduce the literals that tests/test_bcc_gpu.py pins; `planted` returns
its planted answer; the header declares grx_bcc_* and capi binds them (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from oracle import gr_oracle as o

import _bcc_checker as k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, M, blocks, bridges, articulation points, largest block, its id, 2-edge-connected components, the largest, sum of bcc, sum of
# tecc), keyed by (file, read undirected): the simple undirected graph is the same either way
LITERALS = {
    ("bips98_606.mtx", False): (7135, 15190, 895, 802, 841, 13746, 0, 1344, 5792, 3290072, 2055001),
    ("bips98_606.mtx", True): (7135, 15190, 895, 802, 841, 13746, 0, 1344, 5792, 3290072, 2055001),
    ("chesapeake.mtx", False): (39, 170, 1, 0, 0, 170, 0, 1, 39, 0, 0),
    ("chesapeake.mtx", True): (39, 170, 1, 0, 0, 170, 0, 1, 39, 0, 0),
    ("test_bc.mtx", False): (7, 13, 1, 0, 0, 13, 0, 1, 7, 0, 0),
    ("test_bc.mtx", True): (7, 13, 1, 0, 0, 13, 0, 1, 7, 0, 0),
    ("test_cc.mtx", False): (11, 18, 2, 0, 0, 13, 0, 2, 7, 65, 28),
    ("test_cc.mtx", True): (11, 18, 2, 0, 0, 13, 0, 2, 7, 65, 28),
    ("test_pr.mtx", False): (4, 6, 1, 0, 0, 6, 0, 1, 4, 0, 0),
    ("test_pr.mtx", True): (4, 6, 1, 0, 0, 6, 0, 1, 4, 0, 0),
}
RMAT = {12: (4096, 27791, 590, 589, 332, 27202, 0, 1571, 2526, 9859816, 4102745),
        16: (65536, 490084, 9751, 9750, 4567, 480334, 0, 32145, 33392, 2889159670, 1258234369)}


def _all(graph, networkx=True):
    nodes, ro, ci = graph
    a, b = k.simple_edges(nodes, ro, ci)
    assert a.dtype == np.int32 and (a < b).all() and (np.diff(a.astype(np.int64) * max(nodes, 1) + b) > 0).all()
    res = k.hopcroft_tarjan(nodes, a, b)
    assert res["bcc"].dtype == res["tecc"].dtype == np.int32 and res["bridge"].dtype == res["articulation"].dtype == np.uint8
    assert k.same(res, k.tarjan_vishkin(nodes, a, b, bfs=True)), "the rules over a breadth-first forest differ"
    assert k.same(res, k.tarjan_vishkin(nodes, a, b, bfs=False)), "the rules over a non-BFS forest differ"
    if networkx:
        assert k.same(res, k.by_networkx(nodes, a, b)), "networkx differs"
    bcc, tecc = res["bcc"], res["tecc"]
    M = a.shape[0]
    assert (bcc <= np.arange(M)).all() and (bcc[bcc] == bcc).all() and (tecc <= np.arange(nodes)).all() and (tecc[tecc] == tecc).all()
    cut = res["bridge"] != 0
    assert (tecc[a[~cut]] == tecc[b[~cut]]).all() and (tecc[a[cut]] != tecc[b[cut]]).all()
    v, ids = k.block_cut(a, b, res)
    assert v.dtype == ids.dtype == np.int32 and set(v.tolist()) == set(np.flatnonzero(res["articulation"]).tolist())
    return a, b, res


@pytest.mark.parametrize("name,undirected", sorted(LITERALS))
def test_forms_agree_on_goldens(golden_dir, name, undirected):
    g = o.build_market(os.path.join(golden_dir, name), undirected=undirected)
    a, _, res = _all((g.nodes, g.row_offsets, g.col_indices))
    assert k.literal(g.nodes, a, res) == LITERALS[(name, undirected)]


@pytest.mark.parametrize("scale", [12, 16])
def test_forms_agree_on_rmat(scale):
    g = o.rmat_seeded(scale, 8 << scale)
    a, _, res = _all((g.nodes, g.row_offsets, g.col_indices), networkx=scale == 12)  # (networkx takes 17 s at scale 16)
    assert k.literal(g.nodes, a, res) == RMAT[scale]


def test_closed_forms():
    for n in (1, 2, 3, 64, 65):
        a, _, res = _all(k.path(n))
        assert res["bridge"].all() and np.array_equal(res["tecc"], np.arange(n)) and int(res["articulation"].sum()) == max(n - 2, 0)
        assert np.array_equal(res["bcc"], np.arange(n - 1))
    for n in (3, 64, 65):
        _, _, res = _all(k.cycle(n))
        assert not res["bcc"].any() and not res["bridge"].any() and not res["articulation"].any() and not res["tecc"].any()
        _, _, res = _all(k.complete(n))
        assert not res["bcc"].any() and not res["articulation"].any() and not res["tecc"].any()
    for leaves in (1, 2, 63, 64, 65):
        _, _, res = _all(k.star(leaves))
        assert res["bridge"].all() and res["articulation"].tolist() == [int(leaves > 1)] + [0] * leaves
    for blades in (1, 2, 64, 65):
        for hub in (0, 3 % (2 * blades + 1)):
            perm = np.arange(2 * blades + 1)
            perm[[0, hub]] = perm[[hub, 0]]
            _, _, res = _all(k.relabel(k.windmill(blades), perm))
            want = np.zeros(2 * blades + 1, np.uint8)
            want[hub] = blades > 1
            assert np.array_equal(res["articulation"], want) and k.summary(res)["blocks"] == blades and not res["tecc"].any()
    _, _, res = _all(k.barbell(5, 5))
    assert k.summary(res) == {"blocks": 8, "bridges": 6, "articulation_points": 7, "largest_block": 10, "largest_block_id": 0,
                              "tecc_components": 7, "largest_tecc": 5, "largest_tecc_root": 0}
    _, _, res = _all(k.lollipop(5, 4))
    assert k.summary(res)["bridges"] == 4 and k.summary(res)["articulation_points"] == 4
    for graph in (k.ladder(64), k.grid(33, 33), k.grid(1, 9), k.grid(2, 2)):
        _, _, res = _all(graph)
        assert k.summary(res)["blocks"] == (1 if graph[0] != 9 else 8)


def test_cross_trap():
    """one block; the local test `low[w] >= pre[v] and high[w] inside v's subtree` would flag vertex 1 (and its images)"""
    for perm in (np.arange(6), np.array([0, 2, 1, 3, 4, 5]), np.array([5, 4, 3, 2, 1, 0]), np.array([2, 0, 1, 5, 3, 4])):
        _, _, res = _all(k.relabel(k.cross_trap(), perm))
        assert not res["bcc"].any() and not res["articulation"].any() and not res["bridge"].any() and not res["tecc"].any()


def test_raw_csrs():
    i32 = lambda x: np.array(x, np.int32)
    for nodes, ro, ci, M, bridges in ((0, [0], [], 0, 0), (1, [0, 0], [], 0, 0), (1, [0, 1], [0], 0, 0), (5, [0] * 6, [], 0, 0),
                                      (3, [0, 1, 3, 3], [0, 1, 1], 0, 0),             # only self-loops
                                      (2, [0, 2, 3], [1, 1, 0], 1, 1),                # a doubled edge is one edge: a bridge
                                      (4, [0, 3, 4, 6, 7], [3, 1, 2, 0, 3, 1, 2], 5, 0),  # unsorted rows
                                      (3, [0, 2, 2, 2], [2, 1], 2, 2)):               # one-way entries
        a, _, res = _all((nodes, i32(ro), i32(ci)))
        assert a.shape[0] == M and int(res["bridge"].sum()) == bridges and res["tecc"].shape[0] == nodes


def test_random_graphs():
    rng = np.random.default_rng(20261019)
    for case in range(300):
        n = int(rng.integers(1, 60))
        m = int(rng.integers(0, 3 * n))
        graph = k.from_edges(n, rng.integers(0, n, (m, 2)), symmetric=bool(case & 1), shuffle=rng)
        _all(graph, networkx=case < 150)


def test_summary_ties_go_to_the_smaller_id():
    res = {"bcc": np.array([0, 0, 2, 2, 4], np.int32), "bridge": np.array([0, 0, 0, 0, 1], np.uint8), "articulation": np.zeros(6, np.uint8),
           "tecc": np.array([0, 0, 2, 2, 4, 5], np.int32)}
    s = k.summary(res)
    assert (s["largest_block"], s["largest_block_id"], s["largest_tecc"], s["largest_tecc_root"]) == (2, 0, 2, 0)
    assert k.block_sizes(res["bcc"]).tolist() == [2, 2, 2, 2, 1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_returns_its_answer(seed):
    n, ro, ci, a, b, res = k.planted(seed, 2000 + 1000 * seed)
    a2, b2, found = _all((n, ro, ci), networkx=seed == 1)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and k.same(found, res)
    assert res["bridge"].any() and res["articulation"].any() and k.summary(res)["largest_block"] >= 63


def test_header_declares_bcc_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    assert "a doubled edge can still be a bridge" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_bcc_[a-z0-9_]+)\s*\(", text))
    want = {"grx_bcc_create", "grx_bcc_init", "grx_bcc_init_device", "grx_bcc_set_option", "grx_bcc_reset", "grx_bcc_enact", "grx_bcc_stats",
            "grx_bcc_phase_trace", "grx_bcc_edges", "grx_bcc_extract", "grx_bcc_summary", "grx_bcc_block_cut", "grx_bcc_device_results",
            "grx_bcc_destroy"}
    assert want == declared, want ^ declared
    from gunrockinst_amd import capi
    import gunrockinst_amd as ga
    assert declared <= set(capi.exported_symbols()), declared - set(capi.exported_symbols())
    for name in ("BccProblem", "gunrock_bcc", "gunrock_bridges", "gunrock_articulation_points"):
        assert hasattr(ga, name), name
    assert (ga.BCC_AUTO, ga.BCC_ROUNDS, ga.BCC_DEVICE_LOOP) == (0, 1, 2)
    for method in ("init", "init_device", "set_option", "reset", "enact", "stats", "phase_trace", "edges", "extract", "summary", "block_cut",
                   "device_results", "close"):
        assert callable(getattr(ga.BccProblem, method)), method
    legacy = open(os.path.join(ROOT, "include", "gunrock", "gunrock.h")).read()
    assert "grx_bcc" not in legacy and "gunrock_bcc" not in legacy
