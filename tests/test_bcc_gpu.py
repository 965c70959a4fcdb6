"""Biconnected components, articulation points, bridges and 2-edge-connected components on the GPU (grx_bcc_*): every result must
equal tests/_bcc_checker.py's with np.array_equal under all three schedules -- goldens read directed and undirected, raw CSRs of
every awkward shape, closed forms that stress one mechanism each (a path's four chains of levels and the device loop's re-entry, a
star's hub at the lane / wave boundary, the windmill's root and non-root rule, the trap graph that a local articulation test gets
wrong), planted trees of blocks under every schedule and threshold on one handle, R-MAT against the pinned literals -- and the
device-built scale-20 R-MAT must satisfy invariants a wrong kernel breaks."""
import functools
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _bcc_checker as k

pytestmark = pytest.mark.gpu

SCHEDULES = (ga.BCC_AUTO, ga.BCC_ROUNDS, ga.BCC_DEVICE_LOOP)
# computed on the CPU by the checker's three forms (tests/test_bcc_cpu.py): (n, M, blocks, bridges, articulation points, largest
# block, its id, 2-edge-connected components, the largest, sum of bcc, sum of tecc)
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


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    """(nodes, row_offsets, col_indices, a, b, the checker's result): computed once, shared, never written"""
    g = o.rmat_seeded(scale, 8 << scale)
    a, b, ref = k.solve(g.nodes, g.row_offsets, g.col_indices)
    for x in (a, b) + tuple(ref.values()):
        x.setflags(write=False)
    return g.nodes, g.row_offsets, g.col_indices, a, b, ref


def _forest(p, nodes, a, b, st):
    """parent / level: a valid parent one level up (the forest is not unique), roots at level 0, one per tree"""
    from gunrockinst_amd import devgraph
    ptr = p.device_results()
    read = lambda name, count, dtype: devgraph.as_tensor(ptr[name], count).cpu().numpy().astype(dtype, copy=False)
    parent, level = read("parent", nodes, np.int32), read("level", nodes, np.int32)
    assert np.array_equal(read("src", a.shape[0], np.int32), a) and np.array_equal(read("dst", a.shape[0], np.int32), b)
    deg = np.bincount(np.concatenate([a, b]), minlength=nodes)
    roots = parent < 0
    assert (level[roots] == 0).all() and int((roots & (deg > 0)).sum()) == st["trees"] and (roots | (deg > 0)).all()
    kids = np.flatnonzero(~roots)
    assert (level[kids] == level[parent[kids]] + 1).all()
    edges = set(zip(a.tolist(), b.tolist()))
    lo, hi = np.minimum(kids, parent[kids]), np.maximum(kids, parent[kids])
    assert all(e in edges for e in zip(lo.tolist(), hi.tolist())), "a parent that is no neighbour"
    assert st["levels"] == (int(level[deg > 0].max()) + 1 if (deg > 0).any() else 0)


def _run(p, nodes, a, b, ref, **options):
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    p.reset()
    p.enact()
    bad = k.mismatches(p, nodes, a, b, ref)
    assert not bad, "differs from the checker under %s: %s" % (options, bad)
    st = p.stats()
    kind, items, ms = p.phase_trace()
    M = a.shape[0]
    reached = int(np.unique(np.concatenate([a, b])).shape[0])
    assert kind.tolist() == list(range(6)) and (items >= 0).all() and (ms >= 0).all()
    assert items.tolist() == [reached] * 4 + [M, M + nodes] and st["simple_edges"] == M
    assert st["kernel_launches"] > 0 and st["readbacks"] >= 2 and st["build_ms"] >= 0
    assert st["entries_read"] == 4 * 2 * M, "each of the four chains walks every row once"
    return st


def _check(graph, ref=None, schedules=SCHEDULES, forest=True, **options):
    """the graph under every schedule on one handle, everything against the checker"""
    nodes, ro, ci = graph
    a, b, ref = ref if ref is not None else k.solve(nodes, ro, ci)
    p = ga.BccProblem().init(nodes, ro, ci)
    st = None
    for schedule in schedules:
        st = _run(p, nodes, a, b, ref, schedule=schedule, **options)
        if forest:
            _forest(p, nodes, a, b, st)
    p.close()
    return a, b, ref, st


@pytest.mark.parametrize("name,undirected", sorted(LITERALS))
def test_goldens(golden_dir, name, undirected):
    g = o.build_market(os.path.join(golden_dir, name), undirected=undirected)
    graph = (g.nodes, g.row_offsets, g.col_indices)
    a, b, ref, _ = _check(graph)
    assert k.literal(g.nodes, a, ref) == LITERALS[(name, undirected)]
    src, dst, bcc, blocks = ga.gunrock_bcc(*graph)
    assert np.array_equal(src, a) and np.array_equal(dst, b) and np.array_equal(bcc, ref["bcc"]) and blocks == LITERALS[(name, undirected)][2]
    src, dst, mask, bridges = ga.gunrock_bridges(*graph)
    assert np.array_equal(src, a) and np.array_equal(mask, ref["bridge"]) and mask.dtype == np.uint8 and bridges == LITERALS[(name, undirected)][3]
    mask, points = ga.gunrock_articulation_points(*graph)
    assert np.array_equal(mask, ref["articulation"]) and mask.dtype == np.uint8 and points == LITERALS[(name, undirected)][4]


@pytest.mark.parametrize("scale", [12, 16])
def test_rmat(scale):
    n, ro, ci, a, b, ref = _rmat(scale)
    assert k.literal(n, a, ref) == RMAT[scale]
    _, _, _, st = _check((n, ro, ci), (a, b, ref), forest=scale == 12)
    print("rmat%d: %s" % (scale, st))


def test_raw_csrs():
    i32 = lambda x: np.array(x, np.int32)
    for nodes, ro, ci, M, bridges in ((1, [0, 0], [], 0, 0), (1, [0, 1], [0], 0, 0), (5, [0] * 6, [], 0, 0),  # no edge at all
                                      (3, [0, 1, 3, 3], [0, 1, 1], 0, 0),             # only self-loops
                                      (2, [0, 2, 3], [1, 1, 0], 1, 1),                # a doubled edge is one edge: a bridge
                                      (4, [0, 3, 4, 6, 7], [3, 1, 2, 0, 3, 1, 2], 5, 0),  # unsorted rows
                                      (3, [0, 2, 2, 2], [2, 1], 2, 2)):               # an asymmetric input
        a, _, ref, st = _check((nodes, i32(ro), i32(ci)))
        assert a.shape[0] == M == st["simple_edges"] and int(ref["bridge"].sum()) == bridges
        if M == 0:
            assert (st["trees"], st["levels"]) == (0, 0) and np.array_equal(ref["tecc"], np.arange(nodes))


def test_rejected_inputs():
    i32 = lambda x: np.array(x, np.int32)
    with pytest.raises(RuntimeError, match="code -1"):  # nodes = 0
        ga.BccProblem().init(0, i32([0]), i32([]))
    for ro, ci in (([0, 1, 2], [1, 2]),      # a column outside [0, nodes)
                   ([0, 2, 1], [1, 0]),      # a decreasing offset
                   ([0, 1, 1], [1, 0]),      # offsets that do not end at `edges`
                   ([1, 1, 2], [1, 0])):     # offsets that do not start at 0
        with pytest.raises(RuntimeError, match="code -2"):
            ga.BccProblem().init(2, i32(ro), i32(ci))
    p = ga.BccProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        p.init(2, i32([0, 1, 2]), i32([1, -1]))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, i32([0, 1, 2]), i32([1, 0]))
    p.close()
    p = ga.BccProblem().init(2, i32([0, 1, 2]), i32([1, 0]))
    for call in (p.extract, p.summary, p.block_cut):  # before an Enact: an error code, not a crash
        with pytest.raises(RuntimeError):
            call()
    assert p.phase_trace()[0].shape[0] == 0
    assert p.set_option("no_such_option", 1) == 1
    for name, value in (("schedule", 3), ("schedule", -1), ("wave_min_row", 0), ("loop_max_list", -1), ("loop_max_entries", -1)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(2, i32([0, 1, 2]), i32([1, 0]))
    p.enact()  # an Enact without a Reset makes its own
    assert p.summary()["bridges"] == 1
    p.reset()
    with pytest.raises(RuntimeError):  # a Reset forgets the result
        p.extract()
    p.close()


def test_path():
    """every edge a bridge, every inner vertex an articulation point, every vertex its own tecc: four chains of n levels"""
    for n, schedules in ((2, SCHEDULES), (2001, (ga.BCC_ROUNDS,)), (20001, (ga.BCC_AUTO, ga.BCC_DEVICE_LOOP))):
        graph = k.path(n)
        nodes, ro, ci = graph
        a, b = k.simple_edges(nodes, ro, ci)
        ref = {"bcc": np.arange(n - 1, dtype=np.int32), "bridge": np.ones(n - 1, np.uint8),
               "articulation": np.array([0] + [1] * (n - 2) + [0], np.uint8)[:n] if n > 2 else np.zeros(n, np.uint8),
               "tecc": np.arange(n, dtype=np.int32)}
        for schedule in schedules:
            _, _, _, st = _check(graph, (a, b, ref), schedules=(schedule,))
            assert st["levels"] == n and st["trees"] == 1
            if schedule != ga.BCC_ROUNDS and n > 4096:  # the device loop re-enters: more than 4096 steps in each chain
                assert 4 * ((n + 4095) // 4096) <= st["kernel_launches"] < n // 100, st  # (far below the 4 * n levels)
            if schedule == ga.BCC_ROUNDS:
                assert st["kernel_launches"] >= 4 * n


@pytest.mark.parametrize("n", [3, 64, 65, 20001])
def test_cycle(n):
    """n = 20001: 10001 levels, two vertices wide, the last one closed by a non-tree edge; the device loop re-enters in every chain"""
    _, _, ref, st = _check(k.cycle(n))
    assert not ref["bcc"].any() and not ref["bridge"].any() and not ref["articulation"].any() and not ref["tecc"].any()
    assert st["levels"] == n // 2 + 1


@pytest.mark.parametrize("leaves", [63, 64, 65, 4097])
def test_star(leaves):
    """the lane / wave row boundary and a hub with many children in one level, as the root and as a child of the root"""
    for hub in (0, leaves):
        perm = np.arange(leaves + 1)
        perm[[0, hub]] = perm[[hub, 0]]
        for wave_min_row in (16, 64, 65):
            _, _, ref, st = _check(k.relabel(k.star(leaves), perm), wave_min_row=wave_min_row)
            assert ref["bridge"].all() and np.flatnonzero(ref["articulation"]).tolist() == [hub] and st["levels"] == (2 if hub == 0 else 3)


@pytest.mark.parametrize("blades", [1, 64, 65])
def test_windmill(blades):
    """the root's children-labels rule when the hub is vertex 0, the non-root rule when it is not"""
    n = 2 * blades + 1
    for hub in (0, 3 % n, n - 1):
        perm = np.arange(n)
        perm[[0, hub]] = perm[[hub, 0]]
        _, _, ref, _ = _check(k.relabel(k.windmill(blades), perm))
        assert np.flatnonzero(ref["articulation"]).tolist() == ([hub] if blades > 1 else []) and k.summary(ref)["blocks"] == blades


def test_small_closed_forms():
    _, _, ref, _ = _check(k.barbell(5, 5))
    assert k.summary(ref)["bridges"] == 6 and k.summary(ref)["articulation_points"] == 7
    _, _, ref, _ = _check(k.lollipop(5, 4))
    assert k.summary(ref)["bridges"] == 4
    for graph in (k.ladder(64), k.grid(33, 33), k.complete(5), k.complete(65)):
        _, _, ref, st = _check(graph)
        assert k.summary(ref)["blocks"] == 1 and not ref["articulation"].any()
        if graph[0] == 33 * 33:
            assert st["levels"] == 65


def test_cross_trap():
    """one block, nothing fragile: the local articulation test flags vertex 1; also with the trap vertex in other positions"""
    for perm in (np.arange(6), np.array([0, 2, 1, 3, 4, 5]), np.array([5, 4, 3, 2, 1, 0]), np.array([2, 0, 1, 5, 3, 4])):
        _, _, ref, _ = _check(k.relabel(k.cross_trap(), perm))
        assert not ref["bcc"].any() and not ref["articulation"].any() and not ref["bridge"].any() and not ref["tecc"].any()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted(seed):
    """every schedule and row threshold on one handle; Reset / Enact twice gives the same arrays"""
    n, ro, ci, a, b, ref = k.planted(seed, 2000 + 1000 * seed)
    found = k.solve(n, ro, ci)
    assert k.same(found[2], ref), "the checker misses a planted answer"
    p = ga.BccProblem(instrument=seed == 1).init(n, ro, ci)
    for schedule in SCHEDULES:
        for wave_min_row in (1, 16, 1 << 20):
            st = _run(p, n, a, b, ref, schedule=schedule, wave_min_row=wave_min_row)
            assert (st["kernel_ms"] > 0) == (seed == 1)
    first = p.extract()
    st = _run(p, n, a, b, ref)
    again = p.extract()
    assert all(np.array_equal(first[key], again[key]) for key in first)
    _forest(p, n, a, b, st)
    for thresholds in ((0, 0), (1, 1 << 30), (1 << 30, 64)):  # AUTO with every level wide, only single vertices narrow, by entries
        _run(p, n, a, b, ref, schedule=ga.BCC_AUTO, loop_max_list=thresholds[0], loop_max_entries=thresholds[1])
    p.close()


def test_invariants_on_device_built_rmat20():
    """no checker runs here (networkx would take minutes): what a wrong kernel breaks"""
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(20, 8)
    n, m = ro.shape[0] - 1, ci.shape[0]
    p = ga.BccProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    p.reset()
    ms = p.enact()
    a, b = p.edges()
    out, s, st = p.extract(), p.summary(), p.stats()
    print("rmat20: enact %.3f ms %s %s" % (ms, st, s))
    bcc, tecc, size, cut = out["bcc"], out["tecc"], out["block_size"], out["bridge"] != 0
    M = a.shape[0]
    assert M == st["simple_edges"] and (a < b).all()
    assert (bcc <= np.arange(M)).all() and (bcc[bcc] == bcc).all()
    heads = bcc == np.arange(M)
    assert int(size[heads].astype(np.int64).sum()) == M and np.array_equal(size, size[bcc]) and int(heads.sum()) == s["blocks"]
    assert np.array_equal(cut, size == 1) and int(cut.sum()) == s["bridges"] == int((size[heads] == 1).sum())
    assert (tecc[tecc] == tecc).all() and (tecc <= np.arange(n)).all() and int((tecc == np.arange(n)).sum()) == s["tecc_components"]
    assert (tecc[a[~cut]] == tecc[b[~cut]]).all() and (tecc[a[cut]] != tecc[b[cut]]).all()
    assert int(out["articulation"].sum()) == s["articulation_points"]
    v, ids, count = p.block_cut()
    assert count == v.shape[0] and set(np.unique(v).tolist()) == set(np.flatnonzero(out["articulation"]).tolist()) and (bcc[ids] == ids).all()
    p.close()
