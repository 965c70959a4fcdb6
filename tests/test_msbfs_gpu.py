"""Multi-source BFS on the GPU (grx_msbfs_*): depth[source][vertex], the per-source and the per-vertex summaries must equal
tests/_msbfs_checker.py's on every input, int32 / int64 against the same with np.array_equal, under every "direction" (auto, push,
pull, alternate) -- goldens read directed and undirected, the source counts around the batch of 64, the vertex counts and row lengths
around the wave, many-level graphs with tiny frontiers, raw CSRs of every awkward shape, directed graphs with the in-neighbour
lists lent, built, absent and wrongly forced, one handle reset many times, the argument errors, parity with the single-source
engine on R-MAT scale 16, and all-sources closeness down to the bytes of the float64."""
import functools
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _msbfs_checker as mk

pytestmark = pytest.mark.gpu

DIRECTIONS = (ga.MSBFS_AUTO, ga.MSBFS_PUSH, ga.MSBFS_PULL, ga.MSBFS_ALTERNATE)
GOLDENS = [(name, undirected) for name in ("bips98_606.mtx", "chesapeake.mtx", "test_bc.mtx", "test_cc.mtx", "test_pr.mtx") for undirected in (False, True)]


@functools.lru_cache(maxsize=None)
def _rmat(scale, undirected=True):
    g = o.rmat_seeded(scale, 8 << scale, undirected=undirected)
    return g.nodes, g.row_offsets, g.col_indices


def _compare(p, sources, ref, store_depths=True):
    """the handle's results after an enact against the rows of the checker"""
    k = len(sources)
    if store_depths:
        d = p.depths()
        assert d.dtype == np.int32 and d.shape == ref.shape
        assert np.array_equal(d, ref), "depths differ from the checker at (source row, vertex) %s" % np.argwhere(d != ref)[:10].tolist()
    else:
        with pytest.raises(RuntimeError, match="code -4"):
            p.depths()
    reached, dist_sum, ecc = p.source_summary()
    want = mk.source_summary(ref)
    assert reached.shape == dist_sum.shape == ecc.shape == (k,)
    assert (reached.dtype, dist_sum.dtype, ecc.dtype) == (np.int64, np.int64, np.int32)
    assert np.array_equal(reached, want[0]) and np.array_equal(dist_sum, want[1]) and np.array_equal(ecc, want[2])
    reaching, in_dist_sum = p.vertex_summary()
    want_v = mk.vertex_summary(ref)
    assert (reaching.dtype, in_dist_sum.dtype) == (np.int32, np.int64)
    assert np.array_equal(reaching, want_v[0]) and np.array_equal(in_dist_sum, want_v[1]) and int(reaching.max()) <= k
    # a batch runs until a level reaches nothing: its largest eccentricity + 1 levels
    batch, level, kind, frontier, edges, ms = p.level_trace()
    st = p.stats()
    batches = (k + 63) // 64
    assert st["batches"] == batches and st["levels"] == batch.shape[0] == st["push_levels"] + st["pull_levels"]
    assert int((kind == ga.MSBFS_LEVEL_PULL).sum()) == st["pull_levels"] and set(kind.tolist()) <= {0, 1}
    for b in range(batches):
        assert int((batch == b).sum()) == int(want[2][64 * b:64 * b + 64].max()) + 1, "levels of batch %d" % b
        assert level[batch == b].tolist() == list(range(1, int((batch == b).sum()) + 1))
    return st


def _check(nodes, ro, ci, sources, ref=None, directions=DIRECTIONS, store_depths=True, **options):
    """one handle, one run per direction, each against the checker"""
    sources = np.asarray(sources, dtype=np.int32)
    if ref is None:
        ref = mk.depths(nodes, ro, ci, sources)
    p = ga.MsbfsProblem().init(nodes, ro, ci)
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    stats = {}
    for direction in directions:
        assert p.set_option("direction", direction) == 0
        p.reset(sources, store_depths=store_depths)
        p.enact()
        stats[direction] = _compare(p, sources, ref, store_depths)
    p.close()
    return stats


@pytest.mark.parametrize("name,undirected", GOLDENS)
def test_goldens(golden_dir, name, undirected):
    g = o.build_market(os.path.join(golden_dir, name), undirected=undirected)
    n = g.nodes
    if n < 200:
        sources = np.arange(n)
    else:
        sources = np.concatenate([np.arange(130), np.random.default_rng(606).integers(0, n, 64)])
    ref = mk.depths(n, g.row_offsets, g.col_indices, sources)
    _check(n, g.row_offsets, g.col_indices, sources, ref)
    d, reached, dist_sum, ecc = ga.gunrock_msbfs(n, g.row_offsets, g.col_indices, sources)
    want = mk.source_summary(ref)
    assert np.array_equal(d, ref) and np.array_equal(reached, want[0]) and np.array_equal(dist_sum, want[1]) and np.array_equal(ecc, want[2])
    if n < 200:  # every vertex a source: the one-shots that need that
        got_ecc, diameter, radius = ga.gunrock_eccentricity(n, g.row_offsets, g.col_indices)
        assert got_ecc.dtype == np.int32 and np.array_equal(got_ecc, want[2]) and (diameter, radius) == (int(want[2].max()), int(want[2].min()))
        reaching, in_dist_sum = mk.vertex_summary(ref)
        c = ga.gunrock_closeness(n, g.row_offsets, g.col_indices)
        assert c.dtype == np.float64 and c.tobytes() == mk.closeness(n, sources, reaching, in_dist_sum).tobytes()
    some = sources[::3]
    reaching, in_dist_sum = mk.vertex_summary(ref[::3])
    c = ga.gunrock_closeness(n, g.row_offsets, g.col_indices, some, wf_improved=False)
    assert c.tobytes() == mk.closeness(n, some, reaching, in_dist_sum, False).tobytes()


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128, 130])
def test_source_count_boundaries(k):
    n, ro, ci = _rmat(10)
    sources = np.random.default_rng(k).integers(0, n, k)
    sources[k // 2] = sources[0]  # a repeated source, in the same batch or in another
    sources[-1] = sources[0]
    _check(n, ro, ci, sources)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_vertex_count_boundaries(n):
    for make in (mk.path, mk.dicycle, mk.complete):
        nodes, ro, ci = make(n)
        _check(nodes, ro, ci, np.arange(n))
        _check(nodes, ro, ci, np.arange(n)[::-1].repeat(2))


@pytest.mark.parametrize("leaves", [63, 64, 65, 5000])
def test_star(leaves):
    n, ro, ci = mk.star(leaves)
    sources = np.concatenate([[0], np.arange(1, min(leaves, 70) + 1), [leaves]])  # the hub, leaves, the last leaf
    st = _check(n, ro, ci, sources)
    assert st[ga.MSBFS_PULL]["pull_levels"] == st[ga.MSBFS_PULL]["levels"] and st[ga.MSBFS_PUSH]["pull_levels"] == 0


def test_row_length_boundaries():
    """wave_min_row 4: the hub's row (out and in) is one short of it, exactly it, one past it"""
    for leaves in (3, 4, 5):
        n, ro, ci = mk.star(leaves)
        assert ro[1] - ro[0] == leaves
        _check(n, ro, ci, np.arange(n), wave_min_row=4)
    _check(*mk.complete(65), np.arange(65), wave_min_row=4)
    _check(*mk.complete(65), np.arange(65), wave_min_row=65)


def test_many_levels_tiny_frontiers():
    n, ro, ci = mk.path(300)
    st = _check(n, ro, ci, [0, 299, 150])
    assert st[ga.MSBFS_AUTO]["levels"] == 300 and st[ga.MSBFS_ALTERNATE]["pull_levels"] == 150
    n, ro, ci = mk.dipath(300)
    sources = np.array([0, 299, 150], np.int32)
    ref = mk.depths(n, ro, ci, sources)
    assert ref[1].tolist() == [-1] * 299 + [0]
    _check(n, ro, ci, sources, ref)
    reached, dist_sum, ecc = ga.gunrock_msbfs(n, ro, ci, sources)[1:]
    assert (reached[1], dist_sum[1], ecc[1]) == (1, 0, 0) and (reached[0], ecc[0]) == (300, 299)
    n, ro, ci = mk.dicycle(130)
    _check(n, ro, ci, np.arange(130))
    _check(*mk.two_components(70, 60), np.arange(130))


RAW = [
    (1, [0, 1], [0]),                                  # one vertex with a loop
    (1, [0, 0], []),                                   # ... and without
    (6, [0] * 7, []),                                  # no edges
    (3, [0, 1, 3, 3], [0, 1, 1]),                      # only self-loops
    (2, [0, 3, 5], [1, 1, 1, 0, 0]),                   # a two-cycle given with duplicates
    (4, [0, 3, 4, 6, 7], [3, 1, 2, 0, 3, 1, 2]),       # unsorted rows
    (2, [0, 1, 1], [1]),                               # a single one-way edge
    (3, [0, 1, 2, 3], [1, 2, 0]),                      # a three-cycle
]


def test_raw_csrs():
    for n, ro, ci in RAW:
        ro, ci = np.array(ro, np.int32), np.array(ci, np.int32)
        for inverse in (ga.MSBFS_INVERSE_AUTO, ga.MSBFS_INVERSE_BUILD, ga.MSBFS_INVERSE_NONE):
            _check(n, ro, ci, np.arange(n), inverse=inverse)
            _check(n, ro, ci, [n - 1, 0, n - 1], inverse=inverse)


def _run(p, sources, **options):
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    p.reset(sources)
    p.enact()
    return p.depths().copy(), p.source_summary(), p.vertex_summary(), p.stats()


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1] + a[2], b[1] + b[2]))


@pytest.mark.parametrize("graph", ["bowtie", "rmat12"])
def test_directed_graphs_and_the_inverse(graph):
    import torch
    n, ro, ci = mk.bowtie(40, 30, 50) if graph == "bowtie" else _rmat(12, False)
    sources = np.random.default_rng(12).integers(0, n, 100).astype(np.int32)
    ref = mk.depths(n, ro, ci, sources)
    _, iro, ici = mk.from_edges(n, ci, np.repeat(np.arange(n), np.diff(ro)))
    d = [torch.from_numpy(a).cuda() for a in (ro, ci, iro, ici)]
    torch.cuda.synchronize()
    runs = []

    def pulled(st, direction):  # (auto is free to choose)
        return direction == ga.MSBFS_AUTO or (st["pull_levels"] > 0) == (direction != ga.MSBFS_PUSH)

    for direction in DIRECTIONS:
        lent = ga.MsbfsProblem().init_device(n, ci.shape[0], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr())
        runs.append(_run(lent, sources, direction=direction))
        assert runs[-1][3]["build_ms"] == 0 and pulled(runs[-1][3], direction)
        lent.close()
        p = ga.MsbfsProblem().init(n, ro, ci)
        runs.append(_run(p, sources, direction=direction, inverse=ga.MSBFS_INVERSE_BUILD))
        assert runs[-1][3]["build_ms"] > 0 and pulled(runs[-1][3], direction)
        runs.append(_run(p, sources, direction=direction, inverse=ga.MSBFS_INVERSE_AUTO))  # directed: the built transpose again
        assert pulled(runs[-1][3], direction)
        runs.append(_run(p, sources, direction=direction, inverse=ga.MSBFS_INVERSE_NONE))  # absent: every level is a push
        assert runs[-1][3]["pull_levels"] == 0
        # the graph forced to be its own inverse: the symmetry check says it is directed, the reset refuses, nothing has changed
        assert p.set_option("inverse", ga.MSBFS_INVERSE_SELF) == 0
        with pytest.raises(RuntimeError, match="code -5"):
            p.reset(sources)
        assert _same((p.depths(),) + (p.source_summary(), p.vertex_summary()), runs[-1])
        with pytest.raises(RuntimeError, match="code -5"):
            p.reset(sources[:3])
        runs.append(_run(p, sources, direction=direction, inverse=ga.MSBFS_INVERSE_BUILD))
        p.close()
    assert np.array_equal(runs[0][0], ref)
    assert all(_same(r, runs[0]) for r in runs)


def test_inverse_self_on_a_symmetric_graph():
    n, ro, ci = _rmat(10)
    sources = np.arange(0, n, 9)
    ref = mk.depths(n, ro, ci, sources)
    st = _check(n, ro, ci, sources, ref, inverse=ga.MSBFS_INVERSE_SELF)
    assert st[ga.MSBFS_PULL]["build_ms"] == 0 and st[ga.MSBFS_PULL]["pull_levels"] > 0
    st = _check(n, ro, ci, sources, ref, inverse=ga.MSBFS_INVERSE_AUTO)
    assert st[ga.MSBFS_PULL]["build_ms"] == 0 and st[ga.MSBFS_PULL]["pull_levels"] > 0


def test_one_handle_many_resets():
    n, ro, ci = _rmat(10)
    rng = np.random.default_rng(3)
    lists = [rng.integers(0, n, 130), np.array([5]), rng.integers(0, n, 70)]
    p = ga.MsbfsProblem().init(n, ro, ci)
    for direction in DIRECTIONS:
        assert p.set_option("direction", direction) == 0
        for sources in lists:
            p.reset(sources)
            p.enact()
            _compare(p, sources, mk.depths(n, ro, ci, sources))
        p.reset(lists[2], store_depths=False)
        p.enact()
        _compare(p, lists[2], mk.depths(n, ro, ci, lists[2]), store_depths=False)
        assert p.device_results()[0] is None
        p.reset(lists[0])  # on again
        p.enact()
        _compare(p, lists[0], mk.depths(n, ro, ci, lists[0]))
        p.enact()  # an Enact that does not follow a Reset repeats it
        _compare(p, lists[0], mk.depths(n, ro, ci, lists[0]))
    p.close()


def test_reset_without_enact():
    n, ro, ci = _rmat(10)
    sources = np.array([7, 7, 900, 3], np.int32)
    p = ga.MsbfsProblem().init(n, ro, ci)
    p.reset(np.arange(100))
    p.enact()
    p.reset(sources)
    d = p.depths()
    want = np.full((4, n), -1, np.int32)
    want[np.arange(4), sources] = 0
    assert np.array_equal(d, want) and np.array_equal(p.depths(1, 2), want[1:3])
    reached, dist_sum, ecc = p.source_summary()
    assert reached.tolist() == [1] * 4 and dist_sum.tolist() == [0] * 4 and ecc.tolist() == [0] * 4
    reaching, in_dist_sum = p.vertex_summary()
    assert np.array_equal(reaching, np.bincount(sources, minlength=n)) and not in_dist_sum.any()
    p.enact()
    _compare(p, sources, mk.depths(n, ro, ci, sources))
    p.close()


def test_argument_errors():
    n, ro, ci = _rmat(10)
    ref = mk.depths(n, ro, ci, [1, 2])
    p = ga.MsbfsProblem()
    for call in (lambda: p.reset([0]), p.enact, p.depths, p.source_summary, p.vertex_summary):  # before Init: an error code, nothing touched
        with pytest.raises(RuntimeError, match="failed"):
            call()
    assert p.device_results() == (None,) * 6
    assert p.set_option("no_such_option", 1) == 1
    for name, value in (("direction", 4), ("direction", -1), ("inverse", 4), ("inverse", -1), ("alpha", 0), ("beta", -1), ("wave_min_row", 0)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    p.init(n, ro, ci)
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(n, ro, ci)
    for call in (p.enact, p.depths, p.source_summary, p.vertex_summary):  # no sources yet
        with pytest.raises(RuntimeError, match="failed"):
            call()
    p.reset([1, 2])
    p.enact()
    for bad in ([-1], [n], [1, 2, n], [1, -1, 2], []):  # a source outside [0, nodes), no source: -1, and nothing has changed
        with pytest.raises(RuntimeError, match="code -1"):
            p.reset(bad)
        _compare(p, [1, 2], ref)
    for first, count in ((0, 3), (2, 1), (-1, 1), (0, -1)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.depths(first, count)
    assert np.array_equal(p.depths(1, 1), ref[1:])
    p.reset([2, 1])
    p.enact()
    _compare(p, [2, 1], ref[::-1])
    p.close()
    with pytest.raises(RuntimeError, match="code -1"):
        ga.MsbfsProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    q = ga.MsbfsProblem()
    with pytest.raises(RuntimeError, match="code -2"):  # malformed offsets
        q.init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        q.init(n, ro, ci)
    with pytest.raises(RuntimeError, match="failed"):
        q.reset([0])
    q.close()
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.MsbfsProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    fresh = ga.MsbfsProblem().init(n, ro, ci)  # a fresh handle still works
    fresh.reset([1, 2])
    fresh.enact()
    _compare(fresh, [1, 2], ref)
    fresh.close()


def test_parity_with_the_single_source_engine():
    n, ro, ci = _rmat(16)
    sources = np.random.default_rng(16).integers(0, n, 128).astype(np.int32)
    p = ga.MsbfsProblem().init(n, ro, ci)
    p.reset(sources)
    p.enact()
    d = p.depths()
    st = p.stats()
    batch, level, kind, frontier, edges, ms = p.level_trace()
    ecc = p.source_summary()[2]
    print("rmat16, 128 sources, auto: %s; kinds %s" % (st, kind.tolist()))
    assert st["pull_levels"] > 0 and st["push_levels"] > 0  # the dense path has run, and the queue path
    for b in (0, 1):
        assert int((batch == b).sum()) == int(ecc[64 * b:64 * b + 64].max()) + 1
    single = ga.BfsProblem().init(n, ro, ci)
    single.set_inverse_graph()
    for row, s in enumerate(sources.tolist()):
        single.reset(s)
        single.enact(s, traversal_mode=2)
        assert np.array_equal(d[row], single.extract()[0]), "row %d differs from the single-source search from %d" % (row, s)
    single.close()
    g = o.Csr(n, ro, ci)
    for row in range(0, 128, 16):
        assert np.array_equal(d[row], o.bfs(g, int(sources[row]))[0])
    for direction in (ga.MSBFS_PUSH, ga.MSBFS_PULL, ga.MSBFS_ALTERNATE):
        assert p.set_option("direction", direction) == 0
        p.reset(sources)
        p.enact()
        assert p.depths().tobytes() == d.tobytes(), direction
    p.close()


def test_all_sources_closeness(golden_dir):
    c = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    rng = np.random.default_rng(130)
    digraph = mk.from_edges(130, rng.integers(0, 130, 400), rng.integers(0, 130, 400))
    for n, ro, ci in ((c.nodes, c.row_offsets, c.col_indices), digraph):
        sources = np.arange(n)
        ref = mk.depths(n, ro, ci, sources)
        _check(n, ro, ci, sources, ref, store_depths=False)
        reaching, in_dist_sum = mk.vertex_summary(ref)
        for wf_improved in (True, False):
            got = ga.gunrock_closeness(n, ro, ci, wf_improved=wf_improved)
            assert got.dtype == np.float64 and got.tobytes() == mk.closeness(n, sources, reaching, in_dist_sum, wf_improved).tobytes()
