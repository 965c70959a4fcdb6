"""The k-core decomposition on the GPU (grx_kcore_*): `core` must equal the numpy peel of tests/_kcore_checker.py on every input,
int32 against int32 with np.array_equal -- goldens read undirected and directed, raw CSRs of every awkward shape, closed forms
that stress one mechanism each (a star's hub, a path's chain of sub-rounds, a ladder of levels), R-MAT, every schedule crossed
with the compaction and row thresholds, limited runs -- and the device-built scale-20 R-MAT, too slow for the numpy peel inside a
test, must satisfy invariants a wrong kernel breaks."""
import functools
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

from _kcore_checker import (clique_ladder, complete, complete_bipartite, cycle, grid, hub_and_cliques, ladder_cores, members, path, peel,
                            shells, simple_edges, star)

pytestmark = pytest.mark.gpu

SCHEDULES = (ga.KCORE_AUTO, ga.KCORE_ROUNDS, ga.KCORE_DEVICE_LOOP)
# (n, simple edges, degeneracy, sum(core), distinct core values, top core: vertices, edges inside): computed on the CPU by the numpy
# peel and networkx.core_number; the same read undirected and directed
LITERALS = {
    "chesapeake.mtx": (39, 170, 6, 207, 4, 26, 119),
    "bips98_606.mtx": (7135, 15190, 7, 21418, 7, 18, 65),
    "test_bc.mtx": (7, 13, 3, 21, 1, 7, 13),
    "test_cc.mtx": (11, 18, 3, 29, 2, 7, 13),
    "test_pr.mtx": (4, 6, 3, 12, 1, 4, 6),
}
RMAT = {12: (4096, 27791, 38, 29261, 37, 72, 1734), 16: (65536, 490084, 109, 516212, 74, 661, 53039)}


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    """(nodes, row_offsets, col_indices, the checker's core, degrees): computed once, shared, never written"""
    g = o.rmat_seeded(scale, 8 << scale)
    core, d, _, _ = peel(g.nodes, g.row_offsets, g.col_indices)
    for a in (core, d):
        a.setflags(write=False)
    return g.nodes, g.row_offsets, g.col_indices, core, d


def _run(p, k_limit=-1, **options):
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    p.reset()
    p.enact(k_limit)
    core, degeneracy = p.extract()
    assert core.dtype == np.int32
    return core.copy(), degeneracy, p.stats()


def _positive_levels(core):
    return int(np.unique(core[core > 0]).shape[0])


def _check(nodes, ro, ci, ref=None, every_k=True, **options):
    """one full run against the checker: core numbers, degeneracy, stats, shells, members(k), the trace"""
    if ref is None:
        ref = peel(nodes, ro, ci)[0]
    a, b = simple_edges(nodes, ro, ci)
    p = ga.KcoreProblem().init(nodes, ro, ci)
    core, degeneracy, st = _run(p, **options)
    assert np.array_equal(core, ref), "core numbers differ from the checker at %s" % np.flatnonzero(core != ref)[:10]
    assert degeneracy == int(ref.max())
    assert st["simple_edges"] == a.shape[0] and st["vertices_peeled"] == nodes and st["levels"] == _positive_levels(ref), st
    assert p.extract(core=False) == (None, degeneracy)
    sh = p.shells()
    assert sh.dtype == np.int64 and np.array_equal(sh, shells(ref))
    k, vertices, ms = p.level_trace()
    assert np.array_equal(k, np.unique(ref[ref > 0])) and np.array_equal(vertices, sh[k]) and (ms >= 0).all()
    for kk in (range(degeneracy + 2) if every_k else (0, 1, degeneracy, degeneracy + 1)):
        mask, nv, ne = p.members(kk)
        want = members(ref, a, b, kk)
        assert mask.dtype == np.uint8 and np.array_equal(mask, want[0]) and (nv, ne) == want[1:], kk
        assert p.members(kk, mask=False) == (None, nv, ne)
    assert p.members(degeneracy + 1)[1:] == (0, 0)
    p.close()
    return core, st


def _summary(nodes, ro, ci, core):
    a, b = simple_edges(nodes, ro, ci)
    top = int(core.max())
    _, vertices, edges = members(core, a, b, top)
    return (int(nodes), int(a.shape[0]), top, int(core.sum()), int(np.unique(core).shape[0]), vertices, edges)


@pytest.mark.parametrize("name", sorted(LITERALS))
def test_goldens_undirected_and_directed(golden_dir, name):
    for und in (True, False):
        g = o.build_market(os.path.join(golden_dir, name), undirected=und)
        core, _ = _check(g.nodes, g.row_offsets, g.col_indices)
        assert _summary(g.nodes, g.row_offsets, g.col_indices, core) == LITERALS[name]
        for schedule in SCHEDULES[1:]:
            other, _ = _check(g.nodes, g.row_offsets, g.col_indices, ref=core, every_k=False, schedule=schedule, wave_min_row=3)
            assert other.tobytes() == core.tobytes()


@pytest.mark.parametrize("scale", [12, 16])
def test_rmat_literals(scale):
    n, ro, ci, ref, d = _rmat(scale)
    core, st = _check(n, ro, ci, ref=ref, every_k=scale == 12)
    assert _summary(n, ro, ci, core) == RMAT[scale]
    assert st["levels"] == RMAT[scale][4] - 1 and st["max_degree"] == int(d.max())  # (one of the distinct values is 0)
    print("rmat%d: %s" % (scale, st))


def test_raw_csrs():
    # unsorted rows and duplicates
    core, _ = _check(4, np.array([0, 4, 6, 8, 9], np.int32), np.array([3, 1, 2, 1, 2, 0, 0, 1, 0], np.int32))
    assert core.tolist() == [2, 2, 2, 1]
    # only self-loops
    core, st = _check(3, np.array([0, 1, 3, 3], np.int32), np.array([0, 1, 1], np.int32))
    assert core.tolist() == [0, 0, 0] and st["simple_edges"] == 0 and st["levels"] == 0
    # one vertex with and without a loop, six vertices with no edges
    for n, ro, ci in ((1, [0, 1], [0]), (1, [0, 0], []), (6, [0] * 7, [])):
        core, st = _check(n, np.array(ro, np.int32), np.array(ci, np.int32))
        assert core.tolist() == [0] * n and st["levels"] == 0 and st["rounds"] == 0
    # one-way edges only
    core, _ = _check(2, np.array([0, 0, 1], np.int32), np.array([0], np.int32))
    assert core.tolist() == [1, 1]
    core, _ = _check(5, np.array([0, 0, 1, 2, 3, 4], np.int32), np.array([0, 1, 2, 3], np.int32))
    assert core.tolist() == [1] * 5
    # a triangle given by three one-way edges
    for schedule in SCHEDULES:
        core, _ = _check(3, np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32), schedule=schedule)
        assert core.tolist() == [2, 2, 2]


def _all_equal(nodes, ro, ci, value, **options):
    """a graph whose cores are all `value`: a closed form, no checker run"""
    p = ga.KcoreProblem().init(nodes, ro, ci)
    core, degeneracy, st = _run(p, **options)
    sh = p.shells()
    p.close()
    assert np.array_equal(core, np.full(nodes, value, np.int32)), np.flatnonzero(core != value)[:10]
    assert degeneracy == value and st["levels"] == 1 and st["vertices_peeled"] == nodes
    assert sh.tolist() == [0] * value + [nodes]
    return st


def test_closed_forms():
    for n in (2, 65, 300):
        ro, ci = complete(n)
        _all_equal(n, ro, ci, n - 1)
    _all_equal(*cycle(1000), 2)
    _all_equal(*grid(64, 64), 2)
    _all_equal(*complete_bipartite(3, 500), 3)


def test_star_hub_is_appended_once():
    # the hub receives 99 999 decrements in one sub-round: it reaches the level once and never rests below it
    for schedule in SCHEDULES:
        st = _all_equal(*star(100_000), 1, schedule=schedule)
        assert st["vertices_peeled"] == 100_000 and st["max_degree"] == 99_999


def test_clique_ladder_levels():
    q = 64
    n, ro, ci = clique_ladder(q)
    for schedule in SCHEDULES:
        p = ga.KcoreProblem(instrument=True).init(n, ro, ci)
        core, degeneracy, st = _run(p, schedule=schedule)
        k, vertices, ms = p.level_trace()
        sh = p.shells()
        p.close()
        assert np.array_equal(core, ladder_cores(q)) and degeneracy == q - 1
        assert k.shape[0] == 63 == st["levels"] and (np.diff(k) > 0).all() and np.array_equal(vertices, sh[k])
        assert st["kernel_ms"] > 0


def test_path_runs_in_the_device_loop():
    # 10 001 dependent sub-rounds in one level: a condition on the mechanism, not a timing
    n, ro, ci = path(20_001)
    st_rounds = _all_equal(n, ro, ci, 1, schedule=ga.KCORE_ROUNDS)
    assert st_rounds["rounds"] >= 10_001, st_rounds
    st_auto = _all_equal(n, ro, ci, 1)
    assert st_auto["rounds"] * 10 <= 10_001, st_auto
    st_loop = _all_equal(n, ro, ci, 1, schedule=ga.KCORE_DEVICE_LOOP)
    assert st_loop["rounds"] * 10 <= 10_001, st_loop
    print("path(20001): rounds %s | auto %s | device loop %s" % (st_rounds, st_auto, st_loop))


def _schedule_graphs():
    n, ro, ci, ref, _ = _rmat(16)
    yield "rmat16", n, ro, ci, ref
    n, ro, ci = path(5001)
    yield "path5001", n, ro, ci, np.ones(n, np.int32)
    n, ro, ci = clique_ladder(40)
    yield "ladder40", n, ro, ci, ladder_cores(40)
    n, ro, ci = hub_and_cliques()
    yield "hub_and_cliques", n, ro, ci, peel(n, ro, ci)[0]


@pytest.mark.parametrize("which", range(4))
def test_every_schedule_agrees(which):
    label, n, ro, ci, ref = list(_schedule_graphs())[which]
    p = ga.KcoreProblem().init(n, ro, ci)
    launches = {}
    for schedule in SCHEDULES:
        for compact_below in (0.0, 0.5, 1.0):
            for wave_min_row in (1, 64, 1 << 30):
                core, _, st = _run(p, schedule=schedule, compact_below=compact_below, wave_min_row=wave_min_row)
                assert core.tobytes() == ref.tobytes(), (label, schedule, compact_below, wave_min_row)
                assert st["vertices_peeled"] == n and st["levels"] == _positive_levels(ref)
                if compact_below == 1.0:
                    assert st["compactions"] > 0, (label, schedule, st)
                if compact_below == 0.0:
                    assert st["compactions"] == 0, (label, schedule, st)
                launches[(schedule, compact_below, wave_min_row)] = st["kernel_launches"]
    p.close()
    print("%s kernel launches: %s" % (label, launches))
    if label == "rmat16":
        assert launches[(ga.KCORE_AUTO, 0.5, 64)] < launches[(ga.KCORE_ROUNDS, 0.5, 64)]
        assert launches[(ga.KCORE_AUTO, 0.0, 64)] < launches[(ga.KCORE_ROUNDS, 0.0, 64)]


def test_limited_runs(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    cases = [(g.nodes, g.row_offsets, g.col_indices, peel(g.nodes, g.row_offsets, g.col_indices)[0])]
    cases.append(_rmat(12)[:4])
    for n, ro, ci, ref in cases:
        a, b = simple_edges(n, ro, ci)
        degeneracy = int(ref.max())
        p = ga.KcoreProblem().init(n, ro, ci)
        for K in (0, 1, 2, 5, degeneracy, degeneracy + 3):
            for schedule in SCHEDULES:
                core, top, st = _run(p, k_limit=K, schedule=schedule)
                assert np.array_equal(core, np.minimum(ref, K)), (K, schedule)
                assert top == min(degeneracy, K)
                assert st["levels"] <= int(np.unique(ref[(ref > 0) & (ref < K)]).shape[0]), (K, schedule, st)
            mask, nv, ne = p.members(K)  # of the limited run: min(core, K) >= K where core >= K
            assert np.array_equal(mask, members(ref, a, b, K)[0])
            got = ga.gunrock_kcore_members(n, ro, ci, K)
            want = members(ref, a, b, K)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] == (nv, ne), K
        p.close()
        core, top = ga.gunrock_kcore(n, ro, ci)
        assert np.array_equal(core, ref) and top == degeneracy


def test_handle_rules():
    with pytest.raises(RuntimeError, match="code -1"):
        ga.KcoreProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.KcoreProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a decreasing offset
        ga.KcoreProblem().init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not end at `edges` (nothing else wrong)
        ga.KcoreProblem().init(2, np.array([0, 1, 1], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(ValueError):  # a wrong offsets length
        ga.KcoreProblem().init(3, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    p = ga.KcoreProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        p.init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError):  # nothing to run on
        p.enact()
    p.close()
    p = ga.KcoreProblem()
    for call in (p.reset, p.enact, p.extract, p.shells, lambda: p.members(1)):  # before Init: an error code, nothing touched
        with pytest.raises(RuntimeError, match="failed"):
            call()
    assert p.set_option("no_such_option", 1) == 1
    assert p.set_option("schedule", 2) == 0 and p.set_option("schedule", 0) == 0
    for name, value in (("schedule", 3), ("schedule", -1), ("compact_below", 1.5), ("compact_below", -0.1), ("wave_min_row", 0)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    n, ro, ci, ref, _ = _rmat(12)
    p.init(n, ro, ci)
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(n, ro, ci)
    a, top_a, _ = _run(p)
    b, top_b, _ = _run(p)
    assert a.tobytes() == b.tobytes() == ref.tobytes() and top_a == top_b
    assert p.extract(core=False) == (None, top_a)
    p.close()


def test_init_device_and_device_results():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(16)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.KcoreProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    core, degeneracy, st = _run(p)
    d_core, d_deg = p.device_results()
    on_device = devgraph.as_tensor(d_core, n, "<i4").cpu().numpy()
    degrees = devgraph.as_tensor(d_deg, n, "<i4").cpu().numpy()
    p.close()
    h_ro, h_ci = ro.cpu().numpy(), ci.cpu().numpy()
    _, o_ro, o_ci, ref, d = _rmat(16)
    if not (np.array_equal(h_ro, o_ro) and np.array_equal(h_ci, o_ci)):  # (the device build gives the oracle's CSR: the shared peel serves)
        ref, d, _, _ = peel(n, h_ro, h_ci)
    assert on_device.dtype == np.int32 and np.array_equal(on_device, core) and np.array_equal(core, ref) and degeneracy == 109
    assert np.array_equal(degrees.astype(np.int64), d)


def test_device_rmat20_invariants():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(20)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.KcoreProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    core, degeneracy, st = _run(p)
    print("rmat20 auto: degeneracy %d %s" % (degeneracy, st))
    sh = p.shells()
    counts = [p.members(k, mask=False)[1:] for k in range(degeneracy + 2)]
    _, d_deg = p.device_results()
    d = devgraph.as_tensor(d_deg, n, "<i4").cpu().numpy().astype(np.int64)
    other, other_top, other_st = _run(p, schedule=ga.KCORE_ROUNDS)
    print("rmat20 rounds: %s" % other_st)
    p.close()
    assert other.tobytes() == core.tobytes() and other_top == degeneracy
    assert ((core >= 0) & (core <= d)).all() and ((core == 0) == (d == 0)).all()
    assert int(sh.sum()) == n and st["vertices_peeled"] == n and sh.shape[0] == degeneracy + 1
    assert st["levels"] == int((sh[1:] > 0).sum())
    assert counts[0] == (n, st["simple_edges"]) and counts[-1] == (0, 0)
    assert all(x[0] >= y[0] and x[1] >= y[1] for x, y in zip(counts, counts[1:]))
    vertices, edges = counts[degeneracy]
    assert vertices > degeneracy and 2 * edges >= degeneracy * vertices  # every member has `degeneracy` neighbours inside
