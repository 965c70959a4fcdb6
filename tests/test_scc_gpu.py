"""Strongly connected components on the GPU (grx_scc_*): `comp` must equal tests/_scc_checker.py's on every input, int32 against
int32 with np.array_equal -- goldens read directed and undirected, raw CSRs of every awkward shape, rows at the lane / wave
boundary, closed forms that stress one mechanism each (a star's hub, a path trimmed to nothing, a cycle's chain of search levels,
colouring's one-component-per-round chain), planted partitions under every schedule and option on one handle, R-MAT -- and the
device-built scale-20 R-MAT must satisfy invariants a wrong kernel breaks."""
import functools
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

from _scc_checker import (bowtie, complete_digraph, condensation, dicycle, dipath, from_edges, in_star, literal, out_star, planted, scc, sizes,
                          summary, two_cycle_chain)

pytestmark = pytest.mark.gpu

SCHEDULES = (ga.SCC_AUTO, ga.SCC_ROUNDS, ga.SCC_DEVICE_LOOP)
# (n, directed entries, components, largest, trivial, sum of comp), keyed by (file, read undirected): computed on the CPU by the
# checker's three forms (tests/test_scc_cpu.py)
LITERALS = {
    ("bips98_606.mtx", False): (7135, 27838, 1070, 6066, 1069, 1104684),
    ("bips98_606.mtx", True): (7135, 30380, 542, 6594, 541, 521647),
    ("chesapeake.mtx", False): (39, 170, 39, 1, 39, 741),
    ("chesapeake.mtx", True): (39, 340, 1, 39, 0, 0),
    ("test_bc.mtx", False): (7, 15, 5, 2, 3, 18),
    ("test_cc.mtx", False): (11, 20, 9, 2, 7, 52),
    ("test_cc.mtx", True): (11, 36, 2, 7, 0, 28),
    ("test_pr.mtx", False): (4, 8, 1, 4, 0, 0),
}
RMAT = {12: (4096, 29522, 1867, 2230, 1866, 4759543), 16: (65536, 503300, 36418, 29119, 36417, 1393929348)}


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    """(nodes, row_offsets, col_indices, the checker's comp): computed once, shared, never written"""
    g = o.rmat_seeded(scale, 8 << scale, undirected=False)
    ref = scc(g.nodes, g.row_offsets, g.col_indices)
    ref.setflags(write=False)
    return g.nodes, g.row_offsets, g.col_indices, ref


def _run(p, **options):
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    p.reset()
    p.enact()
    comp, components = p.extract()
    assert comp.dtype == np.int32
    return comp.copy(), components, p.stats()


def _check(nodes, ro, ci, ref=None, **options):
    """one full run against the checker: comp, the count, sizes, summary, the condensation, the trace"""
    if ref is None:
        ref = scc(nodes, ro, ci)
    p = ga.SccProblem().init(nodes, ro, ci)
    comp, components, st = _run(p, **options)
    assert np.array_equal(comp, ref), "comp differs from the checker at %s" % np.flatnonzero(comp != ref)[:10]
    want = summary(ref)
    assert components == want["components"] and p.summary() == want
    assert p.extract(comp=False) == (None, components)
    size = p.sizes()
    assert size.dtype == np.int32 and np.array_equal(size, sizes(ref))
    f, t, count = p.condensation()
    ref_f, ref_t = condensation(nodes, ro, ci, ref)
    assert f.dtype == np.int32 and t.dtype == np.int32 and count == ref_f.shape[0] and np.array_equal(f, ref_f) and np.array_equal(t, ref_t)
    none_f, none_t, only_count = p.condensation(max_edges=0)
    assert none_f.shape[0] == none_t.shape[0] == 0 and only_count == count
    kind, vertices, ms = p.phase_trace()
    assert int(vertices.sum()) == nodes and (vertices >= 0).all() and (ms >= 0).all() and set(kind.tolist()) <= {0, 1, 2}
    assert int(vertices[kind == ga.SCC_TRIM].sum()) == st["trimmed"] and int((kind == ga.SCC_COLOUR).sum()) == st["colour_rounds"]
    assert int(vertices[kind == ga.SCC_PIVOT].sum()) == st["pivot_component"]
    p.close()
    return comp, st


@pytest.mark.parametrize("name,undirected", sorted(LITERALS))
def test_goldens(golden_dir, name, undirected):
    g = o.build_market(os.path.join(golden_dir, name), undirected=undirected)
    ref = scc(g.nodes, g.row_offsets, g.col_indices)
    assert literal(g.nodes, g.row_offsets, g.col_indices, ref) == LITERALS[(name, undirected)]
    for schedule in SCHEDULES:
        for pivot_phase in (0, 1):
            _check(g.nodes, g.row_offsets, g.col_indices, ref, schedule=schedule, pivot_phase=pivot_phase)
    comp, components = ga.gunrock_scc(g.nodes, g.row_offsets, g.col_indices)
    assert np.array_equal(comp, ref) and components == LITERALS[(name, undirected)][2]
    one_comp, f, t = ga.gunrock_condensation(g.nodes, g.row_offsets, g.col_indices)
    ref_f, ref_t = condensation(g.nodes, g.row_offsets, g.col_indices, ref)
    assert np.array_equal(one_comp, ref) and np.array_equal(f, ref_f) and np.array_equal(t, ref_t)


@pytest.mark.parametrize("scale", [12, 16])
def test_rmat(scale):
    n, ro, ci, ref = _rmat(scale)
    assert literal(n, ro, ci, ref) == RMAT[scale]
    comp, st = _check(n, ro, ci, ref)
    print("rmat%d auto: %s" % (scale, st))
    assert st["pivot_component"] == RMAT[scale][3]  # the pivot sits in the giant component
    for schedule in (ga.SCC_ROUNDS, ga.SCC_DEVICE_LOOP) if scale == 12 else (ga.SCC_ROUNDS,):
        _check(n, ro, ci, ref, schedule=schedule)
    _check(n, ro, ci, ref, pivot_phase=0)


RAW = [
    (1, [0, 1], [0], [0]),                                  # one vertex with a loop
    (1, [0, 0], [], [0]),                                   # ... and without
    (6, [0] * 7, [], [0, 1, 2, 3, 4, 5]),                   # no edges
    (3, [0, 1, 3, 3], [0, 1, 1], [0, 1, 2]),                # only self-loops
    (2, [0, 3, 5], [1, 1, 1, 0, 0], [0, 0]),                # a two-cycle given with duplicates
    (4, [0, 3, 4, 6, 7], [3, 1, 2, 0, 3, 1, 2], [0, 0, 0, 0]),  # unsorted rows
    (2, [0, 1, 1], [1], [0, 1]),                            # a single one-way edge
]


def test_raw_csrs():
    for n, ro, ci, want in RAW:
        for trim in (0, 1):
            comp, _ = _check(n, np.array(ro, np.int32), np.array(ci, np.int32), trim=trim)
            assert comp.tolist() == want
    for schedule in SCHEDULES:  # a three-cycle
        for pivot_phase in (0, 1):
            comp, _ = _check(3, np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32), schedule=schedule, pivot_phase=pivot_phase)
            assert comp.tolist() == [0, 0, 0]


@pytest.mark.parametrize("row", [15, 16, 17, 63, 64, 65, 256, 257])
def test_row_walk_boundaries(row):
    """vertex 0 sits in a cycle 0 -> 1 -> 2 -> 0 and has `row` out-entries and `row` in-entries; the other ends are leaves, each
    its own component"""
    extra = row - 1
    n = 3 + 2 * extra
    outs, ins = 3 + np.arange(extra), 3 + extra + np.arange(extra)
    src = np.concatenate([[0, 1, 2], np.zeros(extra, np.int64), ins])
    dst = np.concatenate([[1, 2, 0], outs, np.zeros(extra, np.int64)])
    n, ro, ci = from_edges(n, src, dst)
    assert ro[1] - ro[0] == row and int((ci == 0).sum()) == row
    want = np.arange(n, dtype=np.int32)
    want[:3] = 0
    for schedule in SCHEDULES:
        for trim in (0, 1):
            comp, st = _check(n, ro, ci, schedule=schedule, trim=trim, wave_min_row=16)
            assert np.array_equal(comp, want)
            assert st["trimmed"] == (n - 3 if trim else 0)


@pytest.mark.parametrize("n", [63, 64, 65, 1024, 1025])
def test_vertex_count_boundaries(n):
    for make in (complete_digraph, dicycle):
        nodes, ro, ci = make(n)
        for pivot_phase in (0, 1):
            comp, st = _check(nodes, ro, ci, np.zeros(n, np.int32), pivot_phase=pivot_phase)
            assert st["trimmed"] == 0 and st["pivot_component"] == (n if pivot_phase else 0)


def test_closed_forms():
    comp, st = _check(*complete_digraph(300))
    assert (comp == 0).all() and st["pivot_component"] == 300
    n, ro, ci = dipath(5001)
    comp, st = _check(n, ro, ci)
    assert np.array_equal(comp, np.arange(n)) and st["trimmed"] == n and st["colour_rounds"] == 0 and st["pivot_component"] == 0
    for make in (in_star, out_star):  # the hub takes 99 999 decrements in one sub-round and is appended once
        n, ro, ci = make(100_000)
        comp, st = _check(n, ro, ci, np.arange(n, dtype=np.int32))
        assert st["trimmed"] == n and st["trim_rounds"] <= 2, st
    n, ro, ci = bowtie(1000, 500, 1000)
    comp, st = _check(n, ro, ci)
    assert summary(comp) == {"components": 2001, "trivial": 2000, "largest": 500, "largest_root": 1000}
    assert st["trimmed"] == 2000 and st["pivot_component"] == 500


def test_device_loop_is_a_loop():
    """a directed cycle of 20 001 vertices: nothing to trim, 20 001 levels of each search from the pivot.  The plain form takes a
    launch per level; the device loop a launch per few thousand of them."""
    n, ro, ci = dicycle(20_001)
    launches = {}
    p = ga.SccProblem().init(n, ro, ci)
    for schedule in SCHEDULES:
        comp, components, st = _run(p, schedule=schedule, trim=1)
        assert (comp == 0).all() and components == 1
        launches[schedule] = st["kernel_launches"]
        print("dicycle(20001) schedule %d: %s" % (schedule, st))
    p.close()
    assert launches[ga.SCC_ROUNDS] >= 20_001
    assert launches[ga.SCC_AUTO] * 10 <= 20_001 and launches[ga.SCC_DEVICE_LOOP] * 10 <= 20_001


@pytest.mark.parametrize("ascending", [True, False])
def test_colouring_worst_case(ascending):
    n, ro, ci = two_cycle_chain(2000, ascending)
    want = (np.arange(n) // 2 * 2).astype(np.int32)
    for pivot_phase in (0, 1):
        comp, st = _check(n, ro, ci, want, pivot_phase=pivot_phase)
        print("two_cycle_chain(2000, ascending=%s) pivot_phase %d: %s" % (ascending, pivot_phase, st))
    # without the pair step every pair is a colouring round (about 2000 sweeps each when the ids fall: not run at this size,
    # test_colouring_one_component_per_round runs it at 100 pairs); with the ids rising one round finishes them all
    if ascending:
        comp, st = _check(n, ro, ci, want, pair_trim=0)
        print("two_cycle_chain(2000, ascending=True) pair_trim 0: %s" % st)


def test_colouring_one_component_per_round():
    """the falling chain without trimming and without a pivot: the largest live id reaches everything downstream and is reached
    from its own pair alone, so every colouring round finishes exactly one pair"""
    n, ro, ci = two_cycle_chain(100, False)
    for schedule in SCHEDULES:
        comp, st = _check(n, ro, ci, (np.arange(n) // 2 * 2).astype(np.int32), schedule=schedule, trim=0, pivot_phase=0)
        assert st["colour_rounds"] == 100 and st["trimmed"] == 0 and st["pivot_component"] == 0, st


@pytest.mark.parametrize("seed", [11, 12])
def test_planted_partitions_every_option_one_handle(seed):
    rng = np.random.default_rng(seed)
    n, ro, ci, ref, block = planted(rng.choice([1, 2, 3, 64, 65, 1000], 200), 0.002, 0.02, seed)
    assert np.array_equal(scc(n, ro, ci), ref)
    p = ga.SccProblem().init(n, ro, ci)
    seen = set()
    for schedule in SCHEDULES:
        for pivot_phase in (0, 1):
            for trim in (0, 1):
                for wave_min_row in (1, 64, 1 << 30):
                    comp, components, _ = _run(p, schedule=schedule, pivot_phase=pivot_phase, trim=trim, wave_min_row=wave_min_row)
                    assert np.array_equal(comp, ref), (schedule, pivot_phase, trim, wave_min_row)
                    seen.add(comp.tobytes())
    assert len(seen) == 1
    f, t, count = p.condensation()
    p.close()
    ref_f, ref_t = condensation(n, ro, ci, ref)
    assert np.array_equal(f, ref_f) and np.array_equal(t, ref_t) and count > 0
    assert (block[f] < block[t]).all()  # every pair goes from a lower block to a higher one


def test_handle_rules():
    with pytest.raises(RuntimeError, match="code -1"):
        ga.SccProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.SccProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a decreasing offset
        ga.SccProblem().init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not end at `edges` (nothing else wrong)
        ga.SccProblem().init(2, np.array([0, 1, 1], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(ValueError):  # a wrong offsets length
        ga.SccProblem().init(3, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    p = ga.SccProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        p.init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match="code -3"):  # a handle takes one graph, also after a rejection
        p.init(2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32))
    with pytest.raises(RuntimeError):  # nothing to run on
        p.enact()
    p.close()
    p = ga.SccProblem()
    for call in (p.reset, p.enact, p.extract, p.summary, p.sizes, p.condensation):  # before Init: an error code, nothing touched
        with pytest.raises(RuntimeError, match="failed"):
            call()
    assert p.device_results() == (None, None, None)
    assert p.set_option("no_such_option", 1) == 1
    assert p.set_option("schedule", 2) == 0 and p.set_option("schedule", 0) == 0
    assert p.set_option("pair_trim", 0) == 0 and p.set_option("pair_trim", 1) == 0
    for name, value in (("schedule", 3), ("schedule", -1), ("pivot_phase", 2), ("pivot_phase", -1), ("trim", 2), ("pair_trim", 2), ("wave_min_row", 0),
                        ("loop_max_list", -1), ("loop_max_entries", -1)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    n, ro, ci, ref = _rmat(12)
    p.init(n, ro, ci)
    with pytest.raises(RuntimeError, match="code -3"):  # a second graph for the same handle
        p.init(n, ro, ci)
    # results asked for before the first Enact: no vertex has a representative, nothing is indexed with fresh memory
    early, early_count = p.extract()
    assert (early == -1).all() and early_count == 0 and p.condensation()[2] == 0 and p.summary()["components"] == 0
    assert (p.sizes() == -1).all()
    a, count_a, _ = _run(p)
    b, count_b, _ = _run(p)
    assert a.tobytes() == b.tobytes() == ref.tobytes() and count_a == count_b
    p.enact()  # an Enact that does not follow a Reset makes its own
    assert p.extract()[0].tobytes() == ref.tobytes()
    assert p.extract(comp=False) == (None, count_a)
    p.close()


def _row_multisets(ro, ci):
    """a CSR's entries sorted inside each row"""
    rows = np.repeat(np.arange(ro.shape[0] - 1), np.diff(ro))
    order = np.lexsort((ci, rows))
    return ci[order]


def test_init_device_and_device_results():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(16, undirected=False)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.SccProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    comp, components, st = _run(p)
    d_comp, d_iro, d_ici = p.device_results()
    on_device = devgraph.as_tensor(d_comp, n, "<i4").cpu().numpy()
    iro = devgraph.as_tensor(d_iro, n + 1, "<i4").clone()
    ici = devgraph.as_tensor(d_ici, m, "<i4").clone()
    h_ro, h_ci = ro.cpu().numpy(), ci.cpu().numpy()
    _, o_ro, o_ci, ref = _rmat(16)
    if not (np.array_equal(h_ro, o_ro) and np.array_equal(h_ci, o_ci)):  # (the device build gives the oracle's CSR: the shared answer serves)
        ref = scc(n, h_ro, h_ci)
    assert on_device.dtype == np.int32 and np.array_equal(on_device, comp) and np.array_equal(comp, ref) and st["build_ms"] > 0
    # the transpose it built: the same entries as numpy's, row by row as multisets
    t_ro, t_ci = iro.cpu().numpy(), ici.cpu().numpy()
    _, want_ro, want_ci = from_edges(n, h_ci, np.repeat(np.arange(n), np.diff(h_ro)))
    assert np.array_equal(t_ro, want_ro) and np.array_equal(_row_multisets(t_ro, t_ci), _row_multisets(want_ro, want_ci))
    # a borrowed transpose gives the same comp as a built one
    torch.cuda.synchronize()
    q = ga.SccProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr(), iro.data_ptr(), ici.data_ptr())
    other, other_components, other_st = _run(q)
    assert q.device_results()[1:] == (iro.data_ptr(), ici.data_ptr()) and other_st["build_ms"] == 0
    q.close()
    p.close()
    assert other.tobytes() == comp.tobytes() and other_components == components
    with pytest.raises(RuntimeError, match="code -1"):  # one inverse array without the other
        ga.SccProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr(), None, ici.data_ptr())


def test_device_rmat20_invariants():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(20, undirected=False)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    torch.cuda.synchronize()
    p = ga.SccProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
    comp, components, st = _run(p)
    print("rmat20 auto: components %d %s" % (components, st))
    size = p.sizes()
    s = p.summary()
    f, t, count = p.condensation()
    other, other_components, other_st = _run(p, schedule=ga.SCC_ROUNDS)
    print("rmat20 rounds: %s" % other_st)
    p.close()
    assert other.tobytes() == comp.tobytes() and other_components == components
    ids = np.arange(n)
    assert (comp[comp] == comp).all() and (comp <= ids).all()
    roots = comp == ids
    assert int(roots.sum()) == components == s["components"] and int(size[roots].sum()) == n
    assert np.array_equal(size, size[comp]) and np.array_equal(size, np.bincount(comp, minlength=n)[comp])
    assert s["largest"] == int(size.max()) and s["trivial"] == int((size[roots] == 1).sum())
    assert size[s["largest_root"]] == s["largest"] and s["largest_root"] == int(np.flatnonzero(roots & (size == s["largest"]))[0])
    assert count == f.shape[0] and roots[f].all() and roots[t].all() and (f != t).all()
    keys = f.astype(np.int64) * n + t
    assert (np.diff(keys) > 0).all()  # sorted by (from, to), distinct
    assert not np.isin(t.astype(np.int64) * n + f, keys).any()  # no pair with its reverse: a DAG has no two-cycle
