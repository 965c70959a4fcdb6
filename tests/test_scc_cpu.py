"""The SCC checker (tests/_scc_checker.py) on the CPU: its three forms (iterative Tarjan, scipy, networkx) agree on the goldens
read directed and undirected, on the generators and on directed R-MAT, and reproduce the literals; `planted` returns its planted
partition; the undirected reading is the oracle's connected components; the header declares grx_scc_* and capi binds them (no
GPU needed)."""
import os
import re

import numpy as np
import pytest

from oracle import gr_oracle as o

from _scc_checker import (bowtie, by_networkx, by_scipy, canonical, complete_digraph, condensation, dicycle, dipath, in_star, literal, out_star,
                          planted, sizes, summary, tarjan, two_cycle_chain)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, directed entries, components, largest, trivial, sum of comp), keyed by (file, read undirected)
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

RAW = [
    (1, [0, 1], [0], [0]),                                  # one vertex with a loop
    (1, [0, 0], [], [0]),                                   # ... and without
    (6, [0] * 7, [], [0, 1, 2, 3, 4, 5]),                   # no edges
    (3, [0, 1, 3, 3], [0, 1, 1], [0, 1, 2]),                # only self-loops
    (2, [0, 3, 5], [1, 1, 1, 0, 0], [0, 0]),                # a two-cycle given with duplicates
    (4, [0, 3, 4, 6, 7], [3, 1, 2, 0, 3, 1, 2], [0, 0, 0, 0]),  # unsorted rows
    (2, [0, 1, 1], [1], [0, 1]),                            # a single one-way edge
    (3, [0, 1, 2, 3], [1, 2, 0], [0, 0, 0]),                # a three-cycle
]


def _all(nodes, ro, ci, python_loop=True):
    comp = by_scipy(nodes, ro, ci)
    assert comp.dtype == np.int32 and (comp[comp] == comp).all() and (comp <= np.arange(nodes)).all()
    assert np.array_equal(comp, by_networkx(nodes, ro, ci))
    if python_loop:
        assert np.array_equal(comp, tarjan(nodes, ro, ci))
    size = sizes(comp)
    assert size.dtype == np.int32 and int(size[comp == np.arange(nodes)].sum()) == nodes
    f, t = condensation(nodes, ro, ci, comp)
    assert f.dtype == np.int32 and (f != t).all()
    pairs = set(zip(f.tolist(), t.tolist()))
    assert len(pairs) == f.shape[0] and not any((b, a) in pairs for a, b in pairs)  # distinct, and a DAG has no two-cycle
    return comp


@pytest.mark.parametrize("name,undirected", sorted(LITERALS))
def test_forms_agree_on_goldens(golden_dir, name, undirected):
    g = o.build_market(os.path.join(golden_dir, name), undirected=undirected)
    comp = _all(g.nodes, g.row_offsets, g.col_indices)
    assert literal(g.nodes, g.row_offsets, g.col_indices, comp) == LITERALS[(name, undirected)]
    if undirected:  # mutual reachability in a symmetric graph is connectivity
        assert np.array_equal(comp, canonical(o.cc(g)[0]))


@pytest.mark.parametrize("scale", [12, 16])
def test_forms_agree_on_rmat(scale):
    g = o.rmat_seeded(scale, 8 << scale, undirected=False)
    comp = _all(g.nodes, g.row_offsets, g.col_indices)
    assert literal(g.nodes, g.row_offsets, g.col_indices, comp) == RMAT[scale]


def test_forms_agree_on_raw_csrs():
    for n, ro, ci, want in RAW:
        assert _all(n, np.array(ro, np.int32), np.array(ci, np.int32)).tolist() == want


def test_closed_forms():
    for n in (1, 2, 3, 64, 65):
        assert (_all(*complete_digraph(n)) == 0).all()
        assert (_all(*dicycle(n)) == 0).all()
        assert np.array_equal(_all(*dipath(n)), np.arange(n))
    for n in (2, 40):
        assert np.array_equal(_all(*in_star(n)), np.arange(n)) and np.array_equal(_all(*out_star(n)), np.arange(n))
    n, ro, ci = bowtie(10, 5, 7)
    comp = _all(n, ro, ci)
    assert summary(comp) == {"components": 18, "trivial": 17, "largest": 5, "largest_root": 10}
    f, t = condensation(n, ro, ci, comp)
    assert f.shape[0] == 17 and (t[:10] == 10).all() and (f[10:] == 10).all()
    for ascending in (True, False):
        n, ro, ci = two_cycle_chain(9, ascending)
        comp = _all(n, ro, ci)
        assert np.array_equal(comp, np.arange(18) // 2 * 2)
        f, t = condensation(n, ro, ci, comp)
        assert f.shape[0] == 8 and (((t - f) == 2) if ascending else ((f - t) == 2)).all()


def test_summary_ties_go_to_the_smaller_root():
    comp = np.array([0, 0, 2, 2, 4], np.int32)
    assert summary(comp) == {"components": 3, "trivial": 1, "largest": 2, "largest_root": 0}
    assert sizes(comp).tolist() == [2, 2, 2, 2, 1]


@pytest.mark.parametrize("seed", [1, 2])
def test_planted_returns_its_partition(seed):
    rng = np.random.default_rng(seed)
    blocks = rng.choice([1, 2, 3, 64, 65, 1000], 60)
    n, ro, ci, comp, block = planted(blocks, 0.002, 0.05, seed)
    assert n == int(blocks.sum()) and np.array_equal(_all(n, ro, ci, python_loop=seed == 1), comp)
    f, t = condensation(n, ro, ci, comp)
    assert f.shape[0] > 0 and (block[f] < block[t]).all()  # every link goes from a lower block to a higher one


def test_header_declares_scc_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_scc_[a-z0-9_]+)\s*\(", text))
    want = {"grx_scc_create", "grx_scc_init", "grx_scc_init_device", "grx_scc_set_option", "grx_scc_reset", "grx_scc_enact", "grx_scc_stats",
            "grx_scc_phase_trace", "grx_scc_extract", "grx_scc_summary", "grx_scc_sizes", "grx_scc_condensation", "grx_scc_device_results",
            "grx_scc_destroy"}
    assert want == declared, want ^ declared
    from gunrockinst_amd import capi
    import gunrockinst_amd as ga
    assert declared <= set(capi.exported_symbols()), declared - set(capi.exported_symbols())
    for name in ("SccProblem", "gunrock_scc", "gunrock_condensation"):
        assert hasattr(ga, name), name
    assert (ga.SCC_AUTO, ga.SCC_ROUNDS, ga.SCC_DEVICE_LOOP) == (0, 1, 2)
    for method in ("init", "init_device", "set_option", "reset", "enact", "stats", "phase_trace", "extract", "summary", "sizes",
                   "condensation", "device_results", "close"):
        assert callable(getattr(ga.SccProblem, method)), method
    legacy = open(os.path.join(ROOT, "include", "gunrock", "gunrock.h")).read()
    assert "grx_scc" not in legacy and "gunrock_scc" not in legacy
