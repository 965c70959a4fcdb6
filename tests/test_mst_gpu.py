"""Minimum spanning forest on the GPU (grx_mst_*): `selected` must equal the Kruskal checker's bit for bit on every input --
fixtures, the golden MARKET files (real, possibly negative weights; all-ones pattern files, where only the tie-break decides),
raw CSRs of every awkward shape, deep paths and stars, R-MAT with mirrored and independent weights -- and the device-built
scale-22 R-MAT is checked against scipy and against its own component count."""
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

from _mst_checker import components, entry_rows, kruskal, scipy_forest_weight

pytestmark = pytest.mark.gpu

IMIN, IMAX = int(np.iinfo(np.int32).min), int(np.iinfo(np.int32).max)


def _run(nodes, ro, ci, w):
    p = ga.MstProblem().init(nodes, ro, ci, w)
    p.reset()
    p.enact()
    out = p.extract()
    st = p.stats()
    p.close()
    return out, st


def _check(nodes, ro, ci, w):
    (sel, total, count), st = _run(nodes, ro, ci, w)
    ref_sel, ref_total, ref_count = kruskal(nodes, ro, ci, w)
    assert np.array_equal(sel, ref_sel), "selected differs from Kruskal at %s" % np.flatnonzero(sel != ref_sel)[:10]
    assert total == ref_total and count == ref_count
    return st


def _hashed_weights(rows, cols):
    """symmetric weights 1..64: a hash of (min(u, v), max(u, v))"""
    lo = np.minimum(rows, cols).astype(np.uint64)
    hi = np.maximum(rows, cols).astype(np.uint64)
    h = (lo * np.uint64(0x9E3779B1) + hi * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    return (h % np.uint64(64) + np.uint64(1)).astype(np.int32)


def test_fixture7_chosen_weights(golden):
    f = golden["fixture7"]
    ro, ci = np.array(f["row_offsets"], np.int32), np.array(f["col_indices"], np.int32)
    for w in ([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9], f["sssp_weights"], [1] * 15, [-7] * 15):
        _check(7, ro, ci, np.array(w, np.int32))


def test_bips98_606_own_weights(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "bips98_606.mtx"), undirected=True)
    assert g.edge_values is not None and (g.edge_values < 0).any()  # (the loader drops the diagonal, as Csr::FromCoo does)
    st = _check(g.nodes, g.row_offsets, g.col_indices, g.edge_values)
    assert st["rounds"] >= 1


@pytest.mark.parametrize("name", ["chesapeake.mtx", "test_bc.mtx", "test_cc.mtx", "test_pr.mtx"])
def test_pattern_files_tie_break_only(golden_dir, name):
    for und in (True, False):
        g = o.build_market(os.path.join(golden_dir, name), undirected=und)
        _check(g.nodes, g.row_offsets, g.col_indices, np.ones(g.edges, np.int32))


def test_raw_csrs():
    # unsorted rows, duplicates, asymmetric weights on mirrored edges
    _check(4, np.array([0, 4, 6, 8, 9], np.int32), np.array([3, 1, 2, 1, 2, 0, 0, 1, 0], np.int32),
           np.array([5, 2, 7, 2, 1, 9, 3, 4, 6], np.int32))
    # self-loops only, one vertex, no edges
    _check(3, np.array([0, 1, 3, 3], np.int32), np.array([0, 1, 1], np.int32), np.array([-1, IMIN, IMAX], np.int32))
    _check(1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([4], np.int32))
    (sel, total, count), _ = _run(1, np.array([0, 0], np.int32), np.array([], np.int32), np.array([], np.int32))
    assert sel.shape == (0,) and total == 0 and count == 0
    (sel, total, count), _ = _run(6, np.zeros(7, np.int32), np.array([], np.int32), np.array([], np.int32))
    assert total == 0 and count == 0
    # extreme weights, mirrored and not
    ro = np.array([0, 3, 5, 7, 9], np.int32)
    ci = np.array([1, 2, 3, 0, 2, 0, 1, 0, 2], np.int32)
    _check(4, ro, ci, np.array([IMAX, IMIN, IMAX, IMAX, 0, IMIN, 0, IMAX, IMIN], np.int32))
    _check(4, ro, ci, np.array([IMAX, IMAX, IMAX, IMAX, IMAX, IMAX, IMAX, IMAX, IMAX], np.int32))
    _check(4, ro, ci, np.array([IMIN, IMIN, IMIN, IMIN, IMIN, IMIN, IMIN, IMIN, IMIN], np.int32))


def test_rejects_bad_input():
    with pytest.raises(RuntimeError, match="code -1"):
        ga.MstProblem().init(0, np.array([0], np.int32), np.array([], np.int32), np.array([], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # a column outside [0, nodes)
        ga.MstProblem().init(2, np.array([0, 1, 1], np.int32), np.array([2], np.int32), np.array([1], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):  # offsets that do not end at `edges`
        ga.MstProblem().init(2, np.array([0, 2, 1], np.int32), np.array([1], np.int32), np.array([1], np.int32))


def _path(n, mirrored=True):
    if mirrored:
        rows = np.concatenate([np.arange(n - 1), np.arange(1, n)])
        cols = np.concatenate([np.arange(1, n), np.arange(n - 1)])
    else:
        rows, cols = np.arange(n - 1), np.arange(1, n)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    return np.searchsorted(rows, np.arange(n + 1)).astype(np.int32), cols.astype(np.int32), rows


def test_deep_path_and_star():
    n = 200_000
    ro, ci, rows = _path(n)
    st = _check(n, ro, ci, np.ones(ci.shape[0], np.int32))  # every vertex hooks left in round 1: one chain n deep
    assert st["rounds"] == 1
    rng = np.random.default_rng(7)
    _check(n, ro, ci, rng.integers(1, 1 << 20, ci.shape[0]).astype(np.int32))  # independent weights per entry
    w = _hashed_weights(rows, ci) + (rng.integers(0, 1 << 20, n + 1)[np.minimum(rows, ci)] << 6).astype(np.int32)
    st = _check(n, ro, ci, w)  # mirrored, random symmetric weights: many rounds
    assert st["rounds"] >= 3
    # star, hub = the largest id, both orientations and one orientation
    hub = n - 1
    leaves = np.arange(hub)
    for mirrored in (True, False):
        rows = np.concatenate([leaves, np.full(hub, hub)]) if mirrored else leaves
        cols = np.concatenate([np.full(hub, hub), leaves]) if mirrored else np.full(hub, hub)
        ro = np.searchsorted(rows, np.arange(n + 1)).astype(np.int32)
        _check(n, ro, cols.astype(np.int32), _hashed_weights(rows, cols))


@pytest.mark.parametrize("scale", [16, 17, 18])
def test_rmat_host(scale):
    g = o.rmat_seeded(scale, 8 << scale, undirected=True)
    rows = entry_rows(g.row_offsets)
    _check(g.nodes, g.row_offsets, g.col_indices, _hashed_weights(rows, g.col_indices))  # mirrored weights: the row round
    rng = np.random.default_rng(scale)
    _check(g.nodes, g.row_offsets, g.col_indices, rng.integers(-50, 50, g.edges).astype(np.int32))  # independent per entry


def test_general_path_on_mirrored_input_gives_the_same_bits(monkeypatch):
    g = o.rmat_seeded(14, 8 << 14, undirected=True)
    w = _hashed_weights(entry_rows(g.row_offsets), g.col_indices)
    (fast, _, _), _ = _run(g.nodes, g.row_offsets, g.col_indices, w)
    monkeypatch.setenv("GUNROCK_MST_MIRRORED", "0")
    (general, _, _), _ = _run(g.nodes, g.row_offsets, g.col_indices, w)
    assert np.array_equal(fast, general) and np.array_equal(fast, kruskal(g.nodes, g.row_offsets, g.col_indices, w)[0])


def test_one_shot_agrees_with_problem_and_repeats():
    g = o.rmat_seeded(15, 8 << 15, undirected=False)
    w = np.random.default_rng(3).integers(1, 3, g.edges).astype(np.int32)
    p = ga.MstProblem(instrument=True).init(g.nodes, g.row_offsets, g.col_indices, w)
    runs = []
    for _ in range(3):
        p.reset()
        p.enact()
        runs.append(p.extract())
    trace = p.round_trace()
    assert len(trace) == p.stats()["rounds"] and all(r["ms"] > 0 for r in trace)
    p.close()
    for sel, total, count in runs[1:]:
        assert np.array_equal(sel, runs[0][0]) and (total, count) == runs[0][1:]
    sel, total, count = ga.gunrock_mst(g.nodes, g.row_offsets, g.col_indices, w)
    assert np.array_equal(sel, runs[0][0]) and (total, count) == runs[0][1:]
    assert np.array_equal(sel, kruskal(g.nodes, g.row_offsets, g.col_indices, w)[0])


def test_device_rmat22_init_device():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(22)
    n, m = int(ro.shape[0]) - 1, int(ci.shape[0])
    rows = torch.repeat_interleave(torch.arange(n, device=ci.device, dtype=torch.int64), (ro[1:] - ro[:-1]).long())
    lo, hi = torch.minimum(rows, ci.long()), torch.maximum(rows, ci.long())
    h = (lo * 0x9E3779B1 + hi * 0x85EBCA77) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    w = (h % 64 + 1).int().contiguous()
    torch.cuda.synchronize()
    p = ga.MstProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr(), w.data_ptr())
    p.reset()
    p.enact()
    sel, total, count = p.extract()
    p.reset()
    p.enact()
    sel2, total2, count2 = p.extract()
    st = p.stats()
    p.close()
    assert np.array_equal(sel, sel2) and (total, count) == (total2, count2)
    h_ro, h_ci, h_w = ro.cpu().numpy(), ci.cpu().numpy(), w.cpu().numpy()
    h_rows = entry_rows(h_ro)
    assert int(sel.astype(np.int64) @ h_w.astype(np.int64)) == total
    assert total == scipy_forest_weight(n, h_ro, h_ci, h_w)
    comps = components(n, h_rows, h_ci)
    assert count == n - comps
    chosen = sel == 1
    assert int(chosen.sum()) == count and components(n, h_rows[chosen], h_ci[chosen]) == comps  # acyclic
    assert (h_rows[chosen] < h_ci[chosen]).all()  # mirrored, equal weights: always the u < v copy
    assert st["rounds"] >= 2
