"""The definition of the neighbourhood sampling (grx_sample_*) without a GPU: the two forms of tests/_sample_checker.py against each
other on small graphs in every mode, the pinned picks, closed forms and invariants that follow from the definition, one distribution
check of the definition itself, and the exports."""
import itertools
import os
import re

import numpy as np
import pytest

import gunrockinst_amd as ga
from gunrockinst_amd import capi
from oracle import gr_oracle as o

import _sample_checker as k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, v, hop, d, f) -> the picks without replacement, computed once with capi.rw_draw
PICKS = {(7, 5, 0, 10, 4): [2, 0, 8, 3], (7, 5, 2, 10, 4): [2, 0, 7, 5], (1, 0, 1, 9, 6): [2, 4, 3, 0, 7, 5]}


def chesapeake():
    g = o.build_market(os.path.join(ROOT, "tests", "golden", "chesapeake.mtx"), undirected=True)
    return g.nodes, np.asarray(g.row_offsets, dtype=np.int32), np.asarray(g.col_indices, dtype=np.int32)


def graphs():
    yield "chesapeake", chesapeake()
    yield "path", k.path(9)
    yield "star", k.star(12)
    yield "K8", k.complete(8)
    yield "cycle+tail", k.cycle_with_tail(5, 4)
    for seed, (n, p) in enumerate([(17, 0.2), (60, 0.05), (200, 0.02), (130, 0.04)]):
        yield "gnp%d" % n, k.gnp(n, p, 100 + seed, directed=bool(seed % 2))


GRAPHS = dict(graphs())
MODES = {"replace0": {}, "replace1": {"replace": True}, "weighted": {"replace": True, "weighted": True}, "all": {}}
FANOUTS = {"replace0": (3, 2, 2), "replace1": (3, 2, 2), "weighted": (3, 2, 2), "all": (2, -1, 3)}


def check_invariants(n, ro, ci, r, fanouts, replace):
    v, e = r["vertices"].shape[0], r["cols"].shape[0]
    assert np.unique(r["vertices"]).shape[0] == v, "vertices are unique"
    assert r["vertex_ptr"].shape[0] == len(fanouts) + 2 and r["edge_ptr"].shape[0] == len(fanouts) + 1
    assert r["vertex_ptr"][0] == 0 and r["vertex_ptr"][-1] == v and r["edge_ptr"][0] == 0 and r["edge_ptr"][-1] == e
    assert r["offsets"].shape[0] == v + 1 and r["offsets"][0] == 0 and r["offsets"][-1] == e and (np.diff(r["offsets"]) >= 0).all()
    # the rows of frontier h hold the edges of hop h; the rows of the last frontier are empty
    for h in range(len(fanouts)):
        assert r["offsets"][r["vertex_ptr"][h]] == r["edge_ptr"][h] and r["offsets"][r["vertex_ptr"][h + 1]] == r["edge_ptr"][h + 1]
    assert (r["offsets"][r["vertex_ptr"][len(fanouts)]:] == e).all()
    assert np.array_equal(np.asarray(ci)[r["eids"]], r["vertices"][r["cols"]]), "caller_col[eids] == vertices[cols]"
    # an edge of row l leaves vertices[l]: its entry lies in that vertex's row of the caller's CSR
    rows = np.repeat(np.arange(v), np.diff(r["offsets"]))
    assert (np.asarray(ro)[r["vertices"][rows]] <= r["eids"]).all() and (r["eids"] < np.asarray(ro)[r["vertices"][rows] + 1]).all()
    if not replace:
        for l in range(v):
            mine = r["eids"][r["offsets"][l]:r["offsets"][l + 1]]
            assert np.unique(mine).shape[0] == mine.shape[0], "the picks of a row are distinct"


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_forms_agree(name, mode):
    n, ro, ci = GRAPHS[name]
    kw = dict(MODES[mode])
    if kw.get("weighted"):
        kw["weights"] = k.row_col_weights(ro, ci)
    seeds = np.arange(n, dtype=np.int32)[::-1] if n <= 20 else np.random.default_rng(5).permutation(n)[:12]
    a = k.scalar(n, ro, ci, seeds, FANOUTS[mode], seed=77, **kw)
    b = k.vectorised(n, ro, ci, seeds, FANOUTS[mode], seed=77, **kw)
    assert k.same(a, b), [key for key in k.KEYS if not np.array_equal(a[key], b[key])]
    assert np.array_equal(a["vertices"][:len(seeds)], seeds)
    check_invariants(n, ro, ci, a, FANOUTS[mode], kw.get("replace", False))


def test_zero_weights_and_dead_rows_agree():
    n, ro, ci = k.gnp(40, 0.1, 9)
    w = k.row_col_weights(ro, ci, 3) - 1  # weights 0 .. 2: zero entries, and rows whose total is 0
    rows = np.repeat(np.arange(n), np.diff(ro))
    w[rows % 5 == 0] = 0
    seeds = np.arange(n)
    a = k.scalar(n, ro, ci, seeds, (4, 2), weights=w, replace=True, weighted=True, seed=3)
    b = k.vectorised(n, ro, ci, seeds, (4, 2), weights=w, replace=True, weighted=True, seed=3)
    assert k.same(a, b)
    assert (w[a["eids"]] > 0).all(), "a zero-weight entry is never picked"
    dead = np.nonzero((np.bincount(rows, weights=w, minlength=n) == 0))[0]
    assert dead.shape[0] and (np.diff(a["offsets"])[dead] == 0).all(), "a row whose total is 0 has no picks"
    # the weights order the rows even when the picks do not consult them
    c = k.scalar(n, ro, ci, seeds, (4, 2), weights=w, replace=True, seed=3)
    d = k.vectorised(n, ro, ci, seeds, (4, 2), weights=w, replace=True, seed=3)
    assert k.same(c, d)


@pytest.mark.parametrize("case", sorted(PICKS))
def test_pinned_picks(case):
    seed, v, hop, d, f = case
    assert k.floyd(seed, v, hop, d, f) == PICKS[case]
    # the same through both forms: row v holds the columns 0 .. d - 1, so that column = position, and a chain of `hop` vertices
    # above them leads to v, so that v is expanded at hop `hop`
    first = max(d, v + 1)
    chain = list(range(first, first + hop)) + [v]
    n, ro, ci, _ = k.csr(first + hop, [v] * d + chain[:-1], list(range(d)) + chain[1:])
    for form in (k.scalar, k.vectorised):
        r = form(n, ro, ci, [chain[0]], [1] * hop + [f], seed=seed)
        assert r["vertices"][r["cols"][r["edge_ptr"][hop]:]].tolist() == PICKS[case]
    collisions = sum(1 for s in range(f) if PICKS[case][s] == d - f + s and
                     ((int(ga.rw_draw(seed, v, hop, s)) >> 32) * (d - f + s + 1)) >> 32 != d - f + s)
    assert collisions == {(7, 5, 0, 10, 4): 1, (7, 5, 2, 10, 4): 0, (1, 0, 1, 9, 6): 2}[case]


def test_draw_is_rw_draw():
    assert int(ga.rw_draw(7, 5, 0, 3)) == k.rk.draw(7, 5, 0, 3)
    assert int(ga.rw_draw((1 << 53) - 1, (1 << 31) - 1, 15, 63)) == k.rk.draw((1 << 53) - 1, (1 << 31) - 1, 15, 63)


def test_complete_graph_rows_are_whole():
    n, ro, ci = k.complete(8)
    for f in (7, 8, 64):
        r = k.vectorised(n, ro, ci, [3], (f, f), seed=1)
        assert r["vertex_ptr"].tolist() == [0, 1, 8, 8] and r["edge_ptr"].tolist() == [0, 7, 7 + 7 * 7]
        assert r["vertices"].tolist() == [3, 0, 1, 2, 4, 5, 6, 7]
        assert np.array_equal(np.diff(r["offsets"]), [7] * 8)


def test_star_hub_picks_distinct_leaves():
    n, ro, ci = k.star(40)
    for form in (k.scalar, k.vectorised):
        r = form(n, ro, ci, [0], (9,), seed=4)
        leaves = r["vertices"][r["cols"]]
        assert leaves.shape[0] == 9 and np.unique(leaves).shape[0] == 9 and (leaves >= 1).all()
        assert r["vertices"][1:].tolist() == sorted(leaves.tolist()), "the new vertices in ascending id"


def test_isolated_seed_is_flat():
    n, ro, ci = k.csr(5, [1, 2], [2, 1])[:3]
    for form in (k.scalar, k.vectorised):
        for kw in ({}, {"replace": True}):
            r = form(n, ro, ci, [4], (3, -1, 2), seed=2, **kw)
            assert r["vertex_ptr"].tolist() == [0, 1, 1, 1, 1] and r["edge_ptr"].tolist() == [0, 0, 0, 0]
            assert r["vertices"].tolist() == [4] and r["offsets"].tolist() == [0, 0] and r["cols"].shape[0] == 0


def test_self_loops_duplicates_and_seed_ids():
    # vertex 0: a self-loop, column 2 twice, column 1; vertex 1 leads back to the seed 0 and to the seed 3
    rows, cols = [0, 0, 0, 0, 1, 1, 3], [2, 0, 2, 1, 0, 3, 2]
    n, ro, ci, _ = k.csr(4, rows, cols)
    for form in (k.scalar, k.vectorised):
        r = form(n, ro, ci, [3, 0], (-1, -1), seed=0)
        assert r["vertices"].tolist() == [3, 0, 1, 2]  # 1 and 2 are new at hop 0, in ascending id; 0 and 3 keep their seed ids
        assert r["offsets"].tolist() == [0, 1, 5, 7, 7]
        assert r["cols"].tolist() == [3, 1, 2, 3, 3, 1, 0]  # row of 0, sorted: 0, 1, 2, 2
        assert r["eids"].tolist() == [6, 1, 3, 0, 2, 4, 5]  # the duplicate column 2 in entry order


def test_floyd_subsets_are_uniform():
    import scipy.stats as scipy_stats
    d, f, count = 7, 3, 70000
    slots = np.arange(f, dtype=np.uint64)
    r = ga.rw_draw(1, np.arange(count, dtype=np.uint64)[:, None], 0, slots[None, :])
    i = (d - f) + np.arange(f, dtype=np.int64)[None, :]
    t = (((r >> np.uint64(32)) * (i + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
    i = np.broadcast_to(i, t.shape)
    for s in range(1, f):
        seen = (t[:, :s] == t[:, s:s + 1]).any(axis=1)
        t[seen, s] = i[seen, s]
    assert k.floyd(1, 11, 0, d, f) == t[11].tolist()
    subsets = {c: j for j, c in enumerate(itertools.combinations(range(d), f))}
    assert len(subsets) == 35
    seen = np.bincount([subsets[tuple(sorted(row))] for row in t.tolist()], minlength=35)
    statistic = float(((seen - count / 35.0) ** 2 / (count / 35.0)).sum())
    bound = float(scipy_stats.chi2.ppf(0.999, 34))
    print("chi-square over the 35 subsets: %.2f (bound %.2f)" % (statistic, bound))
    assert statistic < bound


def test_exports():
    names = ("SampleProblem", "SampleTooLarge", "gunrock_sample_neighbors", "SAMPLE_AUTO", "SAMPLE_LANE", "SAMPLE_GROUP", "SAMPLE_TOO_LARGE")
    for name in names:
        assert name in ga.__all__ and hasattr(ga, name), name
    assert (ga.SAMPLE_AUTO, ga.SAMPLE_LANE, ga.SAMPLE_GROUP, ga.SAMPLE_TOO_LARGE) == (0, 1, 2, -4)
    assert issubclass(ga.SampleTooLarge, ArithmeticError)
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_sample_[a-z0-9_]+)\s*\(", text))
    assert len(declared) == 12 and declared <= set(capi.exported_symbols())
    for method in ("init", "init_device", "set_option", "set_fanouts", "reset", "enact", "stats", "sizes", "extract", "device_results"):
        assert callable(getattr(ga.SampleProblem, method))
