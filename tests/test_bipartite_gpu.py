"""Maximum bipartite matching and the Dulmage-Mendelsohn decomposition on the GPU (grx_bipartite_*): the size, the parts, their
sizes, the cover and the blocks must equal tests/_bipartite_checker.py's with np.array_equal; the matching, which is one of many,
must pass the checker's validate with that size; the certificate counts in the stats must be (0, 0, size).  Degenerate shapes, the
chain whose forced start leaves one augmenting path of 2 k + 1 edges (across a wave, and past the steps of one device-loop launch),
one tree with many ends, complete matrices without the greedy start, every forced strategy around its thresholds, the literals and
the goldens, warm starts, capped runs, handle reuse, the device paths and the refusals."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import maximum_bipartite_matching

import gunrockinst_amd as ga

import _bipartite_checker as k

pytestmark = pytest.mark.gpu

NOT_READY = "code 600"  # hipErrorNotReady
STRATEGIES = (ga.BIPARTITE_AUTO, ga.BIPARTITE_LANE, ga.BIPARTITE_WAVE, ga.BIPARTITE_BLOCK)
_MATRICES = {}


def _matrix(key, make):
    """registers a matrix under a name, so that its reference is computed once and shared"""
    if key not in _MATRICES:
        _MATRICES[key] = make()
    return key


@functools.lru_cache(maxsize=None)
def _reference(key):
    ref = k.decompose(_MATRICES[key])
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def _problem(key, instrument=False):
    shape, ro, ci = _MATRICES[key]
    return ga.BipartiteProblem(instrument=instrument).init(shape, ro, ci)


def _compare(p, key, what):
    """everything of a finished BIPARTITE_MAXIMUM run against the checker; returns the stats"""
    ref = _reference(key)
    st = p.stats()
    print(what, {x: st[x] for x in ("size", "phases", "levels", "vertical_levels", "augmentations", "greedy_pairs", "certificate", "regime_columns",
                                    "loop_levels", "kernel_launches", "readbacks")})
    m = p.extract_matching()
    assert m["mate_row"].dtype == np.int32 and m["mate_col"].dtype == np.int32
    assert k.validate(_MATRICES[key], m["mate_row"], m["mate_col"]) == ref["size"] == m["size"] == st["size"], what
    assert st["state"] == ga.BIPARTITE_MAXIMUM and st["certificate"] == [0, 0, ref["size"]], (what, st)
    assert st["augmentations"] == sum(p.phase_trace()[1].tolist()) and st["phases"] + 1 == len(p.phase_trace()[0]), what
    row_part, col_part, sizes = p.extract_parts()
    assert row_part.dtype == np.int32 and np.array_equal(row_part, ref["row_part"]) and np.array_equal(col_part, ref["col_part"]), what
    assert sizes == ref["part_sizes"], what
    row_cover, col_cover = p.extract_cover()
    assert row_cover.dtype == np.uint8 and np.array_equal(row_cover, ref["row_cover"]) and np.array_equal(col_cover, ref["col_cover"]), what
    row_block, col_block, blocks = p.blocks()
    assert row_block.dtype == np.int32 and np.array_equal(row_block, ref["row_block"]) and np.array_equal(col_block, ref["col_block"]), what
    assert blocks == ref["blocks"], what
    return st


def _run(key, what=None, start=None, instrument=False, **options):
    p = _problem(key, instrument)
    try:
        for name, value in options.items():
            assert p.set_option(name, value) == 0, name
        p.reset(start)
        p.enact()
        return _compare(p, key, what or key + " " + str(options))
    finally:
        p.close()


def _pairs(shape, pairs):
    return lambda: k.from_pairs(shape, [a for a, _ in pairs], [b for _, b in pairs])


def _full(rows, cols):
    return lambda: k.from_pairs((rows, cols), np.repeat(np.arange(rows), cols), np.tile(np.arange(cols), rows))


LITERAL = [(0, 0), (0, 1), (0, 2), (1, 2), (1, 3), (1, 4), (2, 2), (2, 3), (3, 4), (4, 4)]


# ---------------- degenerate shapes ----------------

@pytest.mark.parametrize("greedy", [1, 0])
def test_degenerate_shapes(greedy):
    cases = {
        "0x0": _pairs((0, 0), []), "0x3": _pairs((0, 3), []), "3x0": _pairs((3, 0), []), "1x1": _pairs((1, 1), [(0, 0)]),
        "1x1 empty": _pairs((1, 1), []), "4x6 empty": _pairs((4, 6), []),
        # empty rows and columns among full ones
        "gaps": _pairs((6, 7), [(0, 0), (0, 2), (0, 5), (2, 0), (2, 2), (2, 5), (5, 0), (5, 2), (5, 5), (3, 6)]),
        # duplicates and unsorted rows
        "duplicates": _pairs((4, 4), [(0, 3), (0, 1), (0, 3), (0, 1), (1, 1), (1, 1), (2, 2), (2, 0), (2, 2), (3, 1), (3, 1), (3, 1)]),
    }
    for name, make in cases.items():
        st = _run(_matrix(name, make), greedy=greedy)
        assert st["greedy_pairs"] == 0 or greedy


# ---------------- the chain ----------------

def _chain(kk):
    def make():
        return k.from_pairs((kk + 1, kk + 1), list(range(kk + 1)) + list(range(kk)), list(range(kk + 1)) + list(range(1, kk + 1)))
    return _matrix("chain %d" % kk, make)


@pytest.mark.parametrize("kk", [65, 5000])
def test_chain(kk):
    key = _chain(kk)
    start = np.array(list(range(1, kk + 1)) + [-1], np.int32)  # row i holds column i + 1: row k and column 0 are left
    stats = {}
    for schedule in (ga.BIPARTITE_ROUNDS, ga.BIPARTITE_DEVICE_LOOP, ga.BIPARTITE_SCHEDULE_AUTO):
        st = _run(key, start=start, greedy=0, schedule=schedule)
        # one augmenting path of 2 k + 1 edges: the first phase walks k + 1 levels to its end, the second has no root
        assert (st["phases"], st["levels"], st["augmentations"], st["greedy_pairs"]) == (2, kk + 1, 1, 0), st
        stats[schedule] = st
    # read-backs: one per search start (two phases and the search from the rows), one per wide level or per launch of the device
    # loop (4096 steps at the most: DESIGN.md 3.21), one for the certificate
    rounds, loop = stats[ga.BIPARTITE_ROUNDS], stats[ga.BIPARTITE_DEVICE_LOOP]
    assert rounds["loop_levels"] == 0 and rounds["readbacks"] == 3 + (kk + 1) + 1, rounds
    assert loop["loop_levels"] == kk + 1 and loop["readbacks"] == 3 + -(-(kk + 1) // 4096) + 1, loop
    assert stats[ga.BIPARTITE_SCHEDULE_AUTO]["loop_levels"] == kk + 1  # (every level is one column wide)


# ---------------- one tree, many ends; complete matrices ----------------

@pytest.mark.parametrize("shape", [(130, 1), (1, 130)])
@pytest.mark.parametrize("greedy", [1, 0])
def test_one_tree_many_ends(shape, greedy):
    for strategy in STRATEGIES:
        st = _run(_matrix("full %dx%d" % shape, _full(*shape)), greedy=greedy, strategy=strategy)
        assert st["size"] == 1


@pytest.mark.parametrize("shape", [(64, 64), (65, 63)])
def test_complete_without_greedy(shape):
    key = _matrix("full %dx%d" % shape, _full(*shape))
    for strategy in STRATEGIES:
        st = _run(key, greedy=0, strategy=strategy)
        print("K%s strategy %d: %d phases" % (shape, strategy, st["phases"]))
        assert st["size"] == min(shape) and st["augmentations"] == min(shape)


# ---------------- every forced strategy ----------------

def _ladder():
    """columns whose lengths straddle wave_min_row = 4 and block_min_row = 9 by -1, 0 and +1, and one column of 3000 entries"""
    lengths = [3, 4, 5, 8, 9, 10, 3000]
    rng = np.random.default_rng(5)
    rows, r, c = 3000, [], []
    for col, n in enumerate(lengths):
        r.append(rng.choice(rows, n, replace=False) if n < rows else np.arange(rows))
        c.append(np.full(n, col))
    return k.from_pairs((rows, len(lengths)), np.concatenate(r), np.concatenate(c))


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("greedy", [1, 0])
def test_strategies(strategy, greedy):
    key = _matrix("ladder", _ladder)
    st = _run(key, greedy=greedy, strategy=strategy, wave_min_row=4, block_min_row=9, instrument=True)
    if strategy != ga.BIPARTITE_AUTO:
        # (a workgroup lists 64 long columns per level: the ones beyond are a wave's)
        others = [n for i, n in enumerate(st["regime_columns"]) if i != strategy - 1 and not (strategy == ga.BIPARTITE_BLOCK and i == 1)]
        assert st["regime_columns"][strategy - 1] > 0 and not any(others), st
    elif not greedy:  # (every column is a root: 3 is a lane's, 4, 5 and 8 a wave's, 9, 10 and 3000 a workgroup's)
        assert st["regime_columns"][0] >= 1 and st["regime_columns"][1] >= 3 and st["regime_columns"][2] >= 3, st
    # the transpose of it: one row of 3000 entries, walked by the search from the unmatched rows
    st = _run(_matrix("ladder T", lambda: k.transpose(_MATRICES[key])), greedy=greedy, strategy=strategy, wave_min_row=4, block_min_row=9)
    # the default thresholds: the long column alone is a workgroup's
    st = _run(key, greedy=greedy, strategy=strategy)
    if strategy == ga.BIPARTITE_AUTO and not greedy:
        assert st["regime_columns"][2] >= 1, st  # (16 and 2048: the long column alone is a workgroup's)


# ---------------- the literals and the goldens ----------------

@pytest.mark.parametrize("greedy", [1, 0])
def test_literals(greedy):
    st = _run(_matrix("literal", _pairs((5, 5), LITERAL)), greedy=greedy)
    assert st["size"] == 4
    ref = _reference("literal")
    assert ref["row_part"].tolist() == [0, 1, 1, 2, 2] and ref["col_part"].tolist() == [0, 0, 1, 1, 2] and ref["blocks"] == 1
    _run(_matrix("literal split", _pairs((5, 5), [p for p in LITERAL if p != (2, 2)])), greedy=greedy)
    assert _reference("literal split")["blocks"] == 2 and _reference("literal split")["row_block"].tolist() == [-1, 1, 2, -1, -1]
    got = ga.gunrock_dulmage_mendelsohn(_MATRICES["literal"])
    assert got["row_block"].tolist() == [-1, 1, 1, -1, -1] and got["col_block"].tolist() == [-1, -1, 1, 1, -1] and got["blocks"] == 1
    assert got["row_cover"].tolist() == [1, 1, 1, 0, 0] and got["col_cover"].tolist() == [0, 0, 0, 0, 1] and got["part_sizes"] == [1, 2, 2, 2, 2, 1]


def _golden(golden_dir, name):
    return _matrix(name, lambda: k.read_pattern(os.path.join(golden_dir, name + ".mtx")))


@pytest.mark.parametrize("greedy", [1, 0])
def test_goldens(golden_dir, greedy):
    st = _run(_golden(golden_dir, "chesapeake"), greedy=greedy)
    assert st["size"] == 39 and _reference("chesapeake")["blocks"] == 1
    bips = _golden(golden_dir, "bips98_606")
    for schedule in (ga.BIPARTITE_SCHEDULE_AUTO, ga.BIPARTITE_ROUNDS):
        st = _run(bips, greedy=greedy, schedule=schedule)
        assert st["size"] == 7135 and _reference(bips)["blocks"] == 1299
    st = _run(_matrix("bips rows", lambda: k.take_rows(_MATRICES[bips], 5000)), greedy=greedy)
    assert st["size"] == 5000
    st = _run(_matrix("bips cols", lambda: k.take_cols(_MATRICES[bips], 5000)), greedy=greedy)
    assert st["size"] == 5000
    parts = _reference("bips rows")["part_sizes"], _reference("bips cols")["part_sizes"]
    assert parts[0][0] and parts[0][1] and parts[1][1] and parts[1][2]  # all three parts between the two


def test_one_shots(golden_dir):
    key = _golden(golden_dir, "chesapeake")
    shape, ro, ci = _MATRICES[key]
    ref = _reference(key)
    got = ga.gunrock_bipartite_matching((ro, ci))  # (square: the shape may be left out)
    assert sorted(got) == ["mate_col", "mate_row", "size"] and k.validate(_MATRICES[key], got["mate_row"], got["mate_col"]) == got["size"] == 39
    assert ga.gunrock_structural_rank((shape, ro, ci)) == 39
    tall = _matrix("full 130x1", _full(130, 1))
    assert ga.gunrock_structural_rank(_MATRICES[tall]) == 1
    row_cover, col_cover = ga.gunrock_vertex_cover(_MATRICES[tall])
    assert np.array_equal(row_cover, _reference(tall)["row_cover"]) and col_cover.tolist() == [1]
    coarse = ga.gunrock_dulmage_mendelsohn((shape, ro, ci), fine=False)
    assert "row_block" not in coarse and np.array_equal(coarse["row_part"], ref["row_part"])


# ---------------- warm starts ----------------

def test_warm_start(golden_dir):
    key = _golden(golden_dir, "bips98_606")
    (rows, cols), ro, ci = _MATRICES[key]
    a = sp.csr_matrix((np.ones(len(ci), np.int8), ci.copy(), ro.copy()), shape=(rows, cols))
    full = maximum_bipartite_matching(a, perm_type="column").astype(np.int32)
    for greedy in (0, 1):
        st = _run(key, start=full, greedy=greedy)
        assert (st["phases"], st["augmentations"], st["greedy_pairs"]) == (1, 0, 0), st
    partial = full.copy()
    partial[::3] = -1
    st = _run(key, start=partial, greedy=0)
    assert st["augmentations"] == int((partial < 0).sum()) and st["greedy_pairs"] == 0
    st = _run(key, start=partial, greedy=1)
    assert st["augmentations"] + st["greedy_pairs"] == int((partial < 0).sum())


def test_warm_start_refused():
    key = _matrix("literal", _pairs((5, 5), LITERAL))
    p = _problem(key)
    try:
        for bad in ([-1, -1, -1, -1, 0],   # (4, 0) is no entry
                    [-1, -1, -1, 4, 4],    # column 4 twice
                    [5, -1, -1, -1, -1],   # out of range
                    [-2, -1, -1, -1, -1]):
            with pytest.raises(ValueError):
                p.reset(np.array(bad, np.int32))
        with pytest.raises(ValueError):
            p.reset(np.array([-1, -1, -1], np.int32))  # a wrong length
        # a refused start leaves the empty matching: the run is as good as any
        p.enact()
        _compare(p, key, "after refused starts")
        p.reset(np.array([0, 2, 3, 4, -1], np.int32))
        p.set_option("greedy", 0)
        p.enact()
        st = _compare(p, key, "a maximum start")
        assert (st["phases"], st["augmentations"]) == (1, 0)
    finally:
        p.close()


# ---------------- capped runs, handle reuse ----------------

def test_max_phases():
    kk = 40
    key = _chain(kk)
    # the first phase flips the one path; only a second one, which the cap forbids, could tell that nothing is left
    start = np.array(list(range(1, kk + 1)) + [-1], np.int32)
    p = _problem(key)
    try:
        p.set_option("greedy", 0)
        p.set_option("max_phases", 1)
        p.reset(start)
        p.enact()
        st = p.stats()
        assert st["state"] == ga.BIPARTITE_CAPPED and st["phases"] == 1 and st["certificate"][0] == 0, st
        m = p.extract_matching()
        assert k.validate(_MATRICES[key], m["mate_row"], m["mate_col"]) == m["size"] == st["size"] == kk + 1
        for call in (p.extract_parts, p.extract_cover, p.blocks, p.square_graph):
            with pytest.raises(ga.BipartiteNotMaximum):
                call()
        res = p.device_results()
        assert res["mate_row"] and res["mate_col"] and not res["row_part"] and not res["row_cover"]
        # a cap that is not reached: the same handle goes on to the certified end
        p.set_option("max_phases", 2)
        p.reset(start)
        p.enact()
        _compare(p, key, "max_phases 2")
        # a capped run from nothing on a complete matrix: valid, smaller than maximum or not known to be
        full = _matrix("full 64x64", _full(64, 64))
    finally:
        p.close()
    p = _problem(full)
    try:
        p.set_option("greedy", 0)
        p.set_option("strategy", ga.BIPARTITE_LANE)
        p.set_option("max_phases", 1)
        p.enact()
        st = p.stats()
        m = p.extract_matching()
        assert st["state"] == ga.BIPARTITE_CAPPED and 1 <= k.validate(_MATRICES[full], m["mate_row"], m["mate_col"]) == st["size"] <= 64
    finally:
        p.close()


def test_handle_reuse(golden_dir):
    key = _golden(golden_dir, "chesapeake")
    p = _problem(key, instrument=True)
    try:
        for options in ({"greedy": 1, "schedule": ga.BIPARTITE_SCHEDULE_AUTO, "strategy": ga.BIPARTITE_AUTO},
                        {"greedy": 0, "schedule": ga.BIPARTITE_ROUNDS, "strategy": ga.BIPARTITE_WAVE, "wave_min_row": 2},
                        {"greedy": 0, "schedule": ga.BIPARTITE_DEVICE_LOOP, "strategy": ga.BIPARTITE_BLOCK}):
            for name, value in options.items():
                assert p.set_option(name, value) == 0
            p.reset()
            p.enact()
            st = _compare(p, key, "reuse " + str(options))
            assert st["kernel_ms"] > 0 and abs(sum(st[x] for x in ("roots_ms", "level_ms", "loop_ms", "augment_ms", "rest_ms")) - st["kernel_ms"]) < 1e-6
        p.enact()  # without a reset: from the empty matching
        _compare(p, key, "enact without reset")
    finally:
        p.close()


# ---------------- device paths ----------------

def test_device_paths():
    import torch
    from gunrockinst_amd import devgraph
    key = _matrix("random 300x340", lambda: k.from_pairs((300, 340), np.random.default_rng(9).integers(0, 300, 900),
                                                    np.random.default_rng(10).integers(0, 340, 900)))
    (rows, cols), ro, ci = _MATRICES[key]
    d_ro, d_ci = torch.from_numpy(ro).cuda(), torch.from_numpy(ci).cuda()
    p = ga.BipartiteProblem().init_device((rows, cols), len(ci), d_ro.data_ptr(), d_ci.data_ptr())
    try:
        p.enact()
        _compare(p, key, "init_device")
        res = p.device_results()
        m, (row_part, col_part, _), (row_cover, col_cover) = p.extract_matching(), p.extract_parts(), p.extract_cover()
        host = {"mate_row": m["mate_row"], "mate_col": m["mate_col"], "row_part": row_part, "col_part": col_part, "row_cover": row_cover,
                "col_cover": col_cover}
        for name, want in host.items():
            got = devgraph.as_tensor(res[name], len(want), "|u1" if want.dtype == np.uint8 else "<i4")
            assert np.array_equal(got.cpu().numpy(), want), name
        k_, arcs, s_ro, s_ci, s_rows = p.square_graph()
        assert k_ == _reference(key)["part_sizes"][1] and (k_ == 0 or (s_ro and s_ci and s_rows and arcs >= k_))
        if k_:  # the map local -> row: the square rows in ascending order
            assert np.array_equal(devgraph.as_tensor(s_rows, k_).cpu().numpy(), np.flatnonzero(row_part == ga.BIPARTITE_SQUARE))
    finally:
        p.close()


# ---------------- refusals ----------------

def test_refusals():
    ro, ci = np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32)
    for bad_ro, bad_ci, shape in ((np.array([0, 2, 1], np.int32), ci, (2, 2)),      # offsets fall
                                  (np.array([0, 2, 4], np.int32), ci, (2, 2)),      # offsets beyond the entries
                                  (ro, np.array([0, 2, 1], np.int32), (2, 2)),      # a column out of range
                                  (ro, np.array([0, -1, 1], np.int32), (2, 2))):
        p = ga.BipartiteProblem()
        with pytest.raises(RuntimeError, match="code -2"):
            p.init(shape, bad_ro, bad_ci)
        with pytest.raises(RuntimeError, match="code -3"):  # the handle has been given a matrix
            p.init((2, 2), ro, ci)
        p.close()
    p = ga.BipartiteProblem()
    for call in (p.enact, p.reset, p.extract_matching, p.extract_parts, p.extract_cover, p.square_graph):
        with pytest.raises(RuntimeError, match=NOT_READY):
            call()
    assert not any(p.device_results().values())
    p.init((2, 2), ro, ci)
    with pytest.raises(RuntimeError, match="code -3"):
        p.init((2, 2), ro, ci)
    for call in (p.extract_matching, p.extract_parts, p.extract_cover, p.square_graph):  # no enact yet
        with pytest.raises(RuntimeError, match=NOT_READY):
            call()
    assert p.set_option("no such option", 1) == 1
    for name, value in (("strategy", 4), ("greedy", 2), ("max_phases", -1), ("schedule", 3), ("wave_min_row", 0), ("block_min_row", 0)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    with pytest.raises(ValueError):
        ga.BipartiteProblem().init((2, 2), np.array([0, 1], np.int32), np.array([0], np.int32))  # offsets of another shape
    p.enact()
    assert p.stats()["size"] == 2
    p.close()
