"""Random walks on the GPU (grx_rw_*): `walks`, `lengths`, `visits`, `steps` and the counters of the biased steps must equal
tests/_rw_checker.py bit for bit (tests/test_rw_cpu.py holds its two forms against each other), and must not move under anything
that is not the definition: the strategy, the grid, the order of the entries within a row, host or device input."""
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _rw_checker as k

pytestmark = pytest.mark.gpu

STRATEGIES = (ga.RW_AUTO, ga.RW_LANE, ga.RW_TILE)
NOT_READY = "code 600"  # hipErrorNotReady
DEFAULTS = {"strategy": ga.RW_AUTO, "seed": 0, "weighted": 0, "bias_return": 1, "bias_in": 1, "bias_out": 1, "tries": 32, "visits": 1}
COUNTERS = ("steps", "ended_early", "biased_tries", "forced_fallbacks")


def _run(p, starts, length, grid=0, strategy=ga.RW_AUTO, seed=0, weighted=False, bias=(1, 1, 1), tries=32, visits=True):
    options = {"strategy": strategy, "length": length, "seed": seed, "weighted": int(weighted), "bias_return": bias[0], "bias_in": bias[1],
               "bias_out": bias[2], "tries": tries, "visits": int(visits)}
    for key, value in options.items():
        assert p.set_option(key, value) == 0, key
    p.reset(starts)
    p.enact(grid)
    walks, lengths, vis, steps = p.extract(visits=visits)
    st = p.stats()
    assert walks.dtype == np.int32 and lengths.dtype == np.int32 and walks.shape == (len(starts), length + 1)
    assert st["steps"] == steps and st["walks"] == len(starts) and st["kernel_launches"] == 1 + int(visits)
    return {"walks": walks.copy(), "lengths": lengths.copy(), "visits": None if vis is None else vis.copy(), "steps": steps,
            "ended_early": st["ended_early"], "biased_tries": st["biased_tries"], "forced_fallbacks": st["forced_fallbacks"]}


def _same(got, want, what=""):
    bad = np.flatnonzero((got["walks"] != want["walks"]).any(axis=1))
    assert bad.shape[0] == 0, "%s: walks differ in rows %s: %s against %s" % (what, bad[:5], got["walks"][bad[:1]], want["walks"][bad[:1]])
    assert np.array_equal(got["lengths"], want["lengths"]), what
    if got["visits"] is not None:
        assert got["visits"].dtype == np.int64 and np.array_equal(got["visits"], want["visits"]), what
    for key in COUNTERS:
        assert got[key] == want[key], (what, key, got[key], want[key])


def _check(n, ro, ci, starts, length, weights=None, what="", strategies=STRATEGIES, grids=(0,), p=None, **kw):
    """every strategy and grid against the vectorised form of the checker"""
    want = k.vectorised(n, ro, ci, starts, length, weights=weights, **kw)
    own = p is None
    if own:
        p = ga.RwProblem().init(n, ro, ci, weights)
    for strategy in strategies:
        for grid in grids:
            _same(_run(p, starts, length, grid=grid, strategy=strategy, weighted=weights is not None, **kw), want,
                  "%s strategy %d grid %d %s" % (what, strategy, grid, kw))
    if own:
        p.close()
    return want


MODES = {"uniform": (False, {}), "weighted": (True, {}), "biased": (False, {"bias": (1, 4, 1)}), "weighted+biased": (True, {"bias": (5, 0, 2), "tries": 3})}


# ---------------- golden graphs ----------------

@pytest.mark.parametrize("graph", ["chesapeake", "bips98_606"])
def test_golden(golden_dir, graph):
    g = o.build_market(os.path.join(golden_dir, graph + ".mtx"), undirected=True)
    n, ro, ci = g.nodes, np.asarray(g.row_offsets), np.asarray(g.col_indices)
    w = k.row_col_weights(ro, ci)
    starts = np.arange(n) if n <= 300 else np.random.default_rng(1).integers(0, n, 300)
    p = ga.RwProblem().init(n, ro, ci, w)
    steps = 0
    for mode, (weighted, kw) in MODES.items():
        steps += _check(n, ro, ci, starts, 20, weights=w if weighted else None, what=graph + " " + mode, p=p, seed=11, **kw)["steps"]
    p.close()
    assert steps > 0
    if graph == "chesapeake":  # the scalar form, and the one-shot
        want = k.scalar(n, ro, ci, starts, 20, weights=w, seed=11, bias=(5, 0, 2), tries=3)
        walks, lengths, visits = ga.gunrock_random_walks(n, ro, ci, starts, 20, weights=w, seed=11, bias=(5, 0, 2), tries=3, visits=True)
        assert np.array_equal(walks, want["walks"]) and np.array_equal(lengths, want["lengths"]) and np.array_equal(visits, want["visits"])
        walks, lengths = ga.gunrock_random_walks(n, ro, ci, starts, 5)
        assert np.array_equal(walks, k.scalar(n, ro, ci, starts, 5)["walks"])


# ---------------- tile and wave borders ----------------

@pytest.fixture(scope="module")
def gnp300():
    n, ro, ci = k.gnp(300, 0.03, 42)
    return n, ro, ci, k.row_col_weights(ro, ci)


@pytest.mark.parametrize("columns", [1, 2, 15, 16, 17, 32, 33, 49])
def test_tile_and_wave_borders(gnp300, columns):
    from gunrockinst_amd import devgraph
    n, ro, ci, w = gnp300
    length = columns - 1
    p = ga.RwProblem().init(n, ro, ci, w)
    for num_walks in (1, 63, 64, 65, 257):
        starts = (np.arange(num_walks) * 7 + 3) % n
        want = k.vectorised(n, ro, ci, starts, length, seed=columns, bias=(2, 1, 3))
        for strategy in (ga.RW_LANE, ga.RW_TILE):
            got = _run(p, starts, length, strategy=strategy, seed=columns, bias=(2, 1, 3))
            _same(got, want, "columns %d walks %d strategy %d" % (columns, num_walks, strategy))
            d = p.device_results()
            assert d["pitch"] == (columns + 15) // 16 * 16 and d["pitch"] % 16 == 0
            rows = devgraph.as_tensor(d["walks"], num_walks * d["pitch"], "<i4").cpu().numpy().reshape(num_walks, d["pitch"])
            assert np.array_equal(rows[:, :columns], want["walks"])
            assert np.array_equal(devgraph.as_tensor(d["lengths"], num_walks, "<i4").cpu().numpy(), want["lengths"])
            assert np.array_equal(devgraph.as_tensor(d["visits"], n, "<i8").cpu().numpy(), want["visits"])
    p.close()


def test_padding_is_never_written(gnp300):
    """the entries of a device row behind length + 1 belong to nobody: a poisoned buffer keeps its poison there"""
    import torch
    from gunrockinst_amd import devgraph
    n, ro, ci, w = gnp300
    p = ga.RwProblem().init(n, ro, ci)
    starts = np.arange(130) % n
    _run(p, starts, 40, strategy=ga.RW_TILE)  # allocates 130 x 48
    d = p.device_results()
    devgraph.as_tensor(d["walks"], 130 * 48, "<i4").fill_(-77)
    torch.cuda.synchronize()
    for strategy, length in ((ga.RW_TILE, 40), (ga.RW_LANE, 36), (ga.RW_TILE, 33)):
        got = _run(p, starts, length, strategy=strategy)
        d = p.device_results()
        assert d["pitch"] == 48
        rows = devgraph.as_tensor(d["walks"], 130 * 48, "<i4").cpu().numpy().reshape(130, 48)
        assert np.array_equal(rows[:, :length + 1], got["walks"]) and np.all(rows[:, 41:] == -77)
    p.close()


# ---------------- ends inside a tile ----------------

def test_rows_end_at_every_offset_of_a_tile():
    n, ro, ci = k.directed_path(40)
    want = _check(n, ro, ci, np.arange(n), 48, what="directed path")
    assert want["lengths"].tolist() == list(range(40, 0, -1)) and want["ended_early"] == 40
    for v in range(n):
        assert want["walks"][v].tolist() == list(range(v, 40)) + [-1] * (9 + v)


def test_sinks_and_zero_total_rows():
    rng = np.random.default_rng(8)
    n, ro, ci = k.gnp(150, 0.04, 77)
    rows = np.repeat(np.arange(n), np.diff(ro))
    w = rng.integers(0, 4, ci.shape[0]).astype(np.int32)
    w[rows % 5 == 0] = 0  # rows whose weights are all zero: a weighted walk ends there, an unweighted one goes on
    keep = rows % 7 != 3  # sinks
    n, ro, ci, w = k.csr(n, rows[keep], ci[keep], w[keep])
    deg = np.diff(ro)
    assert np.any(deg == 0) and np.any((deg > 0) & (np.bincount(rows[keep], weights=w, minlength=n) == 0))
    starts = np.arange(n)
    weighted = _check(n, ro, ci, starts, 37, weights=w, what="zero totals", seed=5)
    biased = _check(n, ro, ci, starts, 37, weights=w, what="zero totals, biased", seed=5, bias=(0, 3, 1), tries=2)
    assert 0 < weighted["ended_early"] and 0 < biased["ended_early"]
    plain = _check(n, ro, ci, starts, 37, what="sinks", seed=5)
    assert plain["steps"] > weighted["steps"]


# ---------------- degrees ----------------

@pytest.fixture(scope="module")
def hub_graph():
    """rows of 1, 2, 64, 65 and 5,000 entries with duplicates and self-loops, the entries of the other rows pointing back at them"""
    rng = np.random.default_rng(3)
    n = 400
    degrees = {0: 5000, 1: 1, 2: 2, 3: 64, 4: 65}
    rows, cols = [], []
    for v in range(n):
        d = degrees.get(v, int(rng.integers(1, 6)))
        c = rng.integers(0, n, d)
        c[: d // 3] = rng.integers(0, 5, d // 3)  # back to the special rows
        if d > 1:
            c[-1] = v      # a self-loop
            c[-2] = c[0]   # a duplicate
        rows.append(np.full(d, v))
        cols.append(c)
    n, ro, ci, w = k.csr(n, np.concatenate(rows), np.concatenate(cols), rng.integers(0, 1000, sum(len(c) for c in cols)))
    return n, ro, ci, w


@pytest.mark.parametrize("mode", sorted(MODES))
def test_degrees_sorted_and_shuffled(hub_graph, mode):
    n, ro, ci, w = hub_graph
    weighted, kw = MODES[mode]
    starts = np.concatenate([np.arange(5).repeat(20), np.arange(n)])
    ro64, sci, sw = k.sorted_copy(n, ro, ci, w)
    sci, sw = sci.astype(np.int32), sw.astype(np.int32)
    ci2, w2 = k.shuffled_rows(ro, ci, w, np.random.default_rng(4))
    assert not np.array_equal(sci, ci) and not np.array_equal(ci2, ci)
    want = _check(n, ro, ci, starts, 18, weights=w if weighted else None, what="as built", seed=9, **kw)
    for name, (c, x) in {"sorted": (sci, sw), "shuffled": (ci2, w2)}.items():
        p = ga.RwProblem().init(n, ro, c, x if weighted else None)
        for strategy in (ga.RW_LANE, ga.RW_TILE):
            _same(_run(p, starts, 18, strategy=strategy, seed=9, weighted=weighted, **kw), want, name)
        p.close()


def test_weights_that_need_the_high_word():
    big = 2 ** 31 - 1
    n, ro, ci, w = k.csr(4, [0, 0, 0, 1, 2, 3, 3], [1, 2, 3, 0, 0, 0, 0], [big, big, big, 1, big, 0, big])
    starts = np.zeros(200, dtype=np.int32)
    want = _check(n, ro, ci, starts, 9, weights=w, what="2^31 - 1", seed=1)
    same(want, k.scalar(n, ro, ci, starts, 9, weights=w, seed=1))
    first = np.bincount(want["walks"][:, 1], minlength=4)
    assert first[0] == 0 and np.all(first[1:] > 30)  # the three equal weights share the 200 first steps


def same(a, b):
    for key in ("walks", "lengths", "visits") + COUNTERS:
        assert np.array_equal(a[key], b[key]), key


# ---------------- what must not change a result ----------------

def test_max_grid_size(gnp300):
    n, ro, ci, w = gnp300
    starts = np.arange(700) % n
    for weighted, kw in MODES.values():
        _check(n, ro, ci, starts, 21, weights=w if weighted else None, what="grids", strategies=(ga.RW_LANE, ga.RW_TILE), grids=(1, 2, 0), seed=3, **kw)


@pytest.mark.parametrize("tries", [1, 2, 32])
def test_tries_and_forced_fallbacks(tries):
    n, ro, ci = k.gnp(120, 0.08, 6, directed=False)  # symmetric: triangles give in-neighbours, the rest is out
    starts = np.arange(n)
    want = _check(n, ro, ci, starts, 25, what="tries", seed=tries, bias=(1, 50, 1), tries=tries)
    biased_steps = want["steps"] - int((want["lengths"] >= 2).sum())  # every step but the first of a walk
    assert 0 < biased_steps <= want["biased_tries"] <= tries * biased_steps
    assert want["forced_fallbacks"] <= biased_steps
    if tries <= 2:
        assert want["forced_fallbacks"] > 0  # 49 of 50 draws refuse a candidate of bias 1
    else:
        assert want["forced_fallbacks"] < biased_steps


def test_init_device_against_init(gnp300):
    import torch
    n, ro, ci, w = gnp300
    ci2, w2 = k.shuffled_rows(ro, ci, w, np.random.default_rng(1))
    d_ro, d_ci, d_w = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (ro, ci2, w2))
    starts = np.arange(n)
    for weights, d_weights in ((None, None), (w2, d_w.data_ptr())):
        p = ga.RwProblem().init_device(n, ci2.shape[0], d_ro.data_ptr(), d_ci.data_ptr(), d_weights)
        q = ga.RwProblem().init(n, ro, ci2, weights)
        for kw in ({}, {"bias": (3, 1, 2)}):
            a = _run(p, starts, 19, seed=2, weighted=weights is not None, **kw)
            _same(a, _run(q, starts, 19, seed=2, weighted=weights is not None, **kw), "device against host")
            _same(a, k.vectorised(n, ro, ci, starts, 19, weights=None if weights is None else w, seed=2, **kw), "device against the checker")
        p.close()
        q.close()
    assert np.array_equal(d_ci.cpu().numpy(), ci2) and np.array_equal(d_w.cpu().numpy(), w2)  # borrowed, and left as it was


def test_visits_on_and_off(gnp300):
    n, ro, ci, w = gnp300
    starts = np.arange(100)
    p = ga.RwProblem().init(n, ro, ci)
    on = _run(p, starts, 17, visits=True)
    assert np.array_equal(on["visits"], np.bincount(on["walks"][on["walks"] >= 0], minlength=n)) and p.device_results()["visits"]
    off = _run(p, starts, 17, visits=False)
    assert np.array_equal(off["walks"], on["walks"]) and p.device_results()["visits"] is None
    with pytest.raises(RuntimeError, match="code -1"):
        p.extract(visits=True)
    assert p.extract(walks=False, lengths=False)[3] == on["steps"] == int((on["lengths"] - 1).sum())
    p.close()


# ---------------- protocol ----------------

def test_protocol(gnp300):
    n, ro, ci, w = gnp300
    p = ga.RwProblem()
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.reset([0])
    p.init(n, ro, ci)
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.enact()
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.extract()
    for bad in ([n], [-1], [0, 1, n + 5], []):
        with pytest.raises(RuntimeError, match="code -1"):
            p.reset(bad)
    with pytest.raises(RuntimeError, match="code -3"):
        p.init(n, ro, ci)
    with pytest.raises(RuntimeError, match="code -1"):
        p.set_option("weighted", 1)  # Init had no weights
    assert p.set_option("weighted", 0) == 0 and p.set_option("nope", 1) == 1
    for name, value in (("strategy", 3), ("length", -1), ("length", 2 ** 24), ("seed", -1), ("seed", 2.0 ** 53), ("bias_in", 65536), ("tries", 0),
                        ("tries", 129), ("visits", 2)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    starts = np.arange(n)
    p.reset(starts)
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.extract()  # a Reset, no Enact yet
    # two seeds on one handle, and back
    first = _run(p, starts, 23, seed=1)
    second = _run(p, starts, 23, seed=2 ** 53 - 1)
    assert not np.array_equal(first["walks"], second["walks"])
    _same(second, k.vectorised(n, ro, ci, starts, 23, seed=2 ** 53 - 1), "the largest seed")
    _same(_run(p, starts, 23, seed=1), first, "back to the first seed")
    # two enacts without a reset between them
    assert p.set_option("seed", 2 ** 53 - 1) == 0
    p.enact()
    assert np.array_equal(p.extract()[0], second["walks"])
    # length = 0: the start vertices
    zero = _run(p, starts[:70], 0, strategy=ga.RW_TILE)
    assert np.array_equal(zero["walks"], starts[:70, None]) and zero["steps"] == 0 and zero["lengths"].tolist() == [1] * 70
    assert zero["ended_early"] == 0 and np.array_equal(zero["visits"], np.bincount(starts[:70], minlength=n))
    _same(_run(p, starts[:70], 0, strategy=ga.RW_LANE), zero, "length 0")
    p.close()
    for bad_ro, bad_ci, bad_w in (([0, 2, 1], [0, 1], None), ([0, 1, 2], [0, 2], None), ([0, 1, 2], [1, 0], [1, -1])):
        with pytest.raises(RuntimeError, match="code -2"):
            ga.RwProblem().init(2, np.array(bad_ro, np.int32), np.array(bad_ci, np.int32), None if bad_w is None else np.array(bad_w, np.int32))
    with pytest.raises(RuntimeError, match="code -1"):
        ga.RwProblem().init(0, np.array([0], np.int32), np.array([], np.int32))
    # a graph without an entry: every walk is its start vertex
    walks, lengths = ga.gunrock_random_walks(3, np.zeros(4, np.int32), np.array([], np.int32), [2, 0], 4)
    assert walks.tolist() == [[2, -1, -1, -1, -1], [0, -1, -1, -1, -1]] and lengths.tolist() == [1, 1]
