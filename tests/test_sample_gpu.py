"""Neighbourhood sampling on the GPU (grx_sample_*): every array bit-exact against the vectorised form of tests/_sample_checker.py, for
the strategies AUTO / LANE / GROUP and the grids 0 and 1, on the smallest shapes at which the kernels can go wrong."""
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _sample_checker as k

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_READY = "code 600"  # hipErrorNotReady
STRATEGIES = (ga.SAMPLE_AUTO, ga.SAMPLE_LANE, ga.SAMPLE_GROUP)
MODES = {"replace0": {}, "replace1": {"replace": True}, "weighted": {"replace": True, "weighted": True}}
NO_EIDS = tuple(key for key in k.KEYS if key != "eids")


def market(name, undirected):
    g = o.build_market(os.path.join(ROOT, "tests", "golden", name), undirected=undirected)
    return g.nodes, np.asarray(g.row_offsets, dtype=np.int32), np.asarray(g.col_indices, dtype=np.int32)


def sample(p, seeds, fanouts, strategy=ga.SAMPLE_AUTO, grid=0, seed=0, replace=False, weighted=False, long_row=4096, eids=True, reset=True):
    if replace:
        options = (("replace", 1), ("weighted", int(weighted)))
    else:
        options = (("weighted", 0), ("replace", 0))
    for name, value in options + (("strategy", strategy), ("seed", seed), ("long_row", long_row), ("eids", int(eids))):
        assert p.set_option(name, value) == 0, name
    p.set_fanouts(fanouts)
    if reset:
        p.reset(seeds)
    p.enact(grid)
    return p.extract(eids=eids)


def agree(got, want, keys=k.KEYS, note=""):
    for key in keys:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (key, note)


def sweep(p, n, ro, ci, seeds, fanouts, weights=None, strategies=STRATEGIES, grids=(0, 1), **kw):
    """every strategy and grid against the vectorised form; returns it"""
    want = k.vectorised(n, ro, ci, seeds, fanouts, weights=weights, **kw)
    for strategy in strategies:
        for grid in grids:
            agree(sample(p, seeds, fanouts, strategy=strategy, grid=grid, **kw), want, note=(fanouts, strategy, grid, kw))
    return want


# ---------------- goldens ----------------

def golden_cases():
    n, ro, ci = market("chesapeake.mtx", True)
    yield "chesapeake-all", (n, ro, ci, np.arange(n, dtype=np.int32))
    yield "chesapeake-few", (n, ro, ci, np.array([38, 0, 7], dtype=np.int32))
    n, ro, ci = market("bips98_606.mtx", False)
    yield "bips98_606", (n, ro, ci, np.random.default_rng(606).permutation(n)[:300].astype(np.int32))


GOLDENS = dict(golden_cases())


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_goldens(name, mode):
    n, ro, ci, seeds = GOLDENS[name]
    w = k.row_col_weights(ro, ci)
    p = ga.SampleProblem().init(n, ro, ci, w)
    for fanouts in ((5, 3), (64,), (-1, 2)):
        want = sweep(p, n, ro, ci, seeds, fanouts, weights=w, seed=7, **MODES[mode])
        assert want["cols"].shape[0] > 0
    p.close()


# ---------------- row boundaries ----------------

@pytest.mark.parametrize("f", [1, 2, 64])
def test_row_boundaries_on_a_star(f):
    for d in (f - 1, f, f + 1):
        if d < 1:
            continue
        n, ro, ci = k.star(d + 1)
        p = ga.SampleProblem().init(n, ro, ci)
        for kw in ({}, {"replace": True}):
            want = sweep(p, n, ro, ci, [0], (f, f), seed=d, **kw)
            assert want["edge_ptr"][1] == (f if kw else min(d, f))
        p.close()


@pytest.mark.parametrize("n,prob,f", [(300, 0.005, 1), (300, 0.02, 6), (400, 0.16, 64)])
def test_row_boundaries_on_gnp(n, prob, f):
    n, ro, ci = k.gnp(n, prob, 31 + f)
    deg = np.diff(ro)
    assert all((deg == d).any() for d in (f - 1, f, f + 1)), "rows of f - 1, f and f + 1 entries"
    p = ga.SampleProblem().init(n, ro, ci)
    seeds = np.random.default_rng(f).permutation(n)[:130]
    for kw in ({}, {"replace": True}):
        sweep(p, n, ro, ci, seeds, (f, 2), seed=5, **kw)
    p.close()


# ---------------- chained collisions ----------------

def naive_floyd(seed, v, hop, d, f):
    """a resolve that compares a candidate against the earlier CANDIDATES: not the definition"""
    t = [k.rk.draw(seed, v, hop, s) for s in range(f)]
    t = [((r >> 32) * (d - f + s + 1)) >> 32 for s, r in enumerate(t)]
    return [d - f + s if t[s] in t[:s] else t[s] for s in range(f)]


def test_chained_collisions():
    rng = np.random.default_rng(64)
    n = 101
    rows, cols = [], []
    for v in range(n):
        d = 65 + v % 36  # 65 .. 100
        rows += [v] * d
        cols += rng.permutation(n)[:d].tolist()
    n, ro, ci, _ = k.csr(n, rows, cols)
    assert np.diff(ro).min() == 65 and np.diff(ro).max() == 100
    # the case is one: somewhere a candidate equals an i that an earlier collision chose
    assert any(naive_floyd(9, v, 0, 65 + v % 36, 64) != k.floyd(9, v, 0, 65 + v % 36, 64) for v in range(n))
    p = ga.SampleProblem().init(n, ro, ci)
    want = sweep(p, n, ro, ci, np.arange(n), (64,), seed=9)
    assert (np.diff(want["offsets"]) == 64).all()
    for v in range(0, n, 10):
        assert np.array_equal(np.sort(np.asarray(ci)[want["eids"][64 * v:64 * v + 64]]),
                              np.sort(np.sort(np.asarray(ci)[ro[v]:ro[v + 1]])[k.floyd(9, v, 0, 65 + v % 36, 64)]))
    p.close()


# ---------------- group packing ----------------

def test_group_packing():
    n, ro, ci = k.gnp(200, 0.25, 17)
    order = np.random.default_rng(2).permutation(n)
    p = ga.SampleProblem().init(n, ro, ci)
    for f in (3, 4, 5, 8, 9, 16, 17, 33):
        for count in (1, 7, 9, 63, 65):
            for kw in ({}, {"replace": True}):
                sweep(p, n, ro, ci, order[:count], (f,), strategies=(ga.SAMPLE_LANE, ga.SAMPLE_GROUP), seed=f, **kw)
    p.close()


def test_auto_on_both_sides_of_its_seed_threshold():
    """with replacement AUTO takes LANE from 65 536 seeds on, GROUP below"""
    n = 65536 + 7
    v = np.arange(n)
    n, ro, ci, _ = k.csr(n, np.concatenate([v, v, v]), np.concatenate([(v + 1) % n, (v * 7 + 3) % n, (v + 2) % n]))
    p = ga.SampleProblem().init(n, ro, ci)
    for count in (65535, 65536):
        for kw in ({"replace": True}, {}):
            sweep(p, n, ro, ci, v[:count], (2,), strategies=(ga.SAMPLE_AUTO,), grids=(0,), seed=3, **kw)
    p.close()


# ---------------- long rows ----------------

def test_long_rows_under_the_whole_row_fanout():
    leaves = 603  # the hub's row: 75 chunks of 8 and a part of one
    n, ro, ci = k.star(leaves + 1)
    p = ga.SampleProblem().init(n, ro, ci)
    seeds = [5, 0]
    want = k.vectorised(n, ro, ci, seeds, (-1, -1))
    assert want["edge_ptr"].tolist() == [0, leaves + 1, leaves + 1 + leaves - 1]
    for strategy in STRATEGIES:
        for grid in (0, 1, 3):
            agree(sample(p, seeds, (-1, -1), strategy=strategy, grid=grid, long_row=8), want, note=(strategy, grid))
            assert p.stats()["long_rows"] == 1, "the hub went to the long-row kernel"
    agree(sample(p, seeds, (-1, -1)), want)
    assert p.stats()["long_rows"] == 0
    # a sampled hop never takes the long path
    agree(sample(p, seeds, (9, 2), long_row=8), k.vectorised(n, ro, ci, seeds, (9, 2)))
    assert p.stats()["long_rows"] == 0
    p.close()


# ---------------- deduplication ----------------

def test_deduplication_seed_ids_self_loops_and_duplicates():
    rows, cols = [0, 0, 0, 0, 1, 1, 3], [2, 0, 2, 1, 0, 3, 2]
    n, ro, ci, _ = k.csr(4, rows, cols)
    p = ga.SampleProblem().init(n, ro, ci)
    for strategy in STRATEGIES:
        r = sample(p, [3, 0], (-1, -1), strategy=strategy)
        assert r["vertices"].tolist() == [3, 0, 1, 2] and r["offsets"].tolist() == [0, 1, 5, 7, 7]
        assert r["cols"].tolist() == [3, 1, 2, 3, 3, 1, 0] and r["eids"].tolist() == [6, 1, 3, 0, 2, 4, 5]
    p.close()
    # a diamond, wide: every vertex of the middle layer leads to the same few sinks
    rows = [0] * 40 + [m for m in range(1, 41) for _ in range(3)]
    cols = list(range(1, 41)) + [41 + (m + j) % 5 for m in range(1, 41) for j in range(3)]
    n, ro, ci, _ = k.csr(46, rows, cols)
    p = ga.SampleProblem().init(n, ro, ci)
    for fanouts in ((-1, -1, 2), (30, 2, 2)):
        for kw in ({}, {"replace": True}):
            want = sweep(p, n, ro, ci, [0], fanouts, seed=3, **kw)
            assert np.unique(want["vertices"]).shape[0] == want["vertices"].shape[0] and want["vertex_ptr"][3] - want["vertex_ptr"][2] <= 5
    p.close()


# ---------------- hops ----------------

def test_hops_that_run_dry_and_sixteen_hops():
    n, ro, ci = k.rk.directed_path(20)
    p = ga.SampleProblem().init(n, ro, ci)
    want = sweep(p, n, ro, ci, [0], (1,) * 16, seed=1)
    assert want["vertex_ptr"].tolist() == list(range(18)) and want["edge_ptr"].tolist() == list(range(17))
    want = sweep(p, n, ro, ci, [15], (2, -1, 64, 1, 1, 3, 1, 1), seed=1, replace=True)
    assert want["vertex_ptr"].tolist() == [0, 1, 2, 3, 4, 5, 5, 5, 5, 5] and want["edge_ptr"][-1] == 2 + 1 + 64 + 1
    want = sweep(p, n, ro, ci, [19, 3], (3, 3), seed=1)  # an isolated seed among the seeds
    assert want["offsets"][:3].tolist() == [0, 0, 1]
    want = sweep(p, n, ro, ci, [19], (3, -1, 3), seed=1)
    assert want["vertex_ptr"].tolist() == [0, 1, 1, 1, 1] and want["edge_ptr"].tolist() == [0, 0, 0, 0] and want["offsets"].tolist() == [0, 0]
    p.close()
    n, ro, ci = k.cycle_with_tail(5, 4)
    p = ga.SampleProblem().init(n, ro, ci)
    sweep(p, n, ro, ci, [2], (2,) * 12, seed=4)
    p.close()


def test_reset_and_enact_again_on_one_handle():
    n, ro, ci = k.gnp(300, 0.03, 8)
    order = np.random.default_rng(3).permutation(n)
    first, second = order[:40], order[20:90]
    p = ga.SampleProblem().init(n, ro, ci)
    want = [k.vectorised(n, ro, ci, seeds, (4, 3, 2), seed=6) for seeds in (first, second)]
    for strategy in (ga.SAMPLE_LANE, ga.SAMPLE_GROUP):
        agree(sample(p, first, (4, 3, 2), strategy=strategy, seed=6), want[0])
        agree(sample(p, second, (4, 3, 2), strategy=strategy, seed=6), want[1])
        agree(sample(p, first, (4, 3, 2), strategy=strategy, seed=6), want[0])
        # an Enact behind an Enact, without a Reset between, and under other fanouts
        agree(sample(p, first, (2, -1), strategy=strategy, seed=6, reset=False), k.vectorised(n, ro, ci, first, (2, -1), seed=6))
        agree(sample(p, first, (4, 3, 2), strategy=strategy, seed=6, reset=False), want[0])
    p.close()


# ---------------- the input ----------------

def test_entry_order_and_init_device():
    import torch
    n, ro, ci = k.gnp(300, 0.04, 12)
    rng = np.random.default_rng(4)
    again = rng.integers(0, ci.shape[0], 200)  # duplicate entries, so that ties exist
    rows = np.repeat(np.arange(n), np.diff(ro))
    n, ro, ci, w = k.csr(n, np.concatenate([rows, rows[again]]), np.concatenate([ci, ci[again]]), rng.integers(0, 3, ci.shape[0] + 200))
    ci2, w2 = k.shuffled_rows(ro, ci, w, rng)
    seeds = rng.permutation(n)[:50]
    d_ro, d_ci, d_w = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (ro, ci2, w2))
    torch.cuda.synchronize()
    for weights, shuffled, d_weights in ((None, None, None), (w, w2, d_w.data_ptr())):
        modes = [{}, {"replace": True}] + ([{"replace": True, "weighted": True}] if weights is not None else [])
        p = ga.SampleProblem().init(n, ro, ci, weights)
        q = ga.SampleProblem().init(n, ro, ci2, shuffled)
        r = ga.SampleProblem().init_device(n, ci2.shape[0], d_ro.data_ptr(), d_ci.data_ptr(), d_weights)
        for kw in modes:
            for fanouts in ((5, 3), (-1, 2)):
                a = sample(p, seeds, fanouts, seed=2, **kw)
                b = sample(q, seeds, fanouts, seed=2, **kw)
                c = sample(r, seeds, fanouts, seed=2, **kw)
                agree(a, k.vectorised(n, ro, ci, seeds, fanouts, weights=weights, seed=2, **kw))
                agree(b, k.vectorised(n, ro, ci2, seeds, fanouts, weights=shuffled, seed=2, **kw))  # the eids by the tie rule
                agree(b, a, NO_EIDS)
                agree(c, b)
                assert np.array_equal(ci2[b["eids"]], ci[a["eids"]])
        for x in (p, q, r):
            x.close()


# ---------------- refusals ----------------

def test_refusals():
    n, ro, ci = k.gnp(100, 0.1, 5)
    w = k.row_col_weights(ro, ci)
    p = ga.SampleProblem()
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.reset([1])
    p.init(n, ro, ci)
    with pytest.raises(RuntimeError, match="code -3"):
        p.init(n, ro, ci)
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.enact()
    for seeds in ([1, 2, 1], [n], [-1], []):
        with pytest.raises(RuntimeError, match="code -1"):
            p.reset(seeds)
    p.reset([1, 2])
    with pytest.raises(RuntimeError, match=NOT_READY):  # no fanouts yet
        p.enact()
    for fanouts in ((0,), (65,), (-2,), (3, 0), (), (1,) * 17):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_fanouts(fanouts)
    assert p.set_option("nope", 1) == 1
    for name, value in (("weighted", 1), ("strategy", 3), ("seed", -1), ("seed", 2.0 ** 53), ("edge_limit", 0), ("edge_limit", 2.0 ** 31), ("long_row", 7),
                        ("eids", 2), ("replace", 2)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    assert p.set_option("replace", 1) == 0
    with pytest.raises(RuntimeError, match="code -1"):  # Init had no weights
        p.set_option("weighted", 1)
    p.close()

    p = ga.SampleProblem().init(n, ro, ci, w)
    with pytest.raises(RuntimeError, match="code -1"):  # replace 0 + weighted 1
        p.set_option("weighted", 1)
    assert p.set_option("replace", 1) == 0 and p.set_option("weighted", 1) == 0
    with pytest.raises(RuntimeError, match="code -1"):
        p.set_option("replace", 0)
    assert p.set_option("weighted", 0) == 0 and p.set_option("replace", 0) == 0
    seeds = np.arange(0, n, 3)
    want = k.vectorised(n, ro, ci, seeds, (4, 2, 2), weights=w, seed=8)
    edges = int(want["edge_ptr"][-1])
    assert want["edge_ptr"][2] < edges - 1, "the limit falls into the last hop"
    assert p.set_option("edge_limit", edges - 1) == 0
    with pytest.raises(ga.SampleTooLarge):
        sample(p, seeds, (4, 2, 2), seed=8)
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.extract()
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.sizes()
    assert p.device_results() == {"vertices": None, "offsets": None, "cols": None, "eids": None}
    assert p.set_option("edge_limit", edges) == 0
    agree(sample(p, seeds, (4, 2, 2), seed=8, reset=False), want)
    assert p.set_option("edge_limit", 1) == 0  # the first hop already
    with pytest.raises(ga.SampleTooLarge):
        sample(p, seeds, (4, 2, 2), seed=8)
    assert p.set_option("edge_limit", 2 ** 31 - 1) == 0
    agree(sample(p, seeds, (4, 2, 2), seed=8), want)
    p.close()


# ---------------- the surface ----------------

def test_without_eids_stats_and_device_results():
    from gunrockinst_amd import devgraph
    n, ro, ci = k.gnp(300, 0.05, 21)
    seeds = np.arange(5, 105)
    p = ga.SampleProblem(instrument=True).init(n, ro, ci)
    want = k.vectorised(n, ro, ci, seeds, (6, -1, 3), seed=11)
    for strategy in STRATEGIES:
        got = sample(p, seeds, (6, -1, 3), strategy=strategy, seed=11, eids=False)
        assert got["eids"] is None
        agree(got, want, NO_EIDS)
        with pytest.raises(RuntimeError, match="code -1"):
            p.extract(eids=True)
        assert p.device_results()["eids"] is None and p.device_results()["cols"]
    agree(sample(p, seeds, (6, -1, 3), seed=11), want)
    st = p.stats()
    deg = np.diff(ro)
    frontier = [want["vertices"][want["vertex_ptr"][h]:want["vertex_ptr"][h + 1]] for h in range(3)]
    assert st["rows_expanded"] == [f.shape[0] for f in frontier]
    assert st["rows_sampled"] == [int((deg[frontier[0]] > 6).sum()), 0, int((deg[frontier[2]] > 3).sum())]
    assert st["rows_copied"] == [int((deg[frontier[0]] <= 6).sum()), frontier[1].shape[0], int((deg[frontier[2]] <= 3).sum())]
    assert st["readbacks"] == 4 and st["kernel_launches"] > 0 and st["kernel_ms"] > 0 and st["build_ms"] > 0
    assert abs(st["count_ms"] + st["sample_ms"] + st["renumber_ms"] + st["relabel_ms"] - st["kernel_ms"]) < 1e-3 * st["kernel_ms"] + 1e-6
    v, e, vp, ep = p.sizes()
    assert (v, e) == (want["vertices"].shape[0], want["cols"].shape[0]) and np.array_equal(vp, want["vertex_ptr"]) and np.array_equal(ep, want["edge_ptr"])
    # the device arrays are the extracted ones
    d = p.device_results()
    assert np.array_equal(devgraph.as_tensor(d["vertices"], v, "<i4").cpu().numpy(), want["vertices"])
    assert np.array_equal(devgraph.as_tensor(d["offsets"], v + 1, "<i8").cpu().numpy(), want["offsets"])
    assert np.array_equal(devgraph.as_tensor(d["cols"], e, "<i4").cpu().numpy(), want["cols"])
    assert np.array_equal(devgraph.as_tensor(d["eids"], e, "<i4").cpu().numpy(), want["eids"])
    p.close()


def test_one_shot():
    n, ro, ci = market("chesapeake.mtx", True)
    w = k.row_col_weights(ro, ci)
    seeds = [3, 30, 12]
    got = ga.gunrock_sample_neighbors(n, ro, ci, seeds, (5, 3), seed=7)
    assert sorted(got) == sorted(k.KEYS)
    agree(got, k.vectorised(n, ro, ci, seeds, (5, 3), seed=7))
    agree(got, k.scalar(n, ro, ci, seeds, (5, 3), seed=7))
    got = ga.gunrock_sample_neighbors(n, ro, ci, seeds, (5, -1), weights=w, replace=True, seed=7)
    agree(got, k.vectorised(n, ro, ci, seeds, (5, -1), weights=w, replace=True, weighted=True, seed=7))
    with pytest.raises(RuntimeError, match="code -1"):
        ga.gunrock_sample_neighbors(n, ro, ci, seeds, (5,), weights=w)  # weighted without replacement
