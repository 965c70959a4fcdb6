"""Vertex similarity on the GPU (grx_sim_*): `common`, `num`, `den`, `ids`, `count` and `candidates` must equal tests/_sim_checker.py's
forms, int against int with np.array_equal, and `score` its float64 bit for bit; none of them may move under anything that is not the
graph, the metric and skip_neighbors: the regime, the thresholds, the scratch budget, the grid, the form the CSR comes in, host or
device queries.  Which regime took a pair or a source is asserted from stats against the checker's degrees and Wd and a restatement
of the rule."""
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _c4_checker as ck
import _sim_checker as k
from _tc_checker import simple_edges

pytestmark = pytest.mark.gpu

STRATEGIES = (ga.SIM_AUTO, ga.SIM_LANE, ga.SIM_WAVE, ga.SIM_BLOCK, ga.SIM_GLOBAL)
METRICS = (ga.SIM_COMMON, ga.SIM_JACCARD, ga.SIM_OVERLAP, ga.SIM_SORENSEN)
NOT_READY = "code 600"  # hipErrorNotReady
LOW = {"lane_max": 8, "table_slots": 64, "block_slots": 256}  # the borders at d(u) + d(v) = 8 and at Wd = 32 and 128
DEFAULTS = {"metric": ga.SIM_JACCARD, "strategy": ga.SIM_AUTO, "skip_neighbors": 0, "lane_max": 64, "table_slots": 1024, "block_slots": 8192,
            "scratch_mib": 1024}
PAIR_KEYS = ("common", "num", "den", "score")
TOPK_KEYS = ("ids", "common", "num", "den", "score", "count", "candidates")


def _set(p, options):
    for key, value in {**DEFAULTS, **options}.items():
        assert p.set_option(key, value) == 0, key


def _pairs(p, u, v, grid=0, **options):
    _set(p, options)
    p.pairs(u, v, grid)
    got = p.extract_pairs()
    assert got["common"].dtype == np.int32 and got["num"].dtype == np.int64 and got["score"].dtype == np.float64
    return got, p.stats()


def _topk(p, sources, kk, grid=0, **options):
    _set(p, options)
    p.topk(sources, kk, grid)
    got = p.extract_topk()
    assert got["ids"].dtype == np.int32 and got["den"].dtype == np.int64 and got["ids"].shape == (len(sources), kk)
    return got, p.stats()


def _pair_stats(st, ref, u, v, **options):
    rule = {key: value for key, value in options.items() if key in ("strategy", "lane_max")}
    d = np.asarray(ref.d if hasattr(ref, "d") else [len(x) for x in ref.N])
    regimes = [k.pair_regime(int(d[x]) + int(d[y]), **rule) for x, y in zip(u, v)]
    assert (st["lane_pairs"], st["wave_pairs"]) == (regimes.count(k.LANE), regimes.count(k.WAVE)), (st, options)


def _topk_stats(st, ref, sources, got, **options):
    rule = {key: value for key, value in options.items() if key in ("strategy", "table_slots", "block_slots")}
    wd = [int(ref.wd[s]) for s in sources]
    regimes = [k.topk_regime(w, **rule) for w in wd]
    for r, name in ((k.WAVE, "wave"), (k.BLOCK, "block"), (k.GLOBAL, "global")):
        assert st[name + "_sources"] == regimes.count(r), (name, st, options)
        assert st[name + "_wedges"] == sum(w for w, x in zip(wd, regimes) if x == r), (name, st, options)
    assert st["wedges_walked"] == sum(wd) and st["candidates"] == int(got["candidates"].sum()) and st["wedges"] == int(ref.wd.sum())


def _mtx(golden_dir, name):
    g = o.build_market(os.path.join(golden_dir, name + ".mtx"), undirected=True)
    return g.nodes, g.row_offsets, g.col_indices


# ---------------- golden graphs ----------------

@pytest.mark.parametrize("name", ["chesapeake", "test_bc", "bips98_606"])
def test_goldens(golden_dir, name):
    n, ro, ci = _mtx(golden_dir, name)
    ref = k.Sets(n, ro, ci)
    rng = np.random.default_rng(5)
    a, b = simple_edges(n, ro, ci)
    u = np.concatenate([a, rng.integers(0, n, 300), np.arange(min(n, 64))])
    v = np.concatenate([b, rng.integers(0, n, 300), np.arange(min(n, 64))])
    sources = np.arange(n) if n < 200 else np.concatenate([np.argsort(ref.wd)[-40:], rng.integers(0, n, 160)])
    p = ga.SimProblem().init(n, ro, ci)
    for metric in METRICS:
        got, st = _pairs(p, u, v, metric=metric)
        assert k.same(got, ref.pairs(u, v, metric)) is None, metric
        _pair_stats(st, ref, u, v)
        for skip in (0, 1):
            got, st = _topk(p, sources, 16, metric=metric, skip_neighbors=skip)
            assert k.same(got, ref.topk(sources, 16, metric, bool(skip))) is None, (metric, skip)
            _topk_stats(st, ref, sources, got)
    assert st["simple_edges"] == a.shape[0]
    p.close()
    if name == "chesapeake":
        want = k.Dense(n, ro, ci)
        assert k.same(ga.gunrock_similarity(ro, ci, u, v, metric=ga.SIM_OVERLAP), want.pairs(u, v, k.OVERLAP)) is None
        assert k.same(ga.gunrock_similar_vertices(ro, ci, sources, 5, skip_neighbors=True), want.topk(sources, 5, k.JACCARD, True)) is None


# ---------------- pair mode ----------------

def _rows_graph():
    """hubs of degree exactly 0, 1, 4, 5, 63, 64, 65 (twice each) over 70 base vertices that also carry a sparse graph of their own"""
    rng = np.random.default_rng(11)
    base = 70
    r, c = np.nonzero(np.triu(rng.random((base, base)) < 0.08, 1))
    rows, cols, hubs, at = [r], [c], {}, base
    for m in (0, 1, 4, 5, 63, 64, 65):
        for shift in (0, 3):
            hubs.setdefault(m, []).append(at)
            rows.append(np.full(m, at, np.int64))
            cols.append((shift + np.arange(m)) % base)
            at += 1
    return (at, np.concatenate(rows), np.concatenate(cols)), hubs


@pytest.fixture(scope="module")
def rows_case():
    graph, hubs = _rows_graph()
    n, ro, ci = ck.mirrored(graph)
    ref = k.Dense(n, ro, ci)
    assert all(int(ref.d[h]) == m for m, hs in hubs.items() for h in hs)
    ids = [h for hs in hubs.values() for h in hs]
    u = np.array([x for x in ids for _ in ids] + ids + [0, 1, 2, 2, 2] + list(range(70)), dtype=np.int32)
    v = np.array([y for _ in ids for y in ids] + [7] * len(ids) + [1, 0, 2, 5, 5] + list(range(70))[::-1], dtype=np.int32)
    return graph, n, ro, ci, ref, hubs, u, v


def test_pair_rows_regimes_and_grids(rows_case):
    _, n, ro, ci, ref, hubs, u, v = rows_case
    p = ga.SimProblem().init(n, ro, ci)
    wants = {metric: ref.pairs(u, v, metric) for metric in METRICS}
    assert wants[k.JACCARD]["den"].min() == 0 and (wants[k.COMMON]["common"][u == v] == ref.d[u[u == v]]).all()  # isolated ends; u == v
    for options in ({}, LOW):
        for strategy in STRATEGIES:
            for grid in (0, 1):
                got, st = _pairs(p, u, v, grid, strategy=strategy, **options)
                assert k.same(got, wants[k.JACCARD]) is None, (options, strategy, grid)
                _pair_stats(st, ref, u, v, strategy=strategy, **options)
    for metric in METRICS:
        assert k.same(_pairs(p, u, v, 3, metric=metric, **LOW)[0], wants[metric]) is None, metric
    # d(u) + d(v) at lane_max and one beyond
    (h4, h4b), (h5, _) = hubs[4], hubs[5]
    _, st = _pairs(p, [h4, h4], [h4b, h5], **LOW)
    assert (st["lane_pairs"], st["wave_pairs"]) == (1, 1)
    p.close()


@pytest.mark.parametrize("count", [0, 1, 64, 65])
def test_pair_counts_host_and_device(rows_case, count):
    import torch
    _, n, ro, ci, ref, _, u, v = rows_case
    u, v = u[:count], v[:count]
    want = ref.pairs(u, v, k.SORENSEN)
    p = ga.SimProblem().init(n, ro, ci)
    got, _ = _pairs(p, u, v, metric=ga.SIM_SORENSEN)
    assert k.same(got, want) is None and got["common"].shape == (count,)
    d_u, d_v = (torch.as_tensor(x, dtype=torch.int32, device="cuda") for x in (u, v))
    _set(p, {"metric": ga.SIM_SORENSEN, "strategy": ga.SIM_WAVE})
    p.reset()
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.extract_pairs()
    p.pairs_device(count, d_u.data_ptr() if count else 0, d_v.data_ptr() if count else 0)
    assert k.same(p.extract_pairs(), want) is None
    if count:
        from gunrockinst_amd import devgraph
        d = p.device_results()
        assert np.array_equal(devgraph.as_tensor(d["pair_common"], count, "<i4").cpu().numpy(), want["common"])
        assert np.array_equal(devgraph.as_tensor(d["pair_num"], count, "<i8").cpu().numpy(), want["num"])
        assert np.array_equal(devgraph.as_tensor(d["pair_den"], count, "<i8").cpu().numpy(), want["den"])
    p.close()


def test_csr_forms_give_one_result(rows_case):
    graph, n, _, _, ref, _, u, v = rows_case
    want_pairs, sources = ref.pairs(u, v, k.JACCARD), np.arange(n)
    want_topk = ref.topk(sources, 7, k.JACCARD)
    for form, (ro, ci) in ck.entry_forms(graph, np.random.default_rng(3)).items():
        p = ga.SimProblem().init(n, ro, ci)
        assert k.same(_pairs(p, u, v, **LOW)[0], want_pairs) is None, form
        assert k.same(_topk(p, sources, 7, **LOW)[0], want_topk) is None, form
        p.close()


def test_bad_ids_leave_the_handle_usable(rows_case):
    _, n, ro, ci, ref, _, u, v = rows_case
    p = ga.SimProblem().init(n, ro, ci)
    want = ref.pairs(u, v, k.JACCARD)
    assert k.same(_pairs(p, u, v)[0], want) is None
    for bad in (n, -1, 2 ** 31 - 1):
        wrong = v.copy()
        wrong[-1] = bad
        with pytest.raises(RuntimeError, match="code -1"):
            p.pairs(u, wrong)
        with pytest.raises(RuntimeError, match=NOT_READY):  # no result was written
            p.extract_pairs()
        with pytest.raises(RuntimeError, match="code -1"):
            p.topk([0, bad], 4)
        with pytest.raises(RuntimeError, match=NOT_READY):
            p.extract_topk()
        assert k.same(_pairs(p, u, v)[0], want) is None
    for kk in (0, 65):
        with pytest.raises(RuntimeError, match="code -1"):
            p.topk([0], kk)
    # beyond int32 offsets: refused from the counts alone, in front of any read of the arrays
    from gunrockinst_amd import capi
    one = np.zeros(1, dtype=np.int32)
    assert capi.lib().grx_sim_pairs(p._h, 2 ** 31, capi._p(one), capi._p(one), 0, None) == ga.SIM_TOO_LARGE
    assert capi.lib().grx_sim_topk(p._h, 2 ** 25, capi._p(one), 64, 0, None) == ga.SIM_TOO_LARGE
    assert capi.lib().grx_sim_topk(p._h, 2 ** 31, capi._p(one), 1, 0, None) == ga.SIM_TOO_LARGE
    assert k.same(_topk(p, [0, 1], 4)[0], ref.topk([0, 1], 4, k.JACCARD)) is None
    p.close()


# ---------------- top-k mode ----------------

@pytest.fixture(scope="module")
def borders_case():
    """stars whose leaves have Wd = 32, 33, 128 and 129 -- the borders of LOW and one beyond -- next to a G(n, p) with triangles"""
    rng = np.random.default_rng(17)
    r, c = np.nonzero(np.triu(rng.random((180, 180)) < 0.06, 1))
    graph = ck.union(k.star(32), k.star(33), k.star(128), k.star(129), (180, r, c), ck.edgeless(2))
    n, ro, ci = ck.mirrored(graph)
    ref = k.Dense(n, ro, ci)
    assert [int(ref.wd[x]) for x in (1, 34, 68, 197)] == [32, 33, 128, 129]
    return n, ro, ci, ref


def test_topk_regime_borders_strategies_and_grids(borders_case):
    n, ro, ci, ref = borders_case
    sources = np.arange(n)
    p = ga.SimProblem().init(n, ro, ci)
    for skip in (0, 1):
        want = ref.topk(sources, 16, k.JACCARD, bool(skip))
        for options in (LOW, {}):
            for strategy in STRATEGIES:
                for grid in (0, 2):
                    got, st = _topk(p, sources, 16, grid, strategy=strategy, skip_neighbors=skip, **options)
                    assert k.same(got, want) is None, (skip, options, strategy, grid)
                    _topk_stats(st, ref, sources, got, strategy=strategy, **options)
    _, st = _topk(p, [1, 34, 68, 197], 4, **LOW)
    assert (st["wave_sources"], st["block_sources"], st["global_sources"]) == (1, 2, 1)
    for metric in METRICS:
        got, _ = _topk(p, sources, 16, metric=metric, scratch_mib=1, **LOW)
        assert k.same(got, ref.topk(sources, 16, metric)) is None, metric
    p.close()


def test_topk_k_padding_repeats_and_empty_queries():
    import torch
    graph = ck.union(k.star(64), k.star(65), k.star(66), k.star(1), k.star(2), k.star(3), ck.edgeless(1))
    n, ro, ci = ck.mirrored(graph)
    ref = k.Dense(n, ro, ci)
    leaves = [1, 66, 132, 199, 201, 204]  # a leaf of every star: 63, 64, 65 candidates (k - 1, k, k + 1 for 64), then 0, 1, 2
    assert [len(ref.candidates(x, k.JACCARD)) for x in leaves] == [63, 64, 65, 0, 1, 2]
    sources = np.array(leaves + [n - 1, 0, 1, 1, 132], dtype=np.int32)  # ... the isolated vertex, a hub, repeats
    p = ga.SimProblem().init(n, ro, ci)
    for kk in (1, 2, 64):
        want = ref.topk(sources, kk, k.JACCARD)
        for options in ({}, LOW, {"strategy": ga.SIM_GLOBAL}):
            got, _ = _topk(p, sources, kk, **options)
            assert k.same(got, want) is None, (kk, options)
        assert got["count"].tolist()[:7] == [min(kk, c) for c in (63, 64, 65, 0, 1, 2, 0)] and (got["ids"][6] == -1).all()
    d_sources = torch.as_tensor(sources, dtype=torch.int32, device="cuda")
    p.topk_device(sources.shape[0], d_sources.data_ptr(), 64)
    assert k.same(p.extract_topk(), want) is None
    p.topk([], 5)
    got = p.extract_topk()
    assert got["ids"].shape == (0, 5) and got["count"].shape == (0,) and p.device_results()["ids"] is None
    p.close()


def test_everything_ties_the_id_order():
    for graph in (ck.complete_bipartite(3, 5), k.star(9), ck.complete(9)):
        n, ro, ci = ck.mirrored(graph)
        ref = k.Dense(n, ro, ci)
        p = ga.SimProblem().init(n, ro, ci)
        for options in ({}, {"strategy": ga.SIM_BLOCK}, {"strategy": ga.SIM_GLOBAL}):
            got, _ = _topk(p, np.arange(n), 8, **options)
            assert k.same(got, ref.topk(np.arange(n), 8, k.JACCARD)) is None
            assert all((np.diff(row[row >= 0]) > 0).all() for row in got["ids"])
        p.close()


def test_constructed_ties_rank_by_the_fraction():
    (n, r, c), first, second = k.rational_tie()
    _, ro, ci = ck.mirrored((n, r, c))
    p = ga.SimProblem().init(n, ro, ci)
    for strategy in STRATEGIES:
        got, _ = _topk(p, [0], 2, strategy=strategy)
        assert got["ids"].tolist() == [[first, second]] and got["num"].tolist() == [[2, 1]] and got["den"].tolist() == [[6, 3]]
        assert got["score"][0, 0] == got["score"][0, 1] == 1 / 3
    p.close()
    (n, r, c), first, second, m = k.near_tie()
    _, ro, ci = ck.mirrored((n, r, c))
    ref = k.Sets(n, ro, ci)
    p = ga.SimProblem().init(n, ro, ci)
    for strategy in (ga.SIM_AUTO, ga.SIM_GLOBAL):
        got, _ = _topk(p, [0, first], 2, strategy=strategy)
        assert got["ids"][0].tolist() == [first, second] and second < first  # equal as float32: the fraction decides, not the id
        assert got["num"][0].tolist() == [m, m - 1] and got["den"][0].tolist() == [2 * m + 1, 2 * m - 1]
        assert got["score"][0, 0] > got["score"][0, 1] and np.float32(got["score"][0, 0]) == np.float32(got["score"][0, 1])
        assert k.same(got, ref.topk([0, first], 2, k.JACCARD)) is None
    got, _ = _pairs(p, [0, 0], [first, second])
    assert k.same(got, ref.pairs([0, 0], [first, second], k.JACCARD)) is None
    p.close()


# ---------------- the handle ----------------

def test_two_enacts_of_both_modes_on_one_handle(borders_case):
    n, ro, ci, ref = borders_case
    rng = np.random.default_rng(23)
    u, v, sources = rng.integers(0, n, 500), rng.integers(0, n, 500), rng.integers(0, n, 90)
    p = ga.SimProblem(instrument=True).init(n, ro, ci)
    for call in (p.extract_pairs, p.extract_topk):
        with pytest.raises(RuntimeError, match=NOT_READY):
            call()
    first_pairs, _ = _pairs(p, u, v, metric=ga.SIM_OVERLAP, **LOW)
    first_topk, st = _topk(p, sources, 64, metric=ga.SIM_COMMON, skip_neighbors=1, strategy=ga.SIM_BLOCK)
    assert st["kernel_ms"] > 0 and st["kernel_launches"] >= 3 and st["table_probes"] > 0
    assert k.same(p.extract_pairs(), first_pairs) is None  # the pair result stays beside the top-k one
    p.reset()
    for call in (p.extract_pairs, p.extract_topk):
        with pytest.raises(RuntimeError, match=NOT_READY):
            call()
    second_topk, _ = _topk(p, sources[:40], 3, 1, metric=ga.SIM_SORENSEN, **LOW)
    second_pairs, _ = _pairs(p, u[:77], v[:77], 1, metric=ga.SIM_JACCARD, strategy=ga.SIM_WAVE)
    assert k.same(first_pairs, ref.pairs(u, v, k.OVERLAP)) is None and k.same(first_topk, ref.topk(sources, 64, k.COMMON, True)) is None
    assert k.same(second_pairs, ref.pairs(u[:77], v[:77], k.JACCARD)) is None
    assert k.same(second_topk, ref.topk(sources[:40], 3, k.SORENSEN)) is None
    assert p.set_option("nope", 1) == 1
    with pytest.raises(RuntimeError, match="code -1"):
        p.set_option("table_slots", 100)
    with pytest.raises(RuntimeError, match="code -3"):
        p.init(n, ro, ci)
    p.close()


def test_malformed_csr_is_refused():
    with pytest.raises(RuntimeError, match="code -2"):
        ga.SimProblem().init(3, np.array([0, 2, 1, 3], np.int32), np.array([1, 2, 0], np.int32))
    with pytest.raises(RuntimeError, match="code -2"):
        ga.SimProblem().init(3, np.array([0, 1, 2, 3], np.int32), np.array([1, 3, 0], np.int32))
