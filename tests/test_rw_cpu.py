"""The definition of the random walks (grx_rw_*) without a GPU: the two forms of tests/_rw_checker.py against each other on small
graphs, closed forms that follow from the definition, the pinned draws, one distribution check of the definition itself, and the
exports."""
import os
import re

import numpy as np
import pytest

import gunrockinst_amd as ga
from gunrockinst_amd import capi
from oracle import gr_oracle as o

import _rw_checker as k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("walks", "lengths", "visits", "steps", "ended_early", "biased_tries", "forced_fallbacks")

# (seed, walk, step, t) -> Draw, computed once with devgraph._splitmix64
DRAWS = {(0, 0, 0, 0): 12035550249420947055, (1, 2, 3, 4): 13731179152291499476,
         ((1 << 53) - 1, (1 << 31) - 1, (1 << 24) - 1, 255): 4361106646733862201, (20261020, 65, 17, 1): 414575086076068509}


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
MODES = {"uniform": {}, "weighted": {"weights": True}, "biased": {"bias": (3, 1, 7), "tries": 4},
         "weighted+biased": {"weights": True, "bias": (0, 5, 2), "tries": 2}}


def same(a, b):
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_forms_agree(name, mode):
    n, ro, ci = GRAPHS[name]
    kw = dict(MODES[mode])
    if kw.pop("weights", False):
        kw["weights"] = k.row_col_weights(ro, ci)
    starts = np.arange(n, dtype=np.int32) if n <= 64 else np.random.default_rng(5).integers(0, n, 70)
    a = k.scalar(n, ro, ci, starts, 11, seed=77, **kw)
    b = k.vectorised(n, ro, ci, starts, 11, seed=77, **kw)
    same(a, b)
    assert a["steps"] == int((a["lengths"] - 1).sum())
    assert np.array_equal(a["visits"], np.bincount(a["walks"][a["walks"] >= 0], minlength=n))
    assert np.array_equal(a["walks"][:, 0], starts)
    assert np.array_equal((a["walks"] >= 0).sum(axis=1), a["lengths"])


def test_zero_weights_and_dead_rows_agree():
    n, ro, ci = k.gnp(40, 0.1, 9)
    w = k.row_col_weights(ro, ci, 3) - 1  # weights 0 .. 2: zero entries, and rows whose total is 0
    starts = np.arange(n)
    a = k.scalar(n, ro, ci, starts, 9, weights=w, seed=3, bias=(1, 2, 3))
    same(a, k.vectorised(n, ro, ci, starts, 9, weights=w, seed=3, bias=(1, 2, 3)))
    ro64, sci, sw = k.sorted_copy(n, ro, ci, w)
    totals = np.bincount(np.repeat(np.arange(n), np.diff(ro64)), weights=sw, minlength=n)
    assert np.any(sw == 0) and np.any((np.diff(ro64) > 0) & (totals == 0)), "the case has zero entries and zero-total rows"
    positive = set((int(r), int(c)) for r, c, x in zip(np.repeat(np.arange(n), np.diff(ro64)), sci, sw) if x > 0)
    for row in a["walks"]:
        for u, v in zip(row[:-1], row[1:]):
            if v >= 0:
                assert (int(u), int(v)) in positive  # a zero-weight entry is never chosen


def test_directed_cycle_is_the_cycle():
    n, ro, ci = k.directed_cycle(7)
    for form in (k.scalar, k.vectorised):
        r = form(n, ro, ci, np.arange(n), 20, seed=1, bias=(1, 9, 2))
        want = (np.arange(n)[:, None] + np.arange(21)[None, :]) % n
        assert np.array_equal(r["walks"], want) and r["ended_early"] == 0 and r["steps"] == 7 * 20


def test_sink_gives_length_one():
    n, ro, ci = k.directed_path(5)
    r = k.scalar(n, ro, ci, [4, 3, 0], 6)
    assert r["lengths"].tolist() == [1, 2, 5] and r["walks"][0].tolist() == [4] + [-1] * 6
    assert r["walks"][2].tolist() == [0, 1, 2, 3, 4, -1, -1] and r["ended_early"] == 3


def test_all_weight_on_one_entry():
    n, ro, ci = k.complete(6)
    w = np.where(ci == (np.repeat(np.arange(n), 5) + 1) % n, 1000, 0).astype(np.int32)  # every row: only the arc to v + 1
    r = k.vectorised(n, ro, ci, np.arange(n), 12, weights=w, seed=8)
    assert np.array_equal(r["walks"], (np.arange(n)[:, None] + np.arange(13)[None, :]) % n)


def test_no_return_and_only_return():
    n, ro, ci = k.complete(5)  # symmetric, minimum out-degree 4
    r = k.scalar(n, ro, ci, np.arange(n), 30, seed=4, bias=(0, 1, 1), tries=64)
    assert r["forced_fallbacks"] == 0
    assert not np.any(r["walks"][:, 2:] == r["walks"][:, :-2])
    n, ro, ci = k.gnp(30, 0.2, 12, directed=False)
    starts = np.nonzero(np.diff(ro) > 0)[0]
    r = k.vectorised(n, ro, ci, starts, 12, seed=4, bias=(1, 0, 0), tries=128)
    assert r["forced_fallbacks"] == 0  # (a forced fallback may go anywhere; with 128 tries and degrees below 30 none happens here)
    assert np.array_equal(r["walks"][:, 2:], r["walks"][:, :-2])


def test_order_within_rows_does_not_matter():
    n, ro, ci = GRAPHS["gnp60"]
    rng = np.random.default_rng(2)
    w = rng.integers(0, 5, ci.shape[0]).astype(np.int32)
    ci2, w2 = k.shuffled_rows(ro, ci, w, rng)
    assert not np.array_equal(ci, ci2)
    for kw in ({}, {"bias": (2, 1, 4)}):
        same(k.scalar(n, ro, ci, np.arange(n), 10, weights=w, seed=6, **kw), k.scalar(n, ro, ci2, np.arange(n), 10, weights=w2, seed=6, **kw))
        same(k.vectorised(n, ro, ci, np.arange(n), 10, seed=6, **kw), k.vectorised(n, ro, ci2, np.arange(n), 10, seed=6, **kw))


def test_draws_are_pinned():
    for args, want in DRAWS.items():
        assert int(ga.rw_draw(*args)) == want and k.draw(*args) == want
    a = np.array(list(DRAWS), dtype=np.uint64)
    got = ga.rw_draw(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    assert got.dtype == np.uint64 and got.tolist() == list(DRAWS.values())
    assert ga.rw_draw(1, np.arange(3), 3, 4).shape == (3,)


def test_uniform_steps_on_k9_are_uniform():
    """72,000 uniform steps on K_9 from one seed: a step at u goes to each of its 8 neighbours with probability 1/8, so the count of an
    ordered pair (u, v) among the N_u steps taken at u is Binomial(N_u, 1/8), sigma = sqrt(N_u / 8 * 7 / 8): every pair within 5 sigma."""
    n, ro, ci = k.complete(9)
    r = k.vectorised(n, ro, ci, np.arange(720) % 9, 100, seed=2026)
    assert r["steps"] == 72000
    u, v = r["walks"][:, :-1].reshape(-1), r["walks"][:, 1:].reshape(-1)
    counts = np.bincount(u.astype(np.int64) * 9 + v, minlength=81).reshape(9, 9)
    assert np.all(np.diag(counts) == 0)
    at = counts.sum(axis=1)
    worst = 0.0
    for a in range(9):
        sigma = np.sqrt(at[a] * (1 / 8) * (7 / 8))
        for b in range(9):
            if a != b:
                worst = max(worst, abs(counts[a, b] - at[a] / 8) / sigma)
    print("largest deviation: %.3f sigma" % worst)
    assert worst < 5.0


def test_exports():
    for name in ("RwProblem", "gunrock_random_walks", "rw_draw", "RW_AUTO", "RW_LANE", "RW_TILE"):
        assert name in ga.__all__ and hasattr(ga, name)
    assert (ga.RW_AUTO, ga.RW_LANE, ga.RW_TILE) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    declared = set(re.findall(r"\b(grx_rw_\w+)\s*\(", header))
    assert {"grx_rw_create", "grx_rw_init", "grx_rw_init_device", "grx_rw_set_option", "grx_rw_reset", "grx_rw_enact", "grx_rw_stats",
            "grx_rw_extract", "grx_rw_device_results", "grx_rw_destroy"} <= declared
    assert declared <= set(capi.exported_symbols())
