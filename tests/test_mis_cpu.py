"""The host checker of the maximal independent set / greedy colourings (tests/_mis_checker.py) against hand-worked cases, against
itself (the sequential pass and the vectorised equation check must agree), against a literal restatement of the reference's
synchronous iteration, and the package's hash helper against a plain-int implementation.  No GPU."""
import json
import os

import numpy as np
import pytest

from _mis_checker import COLOR_FIRST_FIT, COLOR_ROUNDS, MODES, SET, entry_rows, greedy, higher, priorities, reference_rounds, verify

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _csr(n, pairs, mirrored=True):
    rows = np.array([p[0] for p in pairs] + ([p[1] for p in pairs] if mirrored else []), dtype=np.int64)
    cols = np.array([p[1] for p in pairs] + ([p[0] for p in pairs] if mirrored else []), dtype=np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    return np.searchsorted(rows, np.arange(n + 1)).astype(np.int32), cols.astype(np.int32)


def _fixture7():
    with open(os.path.join(GOLDEN, "reference_goldens.json")) as f:
        fx = json.load(f)["fixture7"]
    return np.array(fx["row_offsets"], np.int32), np.array(fx["col_indices"], np.int32)


# (name, nodes, (row_offsets, col_indices), priorities, expected SET, expected COLOR_ROUNDS, expected COLOR_FIRST_FIT)
HAND = [
    ("triangle, prio = id", 3, _csr(3, [(0, 1), (1, 2), (0, 2)]), [0, 1, 2], [0, 0, 1], [3, 2, 1], [3, 2, 1]),
    ("path of 5, prio = id", 5, _csr(5, [(0, 1), (1, 2), (2, 3), (3, 4)]), [0, 1, 2, 3, 4], [1, 0, 1, 0, 1], [5, 4, 3, 2, 1],
     [1, 2, 1, 2, 1]),
    ("path of 5, mixed", 5, _csr(5, [(0, 1), (1, 2), (2, 3), (3, 4)]), [5, 1, 4, 2, 3], [1, 0, 1, 0, 1], [1, 2, 1, 2, 1],
     [1, 2, 1, 2, 1]),
    ("star, centre last", 5, _csr(5, [(0, 1), (0, 2), (0, 3), (0, 4)]), [0, 1, 2, 3, 4], [0, 1, 1, 1, 1], [2, 1, 1, 1, 1],
     [2, 1, 1, 1, 1]),
    ("star, centre first", 5, _csr(5, [(0, 1), (0, 2), (0, 3), (0, 4)]), [9, 1, 2, 3, 4], [1, 0, 0, 0, 0], [1, 2, 2, 2, 2],
     [1, 2, 2, 2, 2]),
    ("two components and an isolated vertex, equal priorities", 6, _csr(6, [(0, 1), (1, 2), (0, 2), (3, 4)]), [7] * 6,
     [0, 0, 1, 0, 1, 1], [3, 2, 1, 2, 1, 1], [3, 2, 1, 2, 1, 1]),
    ("one-way edges only, {1 -> 0}", 2, _csr(2, [(1, 0)], mirrored=False), [0, 0], [0, 1], [2, 1], [2, 1]),
    # 7-vertex fixture, read undirected: 0-1 0-2 0-3 1-2 1-4 2-3 2-4 2-5 3-5 3-6 4-5 4-6 5-6
    ("fixture7, prio = id", 7, _fixture7(), [0, 1, 2, 3, 4, 5, 6], [0, 0, 1, 0, 0, 0, 1], [6, 5, 4, 3, 3, 2, 1], [4, 2, 1, 3, 3, 2, 1]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_worked(case):
    _, n, (ro, ci), prio, want_set, want_rounds, want_fit = case
    prio = np.array(prio, np.int32)
    for mode, want in ((SET, want_set), (COLOR_ROUNDS, want_rounds), (COLOR_FIRST_FIT, want_fit)):
        got = greedy(n, ro, ci, prio, mode)
        assert got.dtype == np.int32 and got.tolist() == want, (mode, got.tolist())
        assert verify(n, ro, ci, prio, mode, np.array(want, np.int32))


def _random_graph(rng):
    n = int(rng.integers(1, 400))
    m = int(n * rng.uniform(0.0, 5.0))
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)  # duplicates, self-loops, one-way edges, unsorted rows
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    ro = np.searchsorted(rows, np.arange(n + 1)).astype(np.int32)
    kind = int(rng.integers(0, 3))
    if kind == 0:
        prio = int(rng.integers(0, 1 << 32))                                 # hashed, a seed
    elif kind == 1:
        prio = rng.integers(-3, 3, n).astype(np.int32)                       # many ties: the id decides
    else:
        prio = rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    return n, ro, cols.astype(np.int32), prio


def _neighbour_pairs(n, ro, ci):
    rows, cols = entry_rows(ro), ci.astype(np.int64)
    keep = rows != cols
    return rows[keep], cols[keep]


def test_greedy_and_verify_agree_and_results_are_what_they_claim():
    rng = np.random.default_rng(11)
    for _ in range(60):
        n, ro, ci, prio = _random_graph(rng)
        a, b = _neighbour_pairs(n, ro, ci)
        graph = higher(n, ro, ci, prio)
        for mode in MODES:
            ids = greedy(n, ro, ci, prio, mode)
            assert verify(n, ro, ci, prio, mode, ids)
            assert verify(n, ro, ci, prio, mode, ids, graph=graph)
            if mode == SET:
                assert not ((ids[a] == 1) & (ids[b] == 1)).any(), "the set is not independent"
                covered = ids == 1
                covered[a[ids[b] == 1]] = True
                covered[b[ids[a] == 1]] = True
                assert covered.all(), "the set is not maximal"
            else:
                assert (ids >= 1).all() and (ids[a] != ids[b]).all(), "the colouring is not proper"
            # one entry changed: the equations no longer hold
            v = int(rng.integers(0, n))
            wrong = ids.copy()
            wrong[v] = 1 - wrong[v] if mode == SET else wrong[v] + 1
            assert not verify(n, ro, ci, prio, mode, wrong, graph=graph)
            if mode != SET and ids[v] > 1:
                wrong[v] = ids[v] - 1
                assert not verify(n, ro, ci, prio, mode, wrong, graph=graph)
        assert (greedy(n, ro, ci, prio, COLOR_FIRST_FIT) <= greedy(n, ro, ci, prio, COLOR_ROUNDS)).all()


def test_color_rounds_is_the_reference_schedule_run_to_the_end():
    rng = np.random.default_rng(12)
    for _ in range(40):
        n, ro, ci, prio = _random_graph(rng)
        assert np.array_equal(greedy(n, ro, ci, prio, COLOR_ROUNDS), reference_rounds(n, ro, ci, prio))


def test_verify_rejects_values_outside_the_range():
    ro, ci = _csr(3, [(0, 1), (1, 2), (0, 2)])
    prio = np.array([0, 1, 2], np.int32)
    assert not verify(3, ro, ci, prio, SET, np.array([0, 0, 2], np.int32))
    assert not verify(3, ro, ci, prio, COLOR_ROUNDS, np.array([3, 2, 0], np.int32))
    assert not verify(3, ro, ci, prio, COLOR_FIRST_FIT, np.array([3, 2], np.int32))


def _fmix32_int(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


@pytest.mark.parametrize("seed", [0, 1, 7, 0x6772, 0xFFFFFFFF])
def test_hash_helper_is_the_documented_formula(seed):
    import gunrockinst_amd as ga
    n = 1000
    want = [_fmix32_int(v + seed * 0x9E3779B9) for v in range(n)]
    got = ga.mis_priorities(n, seed)
    assert got.dtype == np.uint32 and got.tolist() == want
    assert priorities(n, seed).tolist() == want  # the checker's own hash
    assert _fmix32_int(1) == 0x514E28B7           # MurmurHash3 fmix32 known answer
