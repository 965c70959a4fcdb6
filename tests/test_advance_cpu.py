"""tests/_advance_checker.py against a naive double loop over (frontier entry, out-edge) on tiny graphs: the reference the GPU
tests of the advance operator (tests/test_advance_gpu.py) lean on must itself be right, identities included.  No GPU."""
import numpy as np
import pytest

import _advance_checker as ck

# (degrees, nodes, frontier): a path-like mix, a repeated vertex, a lone hub, vertices without out-edges as destinations
GRAPHS = [
    ([1], 1, [0]),
    ([2, 1, 3, 0, 1], 6, [2, 0, 4]),
    ([3, 3, 3], 3, [1, 1, 0]),
    ([0, 9, 0, 0], 4, [1]),
    ([1, 2, 3, 4, 5, 0, 0, 2], 9, [7, 3, 1, 4, 0, 2]),
]
DTYPES = [np.int32, np.uint32, np.float32, np.int64, np.uint64]


def _naive_slots(ro, ci, frontier):
    for i, v in enumerate(frontier):
        for e in range(int(ro[v]), int(ro[v + 1])):
            yield i, e, v, int(ci[e])


def _combine(op, a, b):
    return {"plus": lambda: a + b, "multiplies": lambda: a * b, "maximum": lambda: max(a, b), "minimum": lambda: min(a, b),
            "bit_or": lambda: a | b, "bit_and": lambda: a & b, "bit_xor": lambda: a ^ b}[op]()


def _naive_identity(op, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        big = float(np.finfo(dtype).max)
        return {"plus": 0.0, "multiplies": 1.0, "maximum": -big, "minimum": big}[op]
    lo, hi = int(np.iinfo(dtype).min), int(np.iinfo(dtype).max)
    return {"plus": 0, "multiplies": 1, "maximum": lo, "minimum": hi, "bit_or": 0, "bit_xor": 0, "bit_and": hi if lo == 0 else -1}[op]


def _wrap(x, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return dtype.type(x)
    bits = dtype.itemsize * 8
    x &= (1 << bits) - 1
    if dtype.kind == "i" and x >= 1 << (bits - 1):
        x -= 1 << bits
    return dtype.type(x)


@pytest.mark.parametrize("case", range(len(GRAPHS)))
@pytest.mark.parametrize("density", [None, 0.0, 0.5, 1.0])
def test_queue_and_claim_against_double_loop(case, density):
    degrees, n, frontier = GRAPHS[case]
    ro, ci = ck.graph_from_degrees(degrees, seed=case, nodes=n)
    assert np.array_equal(np.diff(ro)[:len(degrees)], degrees) and ro[-1] == sum(degrees) == ci.size
    rng = np.random.default_rng(100 + case)
    mask = None if density is None else (rng.random(n) < density).astype(np.int32)
    acc, hits, src = [], np.zeros(ci.size, np.int32), np.full(ci.size, -1, np.int32)
    for _, e, s, d in _naive_slots(ro, ci, frontier):
        if mask is None or mask[d]:
            acc.append(d)
            hits[e] += 1
            src[e] = s
    got = ck.expected_queue(ro, ci, frontier, mask)
    assert np.array_equal(got[0], np.sort(np.array(acc, dtype=np.int32)))
    assert np.array_equal(got[1], hits) and np.array_equal(got[2], src)

    labels = np.where(rng.random(n) < 0.5, -1, 3).astype(np.int32)
    after = labels.copy()
    won = []
    for _, e, s, d in _naive_slots(ro, ci, frontier):
        if after[d] == -1:
            after[d] = 9
            won.append(d)
    w, a = ck.expected_claim(ro, ci, frontier, labels, 9)
    assert np.array_equal(w, np.sort(np.array(won, dtype=np.int32))) and np.array_equal(a, after)


def test_full_frontier_invariants_accept_the_truth_and_reject_a_shift():
    ro, ci = ck.graph_from_degrees([2, 1, 3, 0, 1], seed=1, nodes=6)
    acc, _, _ = ck.expected_queue(ro, ci, [2, 0, 4])
    deg = np.diff(ro)
    v = acc[deg[acc] > 0][::-1].copy()                      # any order is allowed
    sc = np.concatenate([[0], np.cumsum(deg[v])])
    ck.check_full_frontier(ro, acc, v, ro[v], sc[:-1], sc[-1])
    assert (deg[acc] == 0).any(), "this graph is meant to reach a vertex without out-edges"
    with pytest.raises(AssertionError):
        ck.check_full_frontier(ro, acc, v, ro[v], sc[:-1] + 1, sc[-1])
    with pytest.raises(AssertionError):
        ck.check_full_frontier(ro, acc, acc, ro[acc], np.zeros(acc.size), 0)   # zero-degree destinations must be dropped


@pytest.mark.parametrize("case", range(len(GRAPHS)))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r_type", ["vertex", "edge"])
def test_reduce_against_double_loop(case, dtype, r_type):
    degrees, n, frontier = GRAPHS[case]
    ro, ci = ck.graph_from_degrees(degrees, seed=case, nodes=n)
    rng = np.random.default_rng(7 * case + 1)
    size = n if r_type == "vertex" else ci.size
    kind = np.dtype(dtype).kind
    if kind == "f":
        values = rng.integers(-8, 9, size).astype(dtype)
    elif kind == "u":
        values = rng.integers(0, 2 ** 31, size).astype(dtype) * 2 + 1    # high bit in play, products wrap
    else:
        values = rng.integers(-2 ** 31, 2 ** 31, size).astype(dtype)
    ops = [op for op in ck.OPS if kind != "f" or not op.startswith("bit_")]
    for op in ops:
        for density in (None, 0.0, 0.6):
            mask = None if density is None else (rng.random(n) < density).astype(np.int32)
            want = [_naive_identity(op, dtype)] * len(frontier)
            for i, e, s, d in _naive_slots(ro, ci, frontier):
                if mask is None or mask[d]:
                    x = values[d if r_type == "vertex" else e]
                    want[i] = _combine(op, want[i], float(x) if kind == "f" else int(x))
            want = np.array([_wrap(x, dtype) for x in want], dtype=dtype)
            got, wide, mags, degs = ck.expected_reduce(ro, ci, frontier, values, r_type, op, mask)
            assert got.dtype == np.dtype(dtype) and np.array_equal(got, want), (op, density)
            assert np.array_equal(degs, np.diff(ro)[frontier])
            if density == 0.0:
                assert (got == ck.identity(op, dtype)).all()


def test_reduce_by_vertex_placement_prefill_and_sentinel():
    ro, ci = ck.graph_from_degrees([1, 2, 3, 4, 5, 0, 0, 2], seed=3, nodes=9)
    frontier = [7, 3, 1]
    values = np.arange(1, 10, dtype=np.int32)
    by_pos, _, _, _ = ck.expected_reduce(ro, ci, frontier, values, "vertex", "plus")
    sentinel = np.full(9, -77, dtype=np.int32)
    # no prefill: positions outside the frontier keep what was there, the frontier's entries hold the results
    kept, _, _, _ = ck.expected_reduce(ro, ci, frontier, values, "vertex", "plus", by_vertex=True, out=sentinel, prefill=False)
    assert np.array_equal(kept[frontier], by_pos) and (np.delete(kept, frontier) == -77).all()
    # prefill of the first 4 entries only
    part, _, _, _ = ck.expected_reduce(ro, ci, frontier, values, "vertex", "maximum", by_vertex=True, out=sentinel, out_len=4)
    assert part[0] == part[2] == np.iinfo(np.int32).min and part[4] == part[8] == -77
    with pytest.raises(AssertionError):                     # a vertex twice has no by-vertex meaning
        ck.expected_reduce(ro, ci, [1, 1], values, "vertex", "plus", by_vertex=True)


def test_identities():
    assert ck.identity("maximum", np.int64) == -2 ** 63 and ck.identity("minimum", np.uint64) == 2 ** 64 - 1
    assert ck.identity("bit_and", np.uint32) == 0xFFFFFFFF and ck.identity("bit_and", np.int32) == -1
    assert ck.identity("maximum", np.float32) == -np.finfo(np.float32).max and ck.identity("multiplies", np.float32) == 1.0
    assert ck.identity("plus", np.uint32) == 0 and ck.identity("bit_xor", np.int32) == 0 and ck.identity("bit_or", np.int32) == 0


def test_exact_product_values_bound_every_row():
    ro, ci = ck.graph_from_degrees([4000, 3, 70], seed=5, nodes=16)
    frontier = [0, 2, 1, 0]
    rng = np.random.default_rng(0)
    for r_type in ("vertex", "edge"):
        w = ck.max_row_multiplicity(ro, ci, frontier, r_type)
        vals = ck.exact_product_values(w, rng)
        assert set(np.unique(vals)) <= {0.5, 1.0, 2.0}
        entry, edge, _, dst, _ = ck.slots(ro, ci, frontier)
        expo = np.abs(np.log2(vals[dst if r_type == "vertex" else edge]))
        assert np.bincount(entry, weights=expo).max() <= 100


def test_the_binding_builds_the_frontier_triple_and_refuses_a_vertex_without_edges():
    # host-side part of ga.advance_queue / ga.advance_reduce: pure numpy, nothing is launched
    from gunrockinst_amd import advance_frontier
    ro, ci = ck.graph_from_degrees([2, 1, 3, 0, 1], seed=1, nodes=6)
    v, rs, sc, total = advance_frontier(ro, [2, 0, 4, 2])
    _, _, _, _, scan = ck.slots(ro, ci, [2, 0, 4, 2])
    assert np.array_equal(v, [2, 0, 4, 2]) and np.array_equal(rs, ro[[2, 0, 4, 2]]) and np.array_equal(sc, scan[:-1]) and total == scan[-1] == 9
    assert all(a.dtype == np.int32 for a in (v, rs, sc))
    for bad in ([3], [0, 5], [6], [-1]):
        with pytest.raises(ValueError):
            advance_frontier(ro, bad)
    assert advance_frontier(ro, [])[3] == 0
