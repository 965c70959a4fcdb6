"""tests/_blocks_checker.py against naive loops in Python ints on tiny random cases: the references the GPU tests of the
building blocks (tests/test_blocks_gpu.py) lean on must themselves be right, wrap-around and identities included.  No GPU."""
import numpy as np
import pytest

import _blocks_checker as bk

INT_DTYPES = [np.int32, np.uint32, np.int64, np.uint64]
CASES = range(24)


def _wrap(x, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return dtype.type(x)
    bits = dtype.itemsize * 8
    x &= (1 << bits) - 1
    if dtype.kind == "i" and x >= 1 << (bits - 1):
        x -= 1 << bits
    return dtype.type(x)


def _combine(op, a, b):
    return {"plus": lambda: a + b, "multiplies": lambda: a * b, "maximum": lambda: max(a, b), "minimum": lambda: min(a, b),
            "bit_or": lambda: a | b, "bit_and": lambda: a & b, "bit_xor": lambda: a ^ b}[op]()


def _py(x):
    return float(x) if isinstance(x, np.floating) else int(x)


def _random_values(rng, n, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return rng.integers(-8, 9, n).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)


@pytest.mark.parametrize("case", CASES)
def test_exclusive_scan_against_python_ints(case):
    rng = np.random.default_rng(case)
    n = int(rng.integers(0, 40))
    v = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    prefix, total = bk.exclusive_scan(v)
    run = 0
    for i in range(n):
        assert int(prefix[i]) == run
        assert bool(bk.fits(prefix, np.int32)[i]) == (run < 2 ** 31) and bool(bk.fits(prefix, np.uint32)[i]) == (run < 2 ** 32)
        run += int(v[i])
    assert total == run and prefix.size == n


@pytest.mark.parametrize("case", CASES)
def test_stable_sort_against_insertion_sort(case):
    rng = np.random.default_rng(100 + case)
    n = int(rng.integers(0, 30))
    key_bits = int(rng.integers(1, 65))
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    keys[rng.random(n) < 0.3] &= np.uint64(0xFFFFFFFFFFFF0003)        # ties on the sorted bits
    bits = bk.sorted_bits(key_bits)
    assert bits % 8 == 0 and key_bits <= bits < key_bits + 8 and int(bk.sort_mask(key_bits)) == (1 << bits) - 1
    out = []
    for k in keys:                                                    # insertion behind every entry that is not larger: stable
        at = len(out)
        while at > 0 and (int(out[at - 1]) & ((1 << bits) - 1)) > (int(k) & ((1 << bits) - 1)):
            at -= 1
        out.insert(at, k)
    assert np.array_equal(bk.stable_sort(keys, key_bits), np.array(out, dtype=np.uint64))


@pytest.mark.parametrize("case", CASES)
def test_transpose_against_edge_loop(case):
    rng = np.random.default_rng(200 + case)
    nodes = int(rng.integers(1, 9))
    deg = rng.integers(0, 5, nodes)
    ro = np.concatenate([[0], np.cumsum(deg)])
    ci = rng.integers(0, nodes, int(ro[-1]))
    vals = rng.integers(0, 2 ** 32, ci.size, dtype=np.uint64).astype(np.uint32) if case % 2 else None
    rows = [[] for _ in range(nodes)]
    for v in range(nodes):
        for e in range(int(ro[v]), int(ro[v + 1])):
            rows[int(ci[e])].append((v, int(vals[e]) if vals is not None else 0))
    inv_ro, (row, col, val) = bk.transpose(ro, ci, vals)
    flat = [(u,) + p for u in range(nodes) for p in sorted(rows[u])]
    assert [int(x) for x in inv_ro] == [sum(len(r) for r in rows[:u]) for u in range(nodes + 1)]
    assert list(zip(row.tolist(), col.tolist(), val.tolist())) == flat
    # canonical_rows of a transpose written row by row in any order inside a row is the same thing
    inv_ci, inv_vals = [], []
    for u in range(nodes):
        for p in rng.permutation(len(rows[u])):
            inv_ci.append(rows[u][p][0])
            inv_vals.append(rows[u][p][1])
    got = bk.canonical_rows(inv_ro, np.array(inv_ci, dtype=np.int64), np.array(inv_vals, dtype=np.int64) if vals is not None else None)
    assert list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist())) == flat


@pytest.mark.parametrize("dtype", INT_DTYPES + [np.float32])
@pytest.mark.parametrize("case", range(8))
def test_wave_scans_against_double_loop(case, dtype):
    rng = np.random.default_rng(300 + case)
    n = int(rng.integers(1, 200))
    v = _random_values(rng, n, dtype)
    heads = rng.random(n) < (0.05, 0.5, 0.0, 1.0)[case % 4]
    ops = ("plus", "maximum", "minimum") if np.dtype(dtype).kind == "f" else ("plus", "multiplies", "maximum", "minimum", "bit_or",
                                                                              "bit_and", "bit_xor")
    for op in ops:
        seg = bk.wave_segmented(v, heads, op)
        inc = bk.wave_inclusive(v, op)
        none = bk.wave_segmented(v, None, op)
        for i in range(n):
            start = i - i % bk.WAVE
            acc = _py(v[start])
            for j in range(start + 1, i + 1):
                acc = _py(_wrap(_combine(op, acc, _py(v[j])), dtype))
            assert inc[i] == _wrap(acc, dtype) and none[i] == inc[i], (op, i)
            first = max([start] + [j for j in range(start, i + 1) if heads[j]])
            acc = _py(v[first])
            for j in range(first + 1, i + 1):
                acc = _py(_wrap(_combine(op, acc, _py(v[j])), dtype))
            assert seg[i] == _wrap(acc, dtype), (op, i)
        # lane 0 without a head combines the identity with its value: that is the value
        assert _wrap(_combine(op, _py(bk.identity(op, dtype)), _py(v[0])), dtype) == v[0]
    total = bk.wave_sum(v)
    for i in range(n):
        start = i - i % bk.WAVE
        assert total[i] == _wrap(sum(_py(x) for x in v[start:start + bk.WAVE]), dtype)


@pytest.mark.parametrize("case", CASES)
def test_rank_dpp_move_and_block_scan_against_loops(case):
    rng = np.random.default_rng(400 + case)
    n = int(rng.integers(1, 300))
    masks = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    rank = bk.rank_in_mask(masks)
    for i in range(n):
        assert int(rank[i]) == bin(int(masks[i]) & ((1 << (i % 64)) - 1)).count("1")
    v = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    for step in range(bk.DPP_STEPS):
        got = bk.dpp_move(v, step, 7)
        for i in range(n):
            lane, start = i % 64, i - i % 64
            if step < 4:
                src = lane - (1 << step) if lane % 16 >= (1 << step) else -1
            elif step == 4:
                src = {1: 15, 3: 47}.get(lane // 16, -1)
            else:
                src = 31 if lane >= 32 else -1
            want = 7 if src < 0 else (int(v[start + src]) if start + src < n else 0)
            assert int(got[i]) == want, (step, i)
    threads = (64, 256, 1024)[case % 3]
    for dtype in (np.int32, np.uint64):
        x = _random_values(rng, n, dtype)
        first, total1, second, total2 = bk.block_scan(x, threads)
        for i in range(n):
            base, t = i - i % threads, i % threads
            block = [_py(e) for e in x[base:base + threads]] + [0] * (base + threads - min(n, base + threads))
            assert first[i] == _wrap(sum(block[:t]), dtype) and total1[i] == _wrap(sum(block), dtype)
            assert second[i] == _wrap(sum(block[::-1][:t]), dtype) and total2[i] == total1[i]


@pytest.mark.parametrize("case", CASES)
def test_bisect_loop_against_sets(case):
    # the split is a loop already; here its outcome is restated with sets: the fresh, unmarked vertices, each once
    rng = np.random.default_rng(500 + case)
    nodes = int(rng.integers(1, 20))
    n = int(rng.integers(0, 60))
    dist = rng.integers(0, 64, nodes).astype(np.uint32)
    queue = rng.integers(-1, nodes, n).astype(np.int32)
    delta = (0.0, 1.0, 16.0, 2.5)[case % 4]
    level = int(rng.integers(0, 30))
    tag = 3
    lookup = np.where(rng.random(nodes) < 0.2, tag, rng.integers(-1, 3, nodes)).astype(np.int32)
    parked = None
    if case % 3:
        parked = np.where(rng.random(n) < 0.5, dist[np.maximum(queue, 0)], dist[np.maximum(queue, 0)] + 1).astype(np.uint32)
    count = n if case % 5 else n // 2
    near, far, far_min, after = bk.bisect(queue, count, dist, lookup, tag, delta, level, parked)
    live = {int(queue[i]) for i in range(count)
            if queue[i] >= 0 and lookup[queue[i]] != tag and (parked is None or parked[i] == dist[queue[i]])}
    buckets = {v: int(dist[v]) if delta == 0 else int(np.float32(dist[v]) / np.float32(delta)) for v in live}
    assert sorted(near) == sorted(v for v in live if buckets[v] <= level) and len(set(near)) == len(near)
    assert sorted(far) == sorted((v, int(dist[v])) for v in live if buckets[v] > level)
    assert far_min == min([buckets[v] for v, _ in far], default=0xFFFFFFFF)
    assert np.array_equal(after, np.where(np.isin(np.arange(nodes), list(live)), tag, lookup))
    if delta in (1.0, 16.0):
        assert all(bk.bucket_of(d, delta) == d // int(delta) for d in range(0, 4000, 7))
    assert bk.bucket_of(5, 2.5) == 2 and bk.bucket_of(4, 2.5) == 1 and bk.bucket_of(123, 0) == 123
