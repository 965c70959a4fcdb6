"""The device building blocks under the operators, each by itself through the C ABI (lib/blocks_app.hip): the device-wide
exclusive scan and the radix key sort of graphio/device_csr.hpp + device_sort.hpp, the CSR transpose, the wave and workgroup
scans of util/device_intrinsics.hpp, and the near/far split of priority_queue/kernel.hpp.

Expected values come from tests/_blocks_checker.py (numpy and Python ints; itself checked against naive loops in
test_blocks_cpu.py).  Everything here is integer work, or float work that does not depend on the order of combination (float
MINIMUM / MAXIMUM; float PLUS of integer-valued terms whose partial sums stay below 2^24): EVERY comparison is exact.

Sizes are chosen on the edges of the machinery: a scan tile is 4096 elements and ScanSumsKernel takes 1024 tile sums per round;
a sort tile is 4096 keys sorted 8 bits per pass; the transpose handles 64 rows per wave, rows longer than 16 by the whole wave,
2048 * 256 rows per trip of its group loop; a wave is 64 lanes in four DPP rows of 16; the split takes tiles of 1024 queue
entries and flushes its 2048-entry staging buffer when more than 1024 are pending.

Not covered: float MULTIPLIES in the segmented scan (a product is exact only for chosen factors; the advance tests cover it).
"""
import functools

import numpy as np
import pytest

import _advance_checker as ack
import _blocks_checker as bk

pytestmark = pytest.mark.gpu

ga = pytest.importorskip("gunrockinst_amd")

FILL = -7                                                            # what the wrappers pre-fill every output array with


# ================================================================ scan ====================================================

SCAN_TILE, SCAN_ROUND = 4096, 1024
SCAN_SMALL = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8192, 8193)      # one element, a wave, a tile, two tiles
SCAN_LARGE = (SCAN_TILE * SCAN_ROUND - 1, SCAN_TILE * SCAN_ROUND, SCAN_TILE * SCAN_ROUND + 1, SCAN_TILE * 2049)
SCAN_OUT = ("int32", "uint32", "uint64")
SCAN_VALUES = ("zeros", "ones", "random_below_16", "nonzero_first_of_tile", "nonzero_last_of_tile", "nonzero_last_of_short_tile")


def _scan_input(n, kind):
    """None when the pattern does not exist at this length (no full tile, no short tile)"""
    v = np.zeros(n, dtype=np.uint32)
    if kind == "ones":
        v[:] = 1
    elif kind == "random_below_16":
        v[:] = np.random.default_rng(n).integers(0, 16, n)
    elif kind == "nonzero_first_of_tile":                            # first position of the LAST tile
        if n == 0:
            return None
        v[(n - 1) // SCAN_TILE * SCAN_TILE] = 0xFFFFFFFF
        v[0] |= 3
    elif kind == "nonzero_last_of_tile":                             # last position of the last FULL tile
        if n < SCAN_TILE:
            return None
        v[n // SCAN_TILE * SCAN_TILE - 1] = 0xFFFFFFFF
    elif kind == "nonzero_last_of_short_tile":                       # last valid position of a short tile
        if n % SCAN_TILE == 0:
            return None
        v[n - 1] = 0xFFFFFFFF
    return v


def _check_scan(values, label):
    prefix, total = bk.exclusive_scan(values)
    for out_type in SCAN_OUT:
        got, got_total = ga.device_scan(values, out_type)
        assert got.dtype == np.dtype(out_type) and got.size == values.size
        assert got_total == total, "%s %s: the 64-bit total" % (label, out_type)
        if out_type == "uint64":
            assert np.array_equal(got, prefix), "%s: 64-bit prefix" % label
        else:                                                        # a 32-bit output holds the exact prefix wherever that fits
            ok = bk.fits(prefix, out_type)
            assert np.array_equal(got[ok].astype(np.uint64), prefix[ok]), "%s %s: prefix where it fits" % (label, out_type)


def _scan_pattern_exists(n, kind):
    return {"nonzero_first_of_tile": n > 0, "nonzero_last_of_tile": n >= SCAN_TILE, "nonzero_last_of_short_tile": n % SCAN_TILE != 0}.get(kind, True)


@pytest.mark.parametrize("n,kind", [(n, kind) for n in SCAN_SMALL + SCAN_LARGE for kind in SCAN_VALUES if _scan_pattern_exists(n, kind)])
def test_scan_prefix_and_total(n, kind):
    _check_scan(_scan_input(n, kind), "n=%d %s" % (n, kind))


def test_scan_patterns_sit_where_their_names_say():
    assert np.flatnonzero(_scan_input(8193, "nonzero_first_of_tile")).tolist() == [0, 8192]
    assert np.flatnonzero(_scan_input(8193, "nonzero_last_of_tile")).tolist() == [8191]
    assert np.flatnonzero(_scan_input(8193, "nonzero_last_of_short_tile")).tolist() == [8192]
    assert np.flatnonzero(_scan_input(SCAN_TILE * 2049, "nonzero_first_of_tile")).tolist() == [0, SCAN_TILE * 2048]
    assert SCAN_LARGE[1] // SCAN_TILE == SCAN_ROUND and SCAN_LARGE[3] // SCAN_TILE == 2 * SCAN_ROUND + 1


@pytest.mark.parametrize("n", [5000, SCAN_TILE * SCAN_ROUND + 1])
def test_scan_sums_that_leave_32_bits(n):
    values = np.random.default_rng(n).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    expected, run = np.empty(n, dtype=np.uint64), 0                  # Python ints
    for i, x in enumerate(values.tolist()):
        expected[i] = run
        run += x
    assert run >= 2 ** 32 * (n // 4)
    got, total = ga.device_scan(values, "uint64")
    assert total == run and np.array_equal(got, expected)
    for out_type in ("int32", "uint32"):                             # the total stays exact, the prefix where it fits
        got, total = ga.device_scan(values, out_type)
        ok = bk.fits(expected, out_type)
        assert total == run and 0 < np.count_nonzero(ok) < n and np.array_equal(got[ok].astype(np.uint64), expected[ok])


# ================================================================ sort ====================================================

SORT_BITS = (1, 7, 8, 9, 16, 31, 33, 40, 63, 64)
SORT_SIZES = (0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 8193, (1 << 20) + 3)
SORT_SETS = ("random", "sorted", "reversed", "all_equal", "bytes_ff", "bytes_00", "two_values_alternating", "sentinels_mixed_in")
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _random_low(rng, n, bits):
    x = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    return x & np.uint64((1 << bits) - 1)


def _sort_keys(kind, n, key_bits, seed):
    """keys whose sorted bits follow `kind`; where at least 24 bits stay free above the sorted ones they carry the input index,
    so a sort that is not stable, or that touches the upper bits, cannot produce the expected array"""
    bits = bk.sorted_bits(key_bits)
    rng = np.random.default_rng(seed)
    if kind == "random":
        low = _random_low(rng, n, bits)
    elif kind == "sorted":
        low = np.sort(_random_low(rng, n, bits))
    elif kind == "reversed":
        low = np.sort(_random_low(rng, n, bits))[::-1].copy()
    elif kind == "all_equal":                                        # one digit owns every tile: in-wave ranks over a full mask
        low = np.full(n, 0x5A5A5A5A5A5A5A5A & ((1 << bits) - 1), dtype=np.uint64)
    elif kind == "bytes_ff":
        low = np.full(n, (1 << bits) - 1, dtype=np.uint64)
    elif kind == "bytes_00":
        low = np.zeros(n, dtype=np.uint64)
    elif kind == "two_values_alternating":                           # lane by lane
        pair = np.array([0xC3C3C3C3C3C3C3C3 & ((1 << bits) - 1), 0x3C3C3C3C3C3C3C3C & ((1 << bits) - 1)], dtype=np.uint64)
        low = pair[np.arange(n) % 2]
    else:
        low = _random_low(rng, n, bits)
    keys = low
    if 64 - bits >= 24:
        keys = low | (np.arange(n, dtype=np.uint64) << np.uint64(bits))
    if kind == "sentinels_mixed_in":                                 # ~0ull, as the CSR builders mark dropped tuples
        keys = np.where(rng.random(n) < 0.1, ALL_ONES, keys)
    return keys


@pytest.mark.parametrize("key_bits", SORT_BITS)
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_is_ascending_and_stable_on_the_sorted_bits(n, key_bits):
    sets = [_sort_keys(kind, n, key_bits, seed=n + key_bits + i) for i, kind in enumerate(SORT_SETS)]
    got = ga.device_key_sort(sets, [key_bits] * len(sets))
    for kind, keys, out in zip(SORT_SETS, sets, got):
        assert np.array_equal(out, bk.stable_sort(keys, key_bits)), "%s, n=%d, key_bits=%d" % (kind, n, key_bits)


def test_sort_key_sets_are_what_their_names_say():
    for key_bits in SORT_BITS:
        bits, mask = bk.sorted_bits(key_bits), bk.sort_mask(key_bits)
        sets = dict(zip(SORT_SETS, (_sort_keys(kind, 4097, key_bits, 1) for kind in SORT_SETS)))
        assert np.unique(sets["all_equal"] & mask).size == 1 and np.unique(sets["two_values_alternating"] & mask).size == 2
        assert ((sets["bytes_ff"] & mask) == mask).all() and ((sets["bytes_00"] & mask) == 0).all()
        assert (np.diff((sets["sorted"] & mask).astype(np.float64)) >= 0).all() and (np.diff((sets["reversed"] & mask).astype(np.float64)) <= 0).all()
        assert 300 < np.count_nonzero(sets["sentinels_mixed_in"] == ALL_ONES) < 550
        if 64 - bits >= 24:                                          # the input index rides above the sorted bits
            assert np.array_equal(sets["all_equal"] >> np.uint64(bits), np.arange(4097, dtype=np.uint64))
    assert [k for k in SORT_BITS if 64 - bk.sorted_bits(k) >= 24] == [1, 7, 8, 9, 16, 31, 33, 40]


def test_sort_reuses_one_sorter_for_smaller_and_larger_arrays():
    # Reserve keeps the capacity of the largest array so far while the histogram of each sort follows its own tile count
    sizes, bits = (100_000, 17, 4097, 0, 100_000), (40, 16, 64, 8, 33)
    sets = [_sort_keys("random", n, b, seed=1000 + i) for i, (n, b) in enumerate(zip(sizes, bits))]
    assert not np.array_equal(sets[0] & bk.sort_mask(33), sets[4] & bk.sort_mask(33))
    got = ga.device_key_sort(sets, bits)
    for i, (keys, b, out) in enumerate(zip(sets, bits, got)):
        assert np.array_equal(out, bk.stable_sort(keys, b)), "array %d of the sequence (n=%d, key_bits=%d)" % (i, keys.size, b)


# ================================================================ transpose ===============================================

LONG_ROW = 16                                                        # rows longer than this are walked by the whole wave
ROW_DEGREES = (0, 1, 15, 16, 17, 63, 64, 65, 5000)
GROUP_TRIP = 2048 * 256                                              # rows per trip of the scatter's group loop


def _edge_values(ro, ci):
    """a function of (source, destination, ordinal): a value that travelled with the wrong edge shows"""
    src = np.repeat(np.arange(ro.size - 1, dtype=np.uint64), np.diff(ro))
    return ((src * np.uint64(2654435761) + ci.astype(np.uint64) * np.uint64(40503) + np.arange(ci.size, dtype=np.uint64) * np.uint64(7))
            & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _check_transpose(ro, ci):
    for with_values in (False, True):
        vals = _edge_values(ro, ci) if with_values else None
        want_ro, want_rows = bk.transpose(ro, ci, vals)
        got = ga.device_transpose(ro, ci, vals)
        assert np.array_equal(got[0], want_ro), "inverse row offsets"
        got_rows = bk.canonical_rows(got[0], got[1], got[2] if with_values else None)
        for name, a, b in zip(("row", "source", "value"), got_rows, want_rows):
            assert np.array_equal(a, b), "inverse rows as multisets of (source, value): %s" % name


def _graph_with_row(degree, vertex, nodes):
    degs = [1 + i % 3 for i in range(nodes)]
    degs[vertex] = degree
    return ack.graph_from_degrees(degs, seed=degree * 1000 + vertex, nodes=nodes)


# nodes = 2 full groups of 64 rows + a partial group of 37
PLACES = {"lane0_of_a_group": 64, "lane63_of_a_group": 127, "last_partial_group": 128 + 36}


@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("degree", ROW_DEGREES)
def test_transpose_row_of_each_degree_in_each_place(degree, place):
    nodes, v = 165, PLACES[place]
    assert nodes % 64 == 37 and v < nodes and (v % 64 == {"lane0_of_a_group": 0, "lane63_of_a_group": 63}.get(place, 36))
    ro, ci = _graph_with_row(degree, v, nodes)
    assert ro[v + 1] - ro[v] == degree
    _check_transpose(ro, ci)


@pytest.mark.parametrize("nodes", [1, 63, 64, 65, 1000])
def test_transpose_vertex_counts_around_a_group(nodes):
    rng = np.random.default_rng(nodes)
    degs = rng.choice(np.array(ROW_DEGREES[:-1]), nodes)              # every degree on either side of the long-row switch
    ro, ci = ack.graph_from_degrees(degs, seed=nodes, nodes=nodes)
    _check_transpose(ro, ci)


def test_transpose_second_trip_of_the_group_loop():
    nodes = GROUP_TRIP + 65
    degs = np.zeros(nodes, dtype=np.int64)
    degs[np.random.default_rng(5).choice(GROUP_TRIP, 1500, replace=False)] = 2
    degs[GROUP_TRIP + 5] = 300                                       # a long row in the first group past the first trip
    degs[GROUP_TRIP + 63] = LONG_ROW                                 # the longest short row, lane 63 of that group
    degs[nodes - 1] = 17                                             # ... and a long row in the last, one-row group
    ro, ci = ack.graph_from_degrees(degs, seed=6, nodes=nodes)
    assert 3000 < ci.size < 4000
    _check_transpose(ro, ci)


def test_transpose_without_edges():
    _check_transpose(np.zeros(101, dtype=np.int32), np.zeros(0, dtype=np.int32))


def test_transpose_keeps_duplicate_edges_and_self_loops():
    # vertex 0: 0 -> 3 three times and a self loop twice; vertex 3: a long row of self loops and duplicates; vertex 69: a self loop
    rows = {0: [3, 3, 3, 0, 0], 3: [3] * 20 + [0] * 20, 5: [6, 6], 69: [69]}
    nodes = 70
    degs = [len(rows.get(v, [])) for v in range(nodes)]
    ro = np.concatenate([[0], np.cumsum(degs)]).astype(np.int32)
    ci = np.array([u for v in range(nodes) for u in rows.get(v, [])], dtype=np.int32)
    want_ro, _ = bk.transpose(ro, ci)
    assert want_ro[-1] == ci.size == 48 and want_ro[4] - want_ro[3] == 23 and want_ro[1] - want_ro[0] == 22
    _check_transpose(ro, ci)


def test_transpose_one_column_receives_every_edge():
    nodes = 1000
    degs = np.random.default_rng(8).choice(np.array(ROW_DEGREES[:-1]), nodes)
    ro, _ = ack.graph_from_degrees(degs, seed=8, nodes=nodes)
    ci = np.full(int(ro[-1]), 7, dtype=np.int32)                     # an in-hub: every scatter bumps the same cursor
    _check_transpose(ro, ci)


# ================================================================ wave and workgroup blocks ================================

BORDER_LANES = (0, 15, 16, 31, 32, 47, 48, 63)                       # either side of every DPP row boundary, and the ends
THREADS = (64, 256, 1024)
TAIL = 37                                                            # a partial wave behind the patterns


def _one_hot(lane, value):
    w = np.zeros(64, dtype=np.uint64)
    w[lane] = value
    return w


def _sum_waves(dtype, seed):
    """64-lane input patterns for the sums, one per row, plus a partial wave"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    big = 2 ** 32 if dtype.kind == "u" else 2 ** 20                   # signed sums stay inside their type; unsigned ones wrap
    waves = [np.ones(64, dtype=np.uint64), np.arange(64, dtype=np.uint64)]
    waves += [_one_hot(lane, 5 + lane) for lane in BORDER_LANES]
    waves += [rng.integers(0, 1000, 64).astype(np.uint64) for _ in range(6)]
    if dtype.kind == "u":                                            # near 2^32: wrap-around, compared modulo 2^32 (2^64 for 64 bits)
        waves += [np.uint64(big) - rng.integers(1, 50, 64).astype(np.uint64) for _ in range(3)]
        waves += [np.where(_one_hot(lane, 1) != 0, np.uint64(big - 1), np.uint64(1)) for lane in BORDER_LANES]
    if dtype == np.uint64:                                           # sums that cross from the low into the high word, and wrap
        waves += [rng.integers(2 ** 62, 2 ** 63, 64).astype(np.uint64) * np.uint64(2) for _ in range(3)]
    flat = np.concatenate(waves + [rng.integers(0, 1000, TAIL).astype(np.uint64)])
    return flat.astype(dtype)


@pytest.mark.parametrize("threads", THREADS)
def test_wave_inclusive_sums(threads):
    for dtype in (np.int32, np.uint32, np.uint64):
        x = _sum_waves(dtype, 1)
        assert x.size > 1024
        assert np.array_equal(ga.wave_ops("inclusive_sum", x, threads), bk.wave_inclusive(x)), "WaveInclusiveSum %s" % np.dtype(dtype)
        assert np.array_equal(ga.wave_ops("wave_sum", x, threads), bk.wave_sum(x)), "WaveSum %s" % np.dtype(dtype)
    x = _sum_waves(np.uint32, 2)
    got, want = ga.wave_ops("inclusive_sum_dpp", x, threads), bk.wave_inclusive(x)
    assert np.array_equal(got, want), "WaveInclusiveSumDpp: first wrong lanes %s" % (np.flatnonzero(got != want)[:8] % 64)


@pytest.mark.parametrize("threads", THREADS)
def test_wave_inclusive_max(threads):
    rng = np.random.default_rng(3)
    waves = [np.zeros(64, dtype=np.uint32), np.arange(64, 0, -1, dtype=np.uint32) * 1000]         # all zero; strictly decreasing
    for lane in BORDER_LANES:                                        # the maximum at each border lane, smaller values around it
        w = rng.integers(0, 2 ** 31, 64).astype(np.uint32)
        w[lane] = 2 ** 32 - 1 - lane
        waves.append(w)
    waves += [rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32) for _ in range(8)]
    waves.append(rng.integers(0, 2 ** 32, TAIL, dtype=np.uint64).astype(np.uint32))
    x = np.concatenate(waves)
    got, want = ga.wave_ops("inclusive_max_dpp", x, threads), bk.wave_inclusive(x, "maximum")
    assert np.array_equal(got, want), "WaveInclusiveMaxDpp: first wrong lanes %s" % (np.flatnonzero(got != want)[:8] % 64)


def _heads(kind, rng):
    h = np.zeros(64, dtype=bool)
    if kind == "lane0":
        h[0] = True
    elif kind == "every_lane":
        h[:] = True
    elif kind == "all_borders":
        h[list(BORDER_LANES[1:])] = True
    elif isinstance(kind, int):
        h[kind] = True
    elif kind == "random_0.05":
        h = rng.random(64) < 0.05
    elif kind == "random_0.5":
        h = rng.random(64) < 0.5
    return h                                                         # "none": lane 0 starts an implicit segment over the identity


HEAD_PATTERNS = ("none", "lane0", "every_lane") + BORDER_LANES[1:] + ("all_borders", "random_0.05", "random_0.5")
WAVES_PER_PATTERN = 3
# every (operator, type) the library hands to WaveSegmentedScanDpp through advance::LaunchReduce, float MULTIPLIES left out
SEGMENTED = ([(op, t) for t in ("int32", "uint32") for op in ("plus", "multiplies", "maximum", "minimum", "bit_or", "bit_and", "bit_xor")] +
             [(op, "float32") for op in ("plus", "maximum", "minimum")] +
             [(op, t) for t in ("int64", "uint64") for op in ("plus", "maximum", "minimum")])
assert len(SEGMENTED) == 23


def _segmented_values(op, tname, n, rng):
    """values whose scan does not depend on the order of combination and never overflows a signed type"""
    dtype = np.dtype(tname)
    if dtype.kind == "f":
        if op == "plus":
            return rng.integers(-8, 9, n).astype(dtype)              # 64 * 8 < 2^24: every partial sum is exact
        return (rng.standard_normal(n) * 1e6).astype(dtype)          # MINIMUM / MAXIMUM never round
    if dtype.kind == "u":
        x = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)             # odd: a product never collapses to 0
        return x.astype(dtype)                                       # sums and products wrap: defined
    if op == "multiplies":                                           # int32: at most 64 factors of magnitude <= 2 ... but 2^64 overflows:
        x = rng.choice(np.array([1, -1], dtype=dtype), n)            # ... so at most 20 of the 64 lanes of a wave carry a 2 or -2
        for w in range(0, n, 64):
            at = w + rng.choice(min(64, n - w), min(20, n - w), replace=False)
            x[at] = rng.choice(np.array([2, -2], dtype=dtype), at.size)
        return x
    if op == "plus":
        half = 2 ** (8 * dtype.itemsize - 8)                         # 64 terms below 2^(bits - 8): inside the type
        return rng.integers(-half, half, n).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)


@functools.lru_cache(maxsize=None)
def _head_flags():
    rng = np.random.default_rng(4)
    flags = np.concatenate([_heads(kind, rng) for kind in HEAD_PATTERNS for _ in range(WAVES_PER_PATTERN)] + [rng.random(TAIL) < 0.2])
    flags.setflags(write=False)
    return flags


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("op,tname", SEGMENTED)
def test_wave_segmented_scan(op, tname, threads):
    heads = _head_flags()
    assert heads.size == 64 * WAVES_PER_PATTERN * len(HEAD_PATTERNS) + TAIL > 2 * 1024
    x = _segmented_values(op, tname, heads.size, np.random.default_rng(len(op) + heads.size))
    got, want = ga.wave_ops("segmented_scan_dpp", x, threads, r_op=op, heads=heads), bk.wave_segmented(x, heads, op)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s %s: first wrong element %d (head pattern %s, lane %d)" % (
        op, tname, bad[0], HEAD_PATTERNS[min(bad[0] // (64 * WAVES_PER_PATTERN), len(HEAD_PATTERNS) - 1)], bad[0] % 64)
    got = ga.wave_ops("segmented_scan_dpp", x, threads, r_op=op)     # no head array at all: one segment per wave
    assert np.array_equal(got, bk.wave_inclusive(x, op))


def test_head_patterns_are_what_their_names_say():
    h = _head_flags()[:64 * WAVES_PER_PATTERN * len(HEAD_PATTERNS)].reshape(len(HEAD_PATTERNS), WAVES_PER_PATTERN, 64)
    by_name = dict(zip(HEAD_PATTERNS, h))
    assert not by_name["none"].any() and by_name["every_lane"].all()
    assert all(np.flatnonzero(w).tolist() == [0] for w in by_name["lane0"])
    for lane in BORDER_LANES[1:]:
        assert all(np.flatnonzero(w).tolist() == [lane] for w in by_name[lane])
    assert all(np.flatnonzero(w).tolist() == list(BORDER_LANES[1:]) for w in by_name["all_borders"])
    assert 0 < by_name["random_0.05"].sum() < 25 < 60 < by_name["random_0.5"].sum() < 130


@pytest.mark.parametrize("threads", THREADS)
def test_dpp_move_32_and_64_bit(threads):
    rng = np.random.default_rng(5)
    n = 64 * 40 + TAIL
    for dtype in (np.uint32, np.uint64):
        x = (rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)).astype(dtype)
        ident = ga.DPP_MOVE_IDENTITY & (2 ** (8 * np.dtype(dtype).itemsize) - 1)
        for step in range(bk.DPP_STEPS):
            got, want = ga.wave_ops("dpp_move", x, threads, step=step), bk.dpp_move(x, step, ident)
            assert np.array_equal(got, want), "step %d %s: first wrong lanes %s" % (step, np.dtype(dtype), np.flatnonzero(got != want)[:8] % 64)


@pytest.mark.parametrize("threads", THREADS)
def test_rank_in_mask(threads):
    rng = np.random.default_rng(6)
    full = rng.integers(0, 2 ** 63, 24, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 24, dtype=np.uint64)
    uniform = np.concatenate([full[:8] & np.uint64(0xFFFFFFFF),                                   # bits in the low word only
                              full[8:16] & np.uint64(0xFFFFFFFF00000000),                         # ... in the high word only
                              full[16:], [np.uint64(0), ALL_ONES, np.uint64(1), np.uint64(1) << np.uint64(63)]])   # ... in both
    per_lane = rng.integers(0, 2 ** 63, 64 * 8 + TAIL, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    masks = np.concatenate([np.repeat(uniform, 64), per_lane])       # a wave-uniform mask, as a ballot is; then one per lane
    assert masks.size > 2 * 1024
    assert np.array_equal(ga.wave_ops("rank_in_mask", masks, threads), bk.rank_in_mask(masks))


@pytest.mark.parametrize("threads", THREADS)
def test_block_scan_twice_on_the_same_storage(threads):
    rng = np.random.default_rng(7 + threads)
    n = 3 * threads + 77                                             # several workgroups and a partial one
    degree = rng.integers(0, 5000, n).astype(np.uint64)
    # PackTail(1, degree), and 0 for a thread without an entry, as FrontierWriter::Flush feeds it: both halves add independently
    packed = np.where(rng.random(n) < 0.8, (degree << np.uint64(32)) | np.uint64(1), np.uint64(0))
    for x in (rng.integers(-1000, 1000, n).astype(np.int32), packed):
        got = ga.wave_ops("block_scan", x, threads)
        want = bk.block_scan(x, threads)
        for name, a, b in zip(("first result", "first total", "second result", "second total"), got, want):
            assert np.array_equal(a, b), "BlockScan<%d, %s> %s" % (threads, x.dtype, name)
        for lo in range(0, n, threads):                              # the total is the same in every thread of a workgroup
            assert np.unique(got[1][lo:lo + threads]).size == 1 and np.unique(got[3][lo:lo + threads]).size == 1
    count, edges = want[0] & np.uint64(0xFFFFFFFF), want[0] >> np.uint64(32)
    assert count.max() > 0.5 * threads and edges.max() > 2 ** 16     # the halves carry a count and an edge total of their own


# ================================================================ near/far split ==========================================

BISECT_TILE, BISECT_FLUSH = 256 * 4, 1024
BISECT_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000, 300_000)
GRIDS = (1, 2, 3, 0)
UINT_MAX = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _split_graph(nodes):
    """row offsets only (the split reads nothing else): degrees 0..6, every seventh vertex without out-edges"""
    deg = (np.arange(nodes, dtype=np.int64) * 5 + 3) % 7
    ro = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ro.setflags(write=False)
    return ro


def _check_split(res, ro, near, far, far_min, lookup_after, near_capacity, far_capacity):
    """the issue of one call against the loop's (near vertices, far pairs, smallest far bucket, lookup afterwards)"""
    deg = np.diff(ro).astype(np.int64)
    assert res["overflow"] == 0
    near = np.asarray(near, dtype=np.int64)
    want_near = np.sort(near[deg[near] > 0]) if near.size else near  # Flush<true> drops vertices without out-edges
    k = res["near_len"]
    v = res["near_v"][:k].astype(np.int64)
    assert k == want_near.size and np.array_equal(np.sort(v), want_near), "near set as a multiset"
    assert np.array_equal(res["near_row_start"][:k], ro[v]), "row_start != row_offsets[v]"
    prefix = np.concatenate([[0], np.cumsum(deg[v])])
    assert np.array_equal(res["near_scan"][:k], prefix[:-1]), "scan is not the exclusive degree prefix in output order"
    assert res["near_edges"] == int(prefix[-1]), "the packed near tail is not (count, edge sum)"
    for name in ("near_v", "near_row_start", "near_scan"):
        assert res[name].size > near_capacity and (res[name][k:] == FILL).all(), "%s: written past the tail" % name
    f = res["far_len"]
    assert f == len(far), "far tail"
    got_far = sorted(zip(res["far_v"][:f].tolist(), res["far_d"][:f].tolist()))
    assert got_far == sorted(far), "far set as a multiset of (vertex, distance)"
    assert res["far_v"].size > far_capacity and (res["far_v"][f:] == FILL).all() and (res["far_d"][f:].view(np.int32) == FILL).all()
    assert res["far_min"] == far_min, "far_min"
    assert np.array_equal(res["visit_lookup"], lookup_after), "d_visit_lookup afterwards"


def _run_split(ro, dist, lookup, delta, queue, level, tag, parked=None, count=None, grid=0, mark_paths=False):
    n = queue.size
    want = bk.bisect(queue, n if count is None else count, dist, lookup, tag, delta, level, parked)
    res = ga.bisect_queue(ro, dist, lookup, delta, queue, level, tag, parked=parked, count_on_device=count, mark_paths=mark_paths,
                          max_grid_size=grid)
    _check_split(res, ro, *want, near_capacity=max(n, 1), far_capacity=max(n, 1))
    return res, want


@functools.lru_cache(maxsize=None)
def _mixed_case(n):
    """a queue as an advance leaves it: holes, duplicates, near and far vertices, vertices without out-edges"""
    rng = np.random.default_rng(n)
    nodes = max(64, n // 2)
    dist = rng.integers(0, 4000, nodes).astype(np.uint32)
    queue = rng.integers(0, nodes, n).astype(np.int32)
    queue[rng.random(n) < 0.2] = -1
    lookup = np.full(nodes, -1, dtype=np.int32)
    ro = _split_graph(nodes)
    want = bk.bisect(queue, n, dist, lookup, 9, 16.0, 100, None)
    return ro, dist, queue, lookup, want


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", BISECT_SIZES)
def test_bisect_sizes_and_grids(n, grid):
    ro, dist, queue, lookup, want = _mixed_case(n)
    res = ga.bisect_queue(ro, dist, lookup, 16.0, queue, 100, 9, max_grid_size=grid)
    _check_split(res, ro, *want, near_capacity=max(n, 1), far_capacity=max(n, 1))
    if n >= 1023:
        assert len(want[0]) > n // 20 and len(want[1]) > n // 20


def _distinct(n, nodes, seed):
    return np.random.default_rng(seed).permutation(nodes)[:n].astype(np.int32)


@pytest.mark.parametrize("n", [2049, 5000])
def test_bisect_all_near_with_one_workgroup(n):
    # grid 1: the one workgroup takes every tile, its staging buffer passes 1024 pending entries and flushes inside the loop
    nodes = n + 100
    ro, dist = _split_graph(nodes), np.full(nodes, 7, dtype=np.uint32)
    assert n > BISECT_TILE + BISECT_FLUSH
    res, want = _run_split(ro, dist, np.full(nodes, -1, dtype=np.int32), 1.0, _distinct(n, nodes, 1), 7, 1, grid=1)
    assert len(want[0]) == n and not want[1] and res["far_min"] == UINT_MAX and res["far_len"] == 0


@pytest.mark.parametrize("grid", [1, 0])
@pytest.mark.parametrize("n", [1025, 5000])
def test_bisect_all_far_all_holes_and_repeats(n, grid):
    nodes = n + 100
    ro, dist = _split_graph(nodes), (np.arange(nodes, dtype=np.uint32) % 1000) + 50
    fresh = np.full(nodes, -1, dtype=np.int32)
    res, want = _run_split(ro, dist, fresh, 1.0, _distinct(n, nodes, 2), 49, 1, grid=grid)                   # all far
    assert not want[0] and len(want[1]) == n and res["near_len"] == 0 and res["far_min"] == 50
    res, want = _run_split(ro, dist, fresh, 1.0, np.full(n, -1, dtype=np.int32), 49, 1, grid=grid)           # all -1
    assert not want[0] and not want[1] and res["far_min"] == UINT_MAX and (res["visit_lookup"] == -1).all()
    for v, level in ((13, 2000), (13, 0)):                                                                   # one vertex n times: near, far
        res, want = _run_split(ro, dist, fresh, 1.0, np.full(n, v, dtype=np.int32), level, 1, grid=grid)
        assert len(want[0]) + len(want[1]) == 1 and np.diff(ro)[v] > 0
    twice = np.random.default_rng(3).permutation(np.repeat(np.arange(n // 2, dtype=np.int32), 2))            # every vertex twice
    res, want = _run_split(ro, dist, fresh, 1.0, twice, 500, 1, grid=grid)
    assert len(want[0]) + len(want[1]) == n // 2 and want[0] and want[1]


def test_bisect_near_vertex_without_out_edges():
    nodes = 3000
    ro = _split_graph(nodes)
    zero = np.flatnonzero(np.diff(ro) == 0)
    assert zero.size > 400
    dist = np.full(nodes, 5, dtype=np.uint32)
    queue = np.arange(nodes, dtype=np.int32)                         # every vertex near; those without out-edges leave no entry
    res, want = _run_split(ro, dist, np.full(nodes, -1, dtype=np.int32), 0.0, queue, 5, 1, grid=2)
    assert res["near_len"] == nodes - zero.size and len(want[0]) == nodes
    res, want = _run_split(ro, dist, np.full(nodes, -1, dtype=np.int32), 0.0, zero.astype(np.int32), 5, 1, grid=0)
    assert res["near_len"] == 0 and res["near_edges"] == 0 and len(want[0]) == zero.size


@pytest.mark.parametrize("grid", [1, 0])
@pytest.mark.parametrize("staleness", ["all_fresh", "all_stale", "mixed"])
def test_bisect_parked_distances(staleness, grid):
    # a far pile re-split at a later level: an entry whose vertex improved since it was parked is dropped, not re-expanded
    n, nodes = 5000, 4000
    rng = np.random.default_rng(len(staleness))
    ro, dist = _split_graph(nodes), rng.integers(100, 3000, nodes).astype(np.uint32)
    queue = rng.integers(0, nodes, n).astype(np.int32)
    stale = {"all_fresh": np.zeros(n, dtype=bool), "all_stale": np.ones(n, dtype=bool), "mixed": rng.random(n) < 0.5}[staleness]
    parked = (dist[queue] + np.where(stale, rng.integers(1, 40, n), 0)).astype(np.uint32)   # parked with a larger distance
    res, want = _run_split(ro, dist, np.full(nodes, -1, dtype=np.int32), 16.0, queue, 90, 4, parked=parked, grid=grid)
    kept = len(want[0]) + len(want[1])
    if staleness == "all_stale":
        assert kept == 0 and (res["visit_lookup"] == -1).all()
    else:
        assert kept == np.unique(queue[~stale]).size and want[0] and want[1]


@pytest.mark.parametrize("delta", [0.0, 1.0, 16.0, 2.5])
def test_bisect_bucket_widths_and_levels(delta):
    n, nodes = 2049, 3000
    rng = np.random.default_rng(int(delta * 10))
    ro, dist = _split_graph(nodes), rng.integers(0, 1000, nodes).astype(np.uint32)
    dist[:40] = np.arange(40)                                        # every small distance: buckets on either side of each boundary
    queue = np.concatenate([np.arange(40), rng.integers(0, nodes, n - 40)]).astype(np.int32)
    top = max(bk.bucket_of(d, delta) for d in dist[queue].tolist())
    for level in (0, top // 3, top - 1, top):                        # level 0 ... the largest bucket: nothing is far any more
        res, want = _run_split(ro, dist, np.full(nodes, -1, dtype=np.int32), delta, queue, level, 2, grid=3)
        assert (level < top) == bool(want[1]) and (res["far_min"] == UINT_MAX) == (level == top)
        assert want[0] and (level == top or res["far_min"] == min(bk.bucket_of(d, delta) for _, d in want[1]) > level)
    at = [v for v in want[0] if bk.bucket_of(int(dist[v]), delta) == top]
    assert at, "a vertex whose bucket equals the level is near"


@pytest.mark.parametrize("grid", GRIDS)
def test_bisect_count_by_value_and_through_the_device_tail(grid):
    n, nodes = 5000, 6000
    ro, dist = _split_graph(nodes), np.full(nodes, 3, dtype=np.uint32)
    queue = _distinct(n, nodes, 4)
    fresh = np.full(nodes, -1, dtype=np.int32)
    by_value, _ = _run_split(ro, dist, fresh, 1.0, queue, 3, 1, grid=grid)
    assert by_value["near_len"] == np.count_nonzero(np.diff(ro)[queue] > 0)
    for count in (n, n - n // 3, 1025, 1, 0):                        # the queue's length is only the loose upper bound
        res, want = _run_split(ro, dist, fresh, 1.0, queue, 3, 1, count=count, grid=grid)
        assert len(want[0]) == count and np.count_nonzero(res["visit_lookup"] == 1) == count


@pytest.mark.parametrize("mark_paths", [False, True])
def test_bisect_two_calls_with_different_tags(mark_paths):
    # the second call works on the lookup the first one left: its marks are not this call's duplicates
    ro, dist, queue, lookup, _ = _mixed_case(5000)
    first, want1 = _run_split(ro, dist, lookup, 16.0, queue, 100, 1, grid=0, mark_paths=mark_paths)
    assert (first["visit_lookup"] == 1).sum() == len(want1[0]) + len(want1[1]) > 1000
    second, want2 = _run_split(ro, dist, first["visit_lookup"], 16.0, queue, 100, 2, grid=0, mark_paths=mark_paths)
    assert sorted(want2[0]) == sorted(want1[0]) and sorted(want2[1]) == sorted(want1[1])
    again, want3 = _run_split(ro, dist, second["visit_lookup"], 16.0, queue, 100, 2, grid=0, mark_paths=mark_paths)   # the same tag: all seen
    assert not want3[0] and not want3[1] and again["near_len"] == 0 and again["far_len"] == 0


@pytest.mark.parametrize("grid", [1, 0])
@pytest.mark.parametrize("short", ["near", "far"])
def test_bisect_a_queue_too_small_is_reported(short, grid):
    # FrontierWriter::Flush and the far append compare the reserved range with the capacity BEFORE the first store and skip the
    # stores when it does not fit: the flag is set, the call returns, nothing lands past the capacity
    n, nodes = 5000, 6000
    ro, dist = _split_graph(nodes), (np.arange(nodes, dtype=np.uint32) % 2) * 100
    queue = _distinct(n, nodes, 5)
    fresh = np.full(nodes, -1, dtype=np.int32)
    near, far, _, _ = bk.bisect(queue, n, dist, fresh, 1, 1.0, 0)
    need_near, need_far = int(np.count_nonzero(np.diff(ro)[near] > 0)), len(far)
    assert need_near > 1500 and need_far > 1500
    res = ga.bisect_queue(ro, dist, fresh, 1.0, queue, 0, 1, near_capacity=need_near, far_capacity=need_far, max_grid_size=grid)
    assert res["overflow"] == 0 and res["near_len"] == need_near and res["far_len"] == need_far        # exactly enough: fine
    for capacity in sorted({(need_near if short == "near" else need_far) - 1, 700, 0}):
        caps = {"near_capacity": need_near, "far_capacity": need_far}
        caps[short + "_capacity"] = capacity
        res = ga.bisect_queue(ro, dist, fresh, 1.0, queue, 0, 1, max_grid_size=grid, **caps)
        assert res["overflow"] == 1, "capacity %d" % capacity
        for name in ("near_v", "near_row_start", "near_scan"):
            assert res[name].size == caps["near_capacity"] + 64 and (res[name][caps["near_capacity"]:] == FILL).all(), name
        for name in ("far_v", "far_d"):
            assert res[name].size == caps["far_capacity"] + 64 and (res[name][caps["far_capacity"]:].view(np.int32) == FILL).all(), name
