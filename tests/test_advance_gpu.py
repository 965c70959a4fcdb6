"""The advance operator by itself (oprtr/advance/kernel.hpp: ExpandTiles, LaunchKernel, LaunchReduce) through the C ABI
(grx_advance_queue / grx_advance_reduce), with the library's KernelPolicy<256, 4, 8, LB>: a tile is 1024 edge slots, a stage
holds 256 frontier entries, a reduction run is one 64-lane row of slots.

Expected values come from tests/_advance_checker.py (numpy; itself checked against a double loop in test_advance_cpu.py).
Graphs are built from explicit degree sequences, so that every boundary of the tile machinery is hit on purpose (SHAPES
below), and each shape runs with 1, 2, 3 workgroups and with the resident grid (0).

The plain advance is checked exactly: every (frontier entry, edge) pair visited exactly once with the right source.  The
reducing advance is checked bit for bit wherever the result does not depend on the order of combination (all integer
operators; float MINIMUM / MAXIMUM; float PLUS of integer-valued terms whose partial sums stay below 2^24; float MULTIPLIES
of powers of two), and float PLUS of arbitrary terms against the float64 sum under the derived summation bound.

Not covered: the tile tag wrap of ExpandTiles (after 2^24 tiles of one workgroup = 2^34 edge slots) cannot be reached at
test size.
"""
import functools

import numpy as np
import pytest

import _advance_checker as ck

pytestmark = pytest.mark.gpu

ga = pytest.importorskip("gunrockinst_amd")

GRIDS = (1, 2, 3, 0)
TILE, STAGE, ROW = 1024, 256, 64


def _cycle(n, start=0):
    return [1 + (start + i) % 3 for i in range(n)]


def _degrees_summing_to(total, seed):
    rng = np.random.default_rng(seed)
    degs = []
    while sum(degs) < total:
        degs.append(int(min(rng.integers(1, 8), total - sum(degs))))
    return degs


# name -> degree sequence of the frontier, in frontier order (vertex i of the graph is entry i) unless FRONTIERS says otherwise
SHAPES = {}
for _n in (1, 63, 64, 65, 255, 256, 257, 4097):                 # frontier lengths around a wave, a stage, and many stages
    SHAPES["len%d" % _n] = _cycle(_n, _n)
for _s in (1, 1023, 1024, 1025, 2048, 2049):                    # edge slot totals around one and two tiles
    SHAPES["slots%d" % _s] = _degrees_summing_to(_s, _s)
SHAPES["ones300"] = [1] * 300 + _cycle(300)                      # a full stage of rows that begin inside the tile: the tile is cut
SHAPES["ones1000"] = [1] * 1000 + _cycle(600)                    # ... several times in a row
SHAPES["row64"] = [64, 65, 63, 64, 65, 127, 64, 1]               # lists of 64 / 65 that start ON a 64-slot row boundary
SHAPES["row64_shift"] = [1] + SHAPES["row64"]                    # ... and one slot behind it: whole-list store versus atomic
SHAPES["hub_mid"] = [3, 2, 5, 1, 5000, 2, 1, 3]                  # a list that begins mid-tile and spans five tiles
SHAPES["hub_only"] = [100_000]
SHAPES["hub_last"] = [2, 3, 1, 5000]                             # the frontier's last entry: its list ends with the slots
SHAPES["tile_end"] = [1000, 24, 5, 7] + [10] * 101 + [2, 4, 1, 1019, 6]   # lists that end exactly at a tile's last slot, more behind
SHAPES["deg2_100k"] = [2] * 100_000                              # the 64-ary cursor search over several rounds
FRONTIERS = {}


def _irregular(seed, n, hubs):
    rng = np.random.default_rng(seed)
    deg = np.minimum(rng.geometric(0.3, n), 40) * (rng.random(n) < 0.7)
    deg[rng.choice(n, hubs, replace=False)] = rng.integers(1500, 4000, hubs)
    return [int(d) for d in deg]


SHAPES["subset"] = _irregular(11, 3000, 2)                       # a strict subset of the vertices in shuffled order
_deg = np.array(SHAPES["subset"])
_rng = np.random.default_rng(12)
FRONTIERS["subset"] = [int(v) for v in _rng.permutation(np.flatnonzero(_deg > 0))[:1400]]
SHAPES["twice"] = [3, 70, 2, 1, 130, 5]                          # the same vertices twice (results by position only)
FRONTIERS["twice"] = [1, 4, 0, 1, 5, 4, 4, 2]
assert all(0 < sum(d) <= 210_000 for d in SHAPES.values())


@functools.lru_cache(maxsize=None)
def _graph(name):
    degs = SHAPES[name]
    nodes = len(degs) + max(8, len(degs) // 8)                   # the extra vertices have no out-edges: destinations only
    ro, ci = ck.graph_from_degrees(degs, seed=sum(map(ord, name)), nodes=nodes)
    frontier = np.array(FRONTIERS.get(name, range(len(degs))), dtype=np.int32)
    for a in (ro, ci, frontier):
        a.setflags(write=False)
    return ro, ci, frontier


@functools.lru_cache(maxsize=None)
def _mask(name, density):
    if density is None:
        return None
    ro, _, _ = _graph(name)
    m = (np.random.default_rng(int(density * 100) + len(name)).random(ro.size - 1) < density).astype(np.int32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _queue_ref(name, density):
    ro, ci, frontier = _graph(name)
    return ck.expected_queue(ro, ci, frontier, _mask(name, density))


def test_shapes_hit_their_boundaries():
    # the sequences above are only worth something if they put the boundaries where the comments say
    scan = {s: np.concatenate([[0], np.cumsum(np.array(SHAPES[s])[np.asarray(_graph(s)[2])])]) for s in SHAPES}
    assert [int(scan["len%d" % n].size - 1) for n in (1, 63, 64, 65, 255, 256, 257, 4097)] == [1, 63, 64, 65, 255, 256, 257, 4097]
    assert [int(scan["slots%d" % s][-1]) for s in (1, 1023, 1024, 1025, 2048, 2049)] == [1, 1023, 1024, 1025, 2048, 2049]
    assert scan["ones300"][STAGE] == STAGE and scan["ones1000"][3 * STAGE] == 3 * STAGE          # full stages of degree 1
    r = scan["row64"]
    assert r[0] % ROW == 0 and r[1] % ROW == 0 and r[4] % ROW == 0 and r[6] % ROW == 0           # 64, 65, 65, 64 start on a row
    assert SHAPES["row64"][0] == 64 and SHAPES["row64"][1] == 65 and SHAPES["row64"][4] == 65 and SHAPES["row64"][6] == 64
    h = scan["hub_mid"]
    assert 0 < h[4] < TILE and h[5] // TILE - h[4] // TILE == 4                                   # begins mid-tile, spans five tiles
    assert scan["hub_last"][-1] - scan["hub_last"][-2] == 5000
    t = scan["tile_end"]
    assert t[2] == TILE and 2 * TILE in t and 3 * TILE in t and t[-1] > 3 * TILE                  # lists end at slots 1023, 2047, 3071
    assert len(set(FRONTIERS["subset"])) == 1400 < np.count_nonzero(_deg)
    assert len(set(FRONTIERS["twice"])) < len(FRONTIERS["twice"])


# ---------------------------------------------------------------- plain advance -----------------------------------------

@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_mask_rule_visits_every_pair_once(name, grid):
    ro, ci, frontier = _graph(name)
    for density, functor in ((None, "plain"), (0.5, "hooked"), (0.5, "plain"), (None, "hooked")):
        want, hits, src = _queue_ref(name, density)
        got = ga.advance_queue(ro, ci, frontier, mode="ids", functor=functor, mask=_mask(name, density), max_grid_size=grid)
        assert got["out_len"] == want.size and got["out_edges"] == 0
        assert np.array_equal(np.sort(got["v"]), want), "accepted destinations differ as a multiset"
        assert np.array_equal(got["edge_hits"], hits), "an edge was applied too often, too rarely, or for the wrong row"
        assert np.array_equal(got["edge_src"], src), "ApplyEdge saw the wrong source vertex"
        assert (got["buffers"][0][want.size:] == -7).all()
        cnt = ga.advance_queue(ro, ci, frontier, mode="count", functor=functor, mask=_mask(name, density), max_grid_size=grid)
        assert cnt["out_len"] == want.size
        assert (cnt["buffers"][0] == -7).all(), "COUNT_ONLY wrote to the output queue"
        assert np.array_equal(cnt["edge_hits"], hits) and np.array_equal(cnt["edge_src"], src)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_claim_rule_enqueues_every_unlabelled_neighbour_once(name, grid):
    ro, ci, frontier = _graph(name)
    labels = np.where(np.random.default_rng(len(name)).random(ro.size - 1) < 0.5, -1, 2).astype(np.int32)
    won, after = ck.expected_claim(ro, ci, frontier, labels, 5)
    for functor in ("plain", "hooked"):
        got = ga.advance_queue(ro, ci, frontier, mode="ids", rule="claim", functor=functor, labels=labels, depth=5, max_grid_size=grid)
        assert np.array_equal(np.sort(got["v"]), won), "claimed vertices: not each unlabelled neighbour exactly once"
        assert np.array_equal(got["labels"], after)
        assert (got["edge_hits"].sum() == won.size) and (got["edge_hits"] <= 1).all()
        applied = np.flatnonzero(got["edge_hits"])
        assert np.array_equal(np.sort(ci[applied]), won)         # the winning edge of each vertex leads to it ...
        _, edge, src, _, _ = ck.slots(ro, ci, frontier)
        owner = np.full(ci.size, -1, dtype=np.int64)
        owner[edge] = src
        assert np.array_equal(got["edge_src"][applied], owner[applied])   # ... and was applied with its own row as the source


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_full_frontier_output(name, grid):
    ro, ci, frontier = _graph(name)
    assert (np.diff(ro) == 0).any()
    for density, functor in ((None, "plain"), (0.5, "hooked")):
        want, hits, _ = _queue_ref(name, density)
        got = ga.advance_queue(ro, ci, frontier, mode="frontier", functor=functor, mask=_mask(name, density), max_grid_size=grid)
        ck.check_full_frontier(ro, want, got["v"], got["row_start"], got["scan"], got["out_edges"])
        assert got["out_len"] == got["v"].size and np.array_equal(got["edge_hits"], hits)
    labels = np.where(np.random.default_rng(len(name) + 1).random(ro.size - 1) < 0.5, -1, 2).astype(np.int32)
    won, after = ck.expected_claim(ro, ci, frontier, labels, 1)
    got = ga.advance_queue(ro, ci, frontier, mode="frontier", rule="claim", labels=labels, depth=1, max_grid_size=grid)
    ck.check_full_frontier(ro, won, got["v"], got["row_start"], got["scan"], got["out_edges"])
    assert np.array_equal(got["labels"], after)


@pytest.mark.parametrize("mode", ["ids", "frontier"])
@pytest.mark.parametrize("name,grid", [("hub_mid", 1), ("hub_mid", 0), ("len4097", 2), ("row64", 3)])
def test_a_queue_too_small_is_reported(name, grid, mode):
    # FrontierWriter::Flush / FlushIds compare the reserved range with the capacity BEFORE the first store and return without
    # writing when it does not fit (frontier_writer.hpp), so a short queue is reported and nothing lands past its end:
    # the allocation is `capacity` entries and stays inside itself.
    ro, ci, frontier = _graph(name)
    want, _, _ = _queue_ref(name, None)
    needed = want.size if mode == "ids" else int(np.count_nonzero(np.diff(ro)[want] > 0))
    assert needed >= 1
    got = ga.advance_queue(ro, ci, frontier, mode=mode, capacity=needed, max_grid_size=grid)           # exactly enough: fine
    assert got["out_len"] == needed
    for capacity in sorted({needed - 1, needed // 2, 0}):
        with pytest.raises(RuntimeError):
            ga.advance_queue(ro, ci, frontier, mode=mode, capacity=capacity, max_grid_size=grid)


# ---------------------------------------------------------------- reducing advance --------------------------------------

DTYPES = {"int32": np.int32, "uint32": np.uint32, "float32": np.float32, "int64": np.int64, "uint64": np.uint64}
ARITH = ("plus", "multiplies", "maximum", "minimum")
BITS = ("bit_or", "bit_and", "bit_xor")
# what grx_advance_reduce instantiates (each for both r_types and both by_vertex settings)
COMBOS = ([(op, t) for t in ("int32", "uint32", "float32") for op in ARITH] + [(op, t) for t in ("int32", "uint32") for op in BITS] +
          [(op, t) for t in ("int64", "uint64") for op in ("plus", "maximum", "minimum")])
assert len(COMBOS) == 24


def _values(op, tname, name, r_type, seed):
    ro, ci, frontier = _graph(name)
    return _values_for(ro, ci, frontier, op, tname, r_type, np.random.default_rng(seed))


def _values_for(ro, ci, frontier, op, tname, r_type, rng):
    """values whose reduction does not depend on the order of combination, so every case is compared bit for bit:
    unsigned arithmetic wraps by definition; signed sums and products are kept inside their type; float sums are sums of
    small integers (partial sums below 2^24), float products are products of powers of two (every partial product a normal
    power of two), MINIMUM / MAXIMUM never round."""
    size = (ro.size - 1) if r_type == "vertex" else ci.size
    dtype = np.dtype(DTYPES[tname])
    if op == "multiplies":
        w = ck.max_row_multiplicity(ro, ci, frontier, r_type)
        if dtype.kind == "f":
            return ck.exact_product_values(w, rng)
        if dtype.kind == "u":
            return (rng.integers(0, 2 ** 31, size).astype(np.uint32) * 2 + 1).astype(dtype)            # odd: never collapses to 0
        return ck.sparse_values(w, rng, 18, [2, -2, 3, -3], [1, -1], dtype)                            # |product| <= 3^18 < 2^31
    if op == "plus":
        if dtype.kind == "f":
            return rng.integers(-8, 9, size).astype(dtype)                                             # 100 000 * 8 < 2^24
        if dtype.kind == "u":
            return rng.integers(0, 2 ** (8 * dtype.itemsize), size, dtype=np.uint64).astype(dtype)     # wraps: defined
        return rng.integers(-1000, 1001, size).astype(dtype) if dtype.itemsize == 4 else rng.integers(-2 ** 40, 2 ** 40, size).astype(dtype)
    if op in ("maximum", "minimum"):
        if dtype.kind == "f":
            x = (rng.standard_normal(size) * 1000).astype(dtype)
            x[x == 0] = 1                                                                              # (no -0 / +0 ties)
            return x
        if dtype.kind == "u":
            return rng.integers(0, 2 ** (8 * dtype.itemsize), size, dtype=np.uint64).astype(dtype)
        half = 2 ** (8 * dtype.itemsize - 1)
        return rng.integers(-half, half, size, dtype=np.int64).astype(dtype)                           # negative values included
    bits = 8 * dtype.itemsize
    one = (np.uint64(1) << rng.integers(0, bits, size).astype(np.uint64))
    if op == "bit_or":
        return np.where(rng.random(size) < 0.2, one, 0).astype(np.uint32).view(dtype)
    if op == "bit_and":
        return np.where(rng.random(size) < 0.2, ~one, ~np.uint64(0)).astype(np.uint32).view(dtype)
    return rng.integers(0, 2 ** bits, size, dtype=np.uint64).astype(np.uint32).view(dtype)


def _reduce_case(name, grid, op, tname, r_type, by_vertex, density, functor="plain", record=False):
    """one reducing advance with prefill against the checker, bit for bit"""
    ro, ci, frontier = _graph(name)
    values = _values(op, tname, name, r_type, seed=len(name) + len(op))
    mask = _mask(name, density)
    want, _, _, _ = ck.expected_reduce(ro, ci, frontier, values, r_type, op, mask, by_vertex)
    got = ga.advance_reduce(ro, ci, frontier, values, r_type=r_type, op=op, by_vertex=by_vertex, mask=mask, functor=functor,
                            record=record, max_grid_size=grid)
    bits = "u%d" % want.dtype.itemsize
    bad = np.flatnonzero(got["reduced"].view(bits) != want.view(bits))
    assert bad.size == 0, "%s %s %s by_vertex=%s %s grid %d: %d results differ, first at %d: got %r want %r" % (
        op, tname, r_type, by_vertex, name, grid, bad.size, bad[0], got["reduced"][bad[0]], want[bad[0]])
    if record:
        _, hits, src = _queue_ref(name, density)
        assert np.array_equal(got["edge_hits"], hits) and np.array_equal(got["edge_src"], src)


@pytest.mark.parametrize("by_vertex", [False, True])
@pytest.mark.parametrize("r_type", ["vertex", "edge"])
@pytest.mark.parametrize("op,tname", COMBOS)
def test_every_instantiated_reduction(op, tname, r_type, by_vertex):
    # three shapes that drive the reducer: whole-list stores next to straddling lists, a list over five tiles, cut tiles
    for name in ("row64_shift", "hub_mid", "ones300"):
        for grid in GRIDS:
            _reduce_case(name, grid, op, tname, r_type, by_vertex, 0.5 if grid in (2, 0) else None)


# per shape: one reduction of every kind of combine (native atomic, 64-bit atomic, compare-and-swap loop, float add)
SHAPE_COMBOS = [("plus", "int32", "vertex", False), ("minimum", "float32", "edge", True), ("maximum", "int64", "vertex", True),
                ("bit_xor", "uint32", "edge", False), ("multiplies", "float32", "vertex", False), ("plus", "float32", "edge", True)]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_reductions_on_every_shape(name, grid):
    for i, (op, tname, r_type, by_vertex) in enumerate(SHAPE_COMBOS):
        if name == "twice":
            by_vertex = False                                   # a vertex twice has a result per POSITION only
        _reduce_case(name, grid, op, tname, r_type, by_vertex, (None, 0.5)[i % 2], record=(i == 0))


@pytest.mark.parametrize("op,tname", [("plus", "int32"), ("minimum", "int32"), ("plus", "float32"), ("minimum", "float32")])
def test_reductions_with_the_hooked_functor(op, tname):
    for name in ("row64_shift", "hub_mid", "ones300", "twice"):
        for grid in GRIDS:
            _reduce_case(name, grid, op, tname, "vertex", False, 0.5, functor="hooked", record=True)
            if name != "twice":
                _reduce_case(name, grid, op, tname, "edge", True, None, functor="hooked", record=True)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", ["row64", "row64_shift", "hub_mid", "hub_last", "hub_only", "tile_end"])
def test_signed_64bit_extremes_over_lists_that_straddle_rows(name, grid):
    # every value negative: an unsigned comparison would rank them above the identity of MINIMUM and below nothing
    ro, ci, frontier = _graph(name)
    assert (np.array(SHAPES[name]) > ROW).any()                  # a list longer than a row of slots takes the atomic path
    rng = np.random.default_rng(grid)
    for r_type in ("vertex", "edge"):
        size = (ro.size - 1) if r_type == "vertex" else ci.size
        values = -rng.integers(1, 2 ** 62, size, dtype=np.int64)
        for op in ("minimum", "maximum"):
            want, _, _, _ = ck.expected_reduce(ro, ci, frontier, values, r_type, op)
            got = ga.advance_reduce(ro, ci, frontier, values, r_type=r_type, op=op, max_grid_size=grid)["reduced"]
            assert (want < 0).all() and np.array_equal(got, want), (op, r_type)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", ["len257", "row64_shift", "hub_mid", "hub_only", "tile_end", "deg2_100k", "subset", "twice"])
def test_float_plus_of_arbitrary_terms_within_the_summation_bound(name, grid):
    """Any order of adding deg float32 terms x_i differs from the exact sum by at most (deg - 1) * u * sum|x_i| to first order,
    u = 2^-24 (each of the deg - 1 additions rounds a partial sum no larger than sum|x_i|); the float64 reference is exact
    to far below that, and rounding the exact sum to float32 costs at most one ulp of the result.  Derived, not tuned."""
    ro, ci, frontier = _graph(name)
    rng = np.random.default_rng(len(name) + grid)
    for r_type, density in (("vertex", None), ("edge", 0.5)):
        size = (ro.size - 1) if r_type == "vertex" else ci.size
        values = rng.uniform(-1, 1, size).astype(np.float32)
        mask = _mask(name, density)
        _, ref, mags, degs = ck.expected_reduce(ro, ci, frontier, values, r_type, "plus", mask)
        got = ga.advance_reduce(ro, ci, frontier, values, r_type=r_type, op="plus", mask=mask, max_grid_size=grid)["reduced"]
        bound = np.maximum(degs - 1, 0) * 2.0 ** -24 * mags + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - ref)
        worst = int(np.argmax(err - bound))
        print("%s grid %d %s: worst error %.3e against bound %.3e (degree %d)" % (name, grid, r_type, err[worst], bound[worst], degs[worst]))
        assert (err <= bound).all()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("op,tname", [("plus", "float32"), ("maximum", "int32"), ("minimum", "uint64"), ("multiplies", "uint32"),
                                      ("bit_and", "int32"), ("maximum", "float32")])
def test_identity_placement_and_untouched_entries(op, tname, grid):
    name = "subset"
    ro, ci, frontier = _graph(name)
    dtype = np.dtype(DTYPES[tname])
    ident = ck.identity(op, dtype)
    values = _values(op, tname, name, "vertex", seed=3)
    n = ro.size - 1
    # every edge rejected: the identity, at frontier positions and at vertex ids
    none = np.zeros(n, dtype=np.int32)
    got = ga.advance_reduce(ro, ci, frontier, values, op=op, mask=none, max_grid_size=grid)["reduced"]
    assert got.size == frontier.size and (got == ident).all()
    # by vertex without prefill: the caller pre-set the frontier's entries; every other entry keeps the sentinel
    sentinel = dtype.type(77)
    assert sentinel != ident
    out = np.full(n, sentinel, dtype=dtype)
    out[frontier] = ident
    mask = _mask(name, 0.5)
    want, _, _, _ = ck.expected_reduce(ro, ci, frontier, values, "vertex", op, mask, by_vertex=True, out=out, prefill=False)
    got = ga.advance_reduce(ro, ci, frontier, values, op=op, mask=mask, by_vertex=True, out=out, prefill=False, max_grid_size=grid)["reduced"]
    assert np.array_equal(got, want)
    outside = np.setdiff1d(np.arange(n), frontier)
    assert outside.size > 0 and (got[outside] == sentinel).all() and (out[outside] == sentinel).all()
    # by position against by vertex: the same results, at positions / at vertex ids
    pos = ga.advance_reduce(ro, ci, frontier, values, op=op, mask=mask, max_grid_size=grid)["reduced"]
    assert np.array_equal(pos, got[frontier])
    # prefill of a prefix only: entries past out_len keep the sentinel unless the frontier writes them
    k = n // 2
    out = np.full(n, sentinel, dtype=dtype)
    out[frontier[frontier >= k]] = ident
    want, _, _, _ = ck.expected_reduce(ro, ci, frontier, values, "vertex", op, mask, by_vertex=True, out=out, out_len=k)
    got = ga.advance_reduce(ro, ci, frontier, values, op=op, mask=mask, by_vertex=True, out=out, out_len=k, max_grid_size=grid)["reduced"]
    assert np.array_equal(got, want) and (got[outside[outside >= k]] == sentinel).all() and (got[outside[outside < k]] == ident).all()


def test_a_combination_that_is_not_instantiated_is_an_error():
    ro, ci, frontier = _graph("row64")
    n = ro.size - 1
    for op, dtype, kw in (("minus", np.int32, {}), ("modulus", np.int32, {}), ("bit_or", np.float32, {}), ("multiplies", np.int64, {}),
                          ("bit_xor", np.uint64, {}), ("maximum", np.int32, {"functor": "hooked"}),
                          ("plus", np.float32, {"functor": "hooked", "by_vertex": True})):
        out = np.full(n, 5, dtype=dtype)
        with pytest.raises(RuntimeError):
            ga.advance_reduce(ro, ci, frontier, np.ones(n, dtype=dtype), op=op, out=out, **kw)


def _sweep_case(i):
    rng = np.random.default_rng(1000 + i)
    kind = ("ones", "small", "geometric", "hubs")[i % 4]
    n = int(rng.integers(200, 3000))
    if kind == "ones":
        deg = np.ones(n, dtype=np.int64)
    elif kind == "small":
        deg = rng.integers(1, 4, n)
    elif kind == "geometric":
        deg = np.minimum(rng.geometric(0.15, n), 200) * (rng.random(n) < 0.8)
    else:
        deg = rng.integers(0, 4, n)
        deg[rng.choice(n, int(rng.integers(1, 3)), replace=False)] = rng.integers(2000, 60_000)
    ro, ci = ck.graph_from_degrees(deg, seed=2000 + i, nodes=n + 16)
    live = np.flatnonzero(deg > 0)
    frontier = rng.permutation(live)[:int(rng.integers(1, live.size + 1))].astype(np.int32)
    op, tname = COMBOS[int(rng.integers(len(COMBOS)))]
    return dict(ro=ro, ci=ci, frontier=frontier, op=op, tname=tname, r_type=("vertex", "edge")[int(rng.integers(2))],
                by_vertex=bool(rng.integers(2)), grid=int(rng.choice([1, 2, 3, 0, 7, 64])), density=float(rng.choice([0.0, 0.5, 1.0])),
                rng=rng)


@pytest.mark.parametrize("i", range(40))
def test_random_sweep(i):
    c = _sweep_case(i)
    ro, ci, frontier, rng = c["ro"], c["ci"], c["frontier"], c["rng"]
    n = ro.size - 1
    mask = (rng.random(n) < c["density"]).astype(np.int32)
    want, hits, src = ck.expected_queue(ro, ci, frontier, mask)
    got = ga.advance_queue(ro, ci, frontier, mode="frontier", mask=mask, functor=("plain", "hooked")[i % 2], max_grid_size=c["grid"])
    ck.check_full_frontier(ro, want, got["v"], got["row_start"], got["scan"], got["out_edges"])
    assert np.array_equal(got["edge_hits"], hits) and np.array_equal(got["edge_src"], src)

    values = _values_for(ro, ci, frontier, c["op"], c["tname"], c["r_type"], rng)
    exp, _, _, _ = ck.expected_reduce(ro, ci, frontier, values, c["r_type"], c["op"], mask, c["by_vertex"])
    red = ga.advance_reduce(ro, ci, frontier, values, r_type=c["r_type"], op=c["op"], by_vertex=c["by_vertex"], mask=mask,
                            max_grid_size=c["grid"])["reduced"]
    u = "u%d" % exp.dtype.itemsize
    assert np.array_equal(red.view(u), exp.view(u)), (c["op"], c["tname"], c["r_type"], c["by_vertex"], c["grid"], c["density"])
