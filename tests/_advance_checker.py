"""Numpy restatement of the advance operator (grx_advance_queue / grx_advance_reduce): what one advance over a given input
frontier must produce, stated without tiles, stages or waves.

The input frontier is a list of vertex ids (each with at least one out-edge, possibly repeated).  Its edge slots are the
out-edges of entry 0, then of entry 1, ...; `slots()` lists them as (entry, edge id, source, destination).

  expected_queue(...)     rule "mask": the accepted destinations (a multiset: one per accepted slot), how often ApplyEdge
                          must have run per edge, and the source it must have seen
  expected_claim(...)     rule "claim": the destinations that were unlabelled (each exactly once) and the labels afterwards
  check_full_frontier(..) invariants of an output written as a complete frontier
  expected_reduce(...)    per-entry reductions as segment reductions (ufunc.reduceat) in int64 / uint64 / float64, with the
                          operator's identity for entries whose every edge is rejected
"""
import numpy as np

OPS = ("plus", "multiplies", "maximum", "minimum", "bit_or", "bit_and", "bit_xor")
_UFUNC = {"plus": np.add, "multiplies": np.multiply, "maximum": np.maximum, "minimum": np.minimum, "bit_or": np.bitwise_or,
          "bit_and": np.bitwise_and, "bit_xor": np.bitwise_xor}


def graph_from_degrees(degrees, seed, nodes=None):
    """CSR with exactly the given out-degrees (vertex i has degrees[i]; vertices beyond the list have none), columns drawn
    uniformly from all `nodes` vertices with a fixed seed."""
    deg = np.asarray(degrees, dtype=np.int64)
    n = int(nodes if nodes is not None else deg.size)
    assert n >= deg.size and n >= 1
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=ro[1:deg.size + 1])
    ro[deg.size + 1:] = ro[deg.size]
    rng = np.random.default_rng(seed)
    ci = rng.integers(0, n, int(ro[-1]), dtype=np.int32)
    return ro.astype(np.int32), ci


def slots(row_offsets, col_indices, vertices):
    """(entry, edge, src, dst) of every edge slot of the frontier, in slot order, plus the exclusive degree prefix"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    v = np.asarray(vertices, dtype=np.int64)
    deg = ro[v + 1] - ro[v]
    assert (deg > 0).all(), "an advance frontier holds no vertex without out-edges"
    scan = np.concatenate([[0], np.cumsum(deg)])
    entry = np.repeat(np.arange(v.size, dtype=np.int64), deg)
    edge = ro[v][entry] + (np.arange(scan[-1], dtype=np.int64) - scan[:-1][entry])
    return entry, edge, v[entry], np.asarray(col_indices, dtype=np.int64)[edge], scan


def _accepted(dst, mask):
    if mask is None:
        return np.ones(dst.size, dtype=bool)
    return np.asarray(mask)[dst] != 0


def expected_queue(row_offsets, col_indices, vertices, mask=None):
    """rule "mask" -> (accepted destinations sorted, edge_hits per edge, edge_src per edge with -1 where never applied)"""
    entry, edge, src, dst, _ = slots(row_offsets, col_indices, vertices)
    ok = _accepted(dst, mask)
    m = np.asarray(col_indices).size
    hits = np.bincount(edge[ok], minlength=m).astype(np.int32)
    edge_src = np.full(m, -1, dtype=np.int32)
    edge_src[edge[ok]] = src[ok]                      # a repeated vertex writes the same source again
    return np.sort(dst[ok]).astype(np.int32), hits, edge_src


def expected_claim(row_offsets, col_indices, vertices, labels, depth):
    """rule "claim" -> (claimed vertices ascending, each once; labels afterwards)"""
    _, _, _, dst, _ = slots(row_offsets, col_indices, vertices)
    labels = np.asarray(labels, dtype=np.int32)
    won = np.unique(dst[labels[dst] == -1])
    after = labels.copy()
    after[won] = depth
    return won.astype(np.int32), after


def check_full_frontier(row_offsets, accepted, v, row_start, scan, out_edges):
    """an output written as a complete frontier: the accepted destinations that have out-edges, each with its row start, and
    the exclusive prefix of the degrees in OUTPUT order"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    deg = np.diff(ro)
    accepted = np.asarray(accepted, dtype=np.int64)
    want = accepted[deg[accepted] > 0]
    v = np.asarray(v, dtype=np.int64)
    assert np.array_equal(np.sort(v), np.sort(want)), "wrong multiset of enqueued vertices"
    assert np.array_equal(row_start, ro[v]), "row_start != row_offsets[v]"
    prefix = np.concatenate([[0], np.cumsum(deg[v])])
    assert np.array_equal(scan, prefix[:-1]), "scan is not the exclusive degree prefix in output order"
    assert int(out_edges) == int(prefix[-1]), "out_edges is not the degree total"


def identity(op, dtype):
    dtype = np.dtype(dtype)
    if op == "multiplies":
        return dtype.type(1)
    if op == "maximum":
        return np.finfo(dtype).min if dtype.kind == "f" else np.iinfo(dtype).min
    if op == "minimum":
        return np.finfo(dtype).max if dtype.kind == "f" else np.iinfo(dtype).max
    if op == "bit_and":
        return dtype.type(np.iinfo(dtype).max) if dtype.kind == "u" else dtype.type(-1)
    return dtype.type(0)


def _wide(dtype):
    dtype = np.dtype(dtype)
    return np.float64 if dtype.kind == "f" else (np.uint64 if dtype.kind == "u" else np.int64)


def segment_reduce(row_offsets, col_indices, vertices, values, r_type, op, mask=None):
    """per frontier ENTRY: (op over its accepted slots in the wide type, sum of |value| over them, degree).  Integer sums and
    products wrap modulo 2^64, so their low bits are those of the operator's native-width arithmetic."""
    entry, edge, _, dst, scan = slots(row_offsets, col_indices, vertices)
    values = np.asarray(values)
    wide = _wide(values.dtype)
    per_slot = values[dst if r_type == "vertex" else edge].astype(wide)
    ok = _accepted(dst, mask)
    per_slot = np.where(ok, per_slot, np.asarray(identity(op, values.dtype)).astype(wide))
    with np.errstate(over="ignore"):
        red = _UFUNC[op].reduceat(per_slot, scan[:-1])
    mag = np.add.reduceat(np.where(ok, np.abs(per_slot.astype(np.float64)), 0.0), scan[:-1])
    return red, mag, np.diff(scan)


def expected_reduce(row_offsets, col_indices, vertices, values, r_type, op, mask=None, by_vertex=False, out=None, prefill=True,
                    out_len=None):
    """the result array of a reducing advance in the values' own type, and for float values its float64 form with the
    per-position sum of magnitudes and degree (for the summation bound; positions outside the frontier: 0).
    `out` = the array's contents beforehand; prefill sets its first out_len entries to the identity first.  Entries of one
    frontier must have distinct positions (by_vertex: no vertex twice)."""
    values = np.asarray(values)
    v = np.asarray(vertices, dtype=np.int64)
    n_out = (np.asarray(row_offsets).size - 1) if by_vertex else v.size
    res = np.zeros(n_out, dtype=values.dtype) if out is None else np.array(out, dtype=values.dtype, copy=True)
    if prefill:
        res[:res.size if out_len is None else out_len] = identity(op, values.dtype)
    at = v if by_vertex else np.arange(v.size)
    assert np.unique(at).size == at.size, "two frontier entries share a result position"
    red, mag, deg = segment_reduce(row_offsets, col_indices, vertices, values, r_type, op, mask)
    wide = np.zeros(res.size, dtype=red.dtype)
    wide[:] = res.astype(red.dtype)
    wide[at] = red
    with np.errstate(over="ignore"):
        res[at] = red.astype(values.dtype)               # integers: the low bits; floats: exact in the bit-exact cases
    mags = np.zeros(res.size)
    degs = np.zeros(res.size, dtype=np.int64)
    mags[at] = mag
    degs[at] = deg
    return res, wide, mags, degs


def max_row_multiplicity(row_offsets, col_indices, vertices, r_type):
    """per value index (vertex or edge): the largest number of slots of ONE frontier entry that read it -- what bounds the
    exponent range of a product of powers of two"""
    entry, edge, _, dst, _ = slots(row_offsets, col_indices, vertices)
    idx = dst if r_type == "vertex" else edge
    size = (np.asarray(row_offsets).size - 1) if r_type == "vertex" else np.asarray(col_indices).size
    keys, counts = np.unique(entry * size + idx, return_counts=True)
    w = np.zeros(size, dtype=np.int64)
    np.maximum.at(w, keys % size, counts)
    return w


def sparse_values(weights, rng, budget, special, base, dtype):
    """values that are drawn from `base` except at entries drawn from `special`; the special entries are chosen so that the
    multiplicities with which ONE frontier entry can read them (`weights`, max_row_multiplicity) sum to at most `budget`:
    no product over an entry, in any association order, has more than `budget` special factors"""
    weights = np.asarray(weights, dtype=np.int64)
    vals = rng.choice(np.asarray(base, dtype=dtype), weights.size)
    order = rng.permutation(weights.size)
    chosen = order[np.cumsum(weights[order]) <= budget]
    vals[chosen] = rng.choice(np.asarray(special, dtype=dtype), chosen.size)
    return vals


def exact_product_values(weights, rng, budget=100):
    """float32 values from {0.5, 1, 2} whose product over any frontier entry is exact in EVERY association order: every
    partial product is a power of two within 2^-budget .. 2^budget, far inside float32's normal range"""
    return sparse_values(weights, rng, budget, [0.5, 2.0], [1.0], np.float32)
