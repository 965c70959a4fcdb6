"""CPU checker of the sparse product C = A B (no GPU, no scipy): two independent forms that must agree, and the host-side rules of
app/spgemm restated.

A matrix is (shape, offsets, cols, vals): CSR read as given -- duplicate entries add, a row in any order -- with int values, or None
for 1 each.  C is structural: (i, j) is stored when some k has A(i, k) and B(k, j) stored, also when the products cancel to 0.  Both
forms return {"offsets": int32, "cols": int32, "vals": int64, "shape"} with strictly ascending rows.
  dense   A.toarray() @ B.toarray() in int64 for the values, the product of the boolean structures for what is stored
  expand  every product (i, j, a b), stable-sorted by i cols + j, summed over the runs with np.add.reduceat"""
import numpy as np

AUTO, LANE, WAVE, BLOCK, GLOBAL = 0, 1, 2, 3, 4
SELF, TRANSPOSE, GIVEN = 0, 1, 2
REGIMES = ("lane", "wave", "block", "global")
WAVES = 4
INT_MAX = 2 ** 31 - 1
SATURATED = 2 ** 63 - 1


def matrix(shape, offsets, cols, vals=None):
    return ((int(shape[0]), int(shape[1])), np.asarray(offsets, dtype=np.int64), np.asarray(cols, dtype=np.int64),
            None if vals is None else np.asarray(vals, dtype=np.int64))


def from_coo(shape, rows, cols, vals=None):
    """CSR of the entries in the order given inside every row (a stable sort by row)"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    offsets = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=shape[0])))).astype(np.int32)
    return ((int(shape[0]), int(shape[1])), offsets, cols[order].astype(np.int32),
            None if vals is None else np.asarray(vals)[order].astype(np.int32))


def rows_of(m):
    return np.repeat(np.arange(m[0][0], dtype=np.int64), np.diff(np.asarray(m[1], dtype=np.int64)))


def values_of(m):
    return np.ones(len(m[2]), dtype=np.int64) if m[3] is None else np.asarray(m[3], dtype=np.int64)


def transpose(m):
    return from_coo((m[0][1], m[0][0]), np.asarray(m[2]), rows_of(m), None if m[3] is None else m[3])


def crop(m, rows, cols):
    """the first `rows` rows and `cols` columns of m: a rectangular matrix"""
    r, c = rows_of(m), np.asarray(m[2], dtype=np.int64)
    keep = (r < rows) & (c < cols)
    return from_coo((rows, cols), r[keep], c[keep], None if m[3] is None else np.asarray(m[3])[keep])


def shuffled(m, rng):
    """the same matrix, the entries of every row in a random order"""
    rows = rows_of(m)
    order = np.lexsort((rng.random(len(rows)), rows))
    return (m[0], np.asarray(m[1]), np.asarray(m[2])[order], None if m[3] is None else np.asarray(m[3])[order])


def toarray(m, structure=False):
    out = np.zeros(m[0], dtype=np.int64)
    np.add.at(out, (rows_of(m), np.asarray(m[2], dtype=np.int64)), 1 if structure else values_of(m))
    return out


def _csr(shape, stored, values):
    i, j = np.nonzero(stored)
    offsets = np.concatenate(([0], np.cumsum(stored.sum(axis=1)))).astype(np.int32)
    return {"offsets": offsets, "cols": j.astype(np.int32), "vals": values[i, j].astype(np.int64), "shape": shape}


def dense(a, b):
    shape = (a[0][0], b[0][1])
    stored = (toarray(a, True) > 0).astype(np.int64) @ (toarray(b, True) > 0).astype(np.int64) > 0
    return _csr(shape, stored, toarray(a) @ toarray(b))


def expand(a, b):
    shape = (a[0][0], b[0][1])
    bo = np.asarray(b[1], dtype=np.int64)
    ai, ak, av = rows_of(a), np.asarray(a[2], dtype=np.int64), values_of(a)
    lens = bo[ak + 1] - bo[ak] if len(ak) else np.zeros(0, dtype=np.int64)
    total = int(lens.sum())
    offsets = np.zeros(shape[0] + 1, dtype=np.int32)
    if total == 0:
        return {"offsets": offsets, "cols": np.zeros(0, np.int32), "vals": np.zeros(0, np.int64), "shape": shape}
    # product p of entry e of A: entry bo[k] + (p - start of e) of B
    starts = np.cumsum(lens) - lens
    e = np.repeat(np.arange(len(ak)), lens)
    at = bo[ak][e] + (np.arange(total) - starts[e])
    i, j, v = ai[e], np.asarray(b[2], dtype=np.int64)[at], av[e] * values_of(b)[at]
    key = i * max(shape[1], 1) + j
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    heads = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
    sums = np.add.reduceat(v, heads)
    ci, cj = key[heads] // max(shape[1], 1), key[heads] % max(shape[1], 1)
    offsets[1:] = np.cumsum(np.bincount(ci, minlength=shape[0]))
    return {"offsets": offsets, "cols": cj.astype(np.int32), "vals": sums.astype(np.int64), "shape": shape}


def same(got, ref, values=True):
    """None, or what differs first"""
    if tuple(got["shape"]) != tuple(ref["shape"]):
        return "shape %s != %s" % (got["shape"], ref["shape"])
    for name in ("offsets", "cols") + (("vals",) if values else ()):
        g, r = np.asarray(got[name]), np.asarray(ref[name])
        if g.dtype != r.dtype or not np.array_equal(g, r):
            return name
    return None


# ---------------- the rules of app/spgemm restated ----------------

def work(a, b):
    """w_i: the products of row i"""
    lens = np.diff(np.asarray(b[1], dtype=np.int64))
    out = np.zeros(a[0][0], dtype=np.int64)
    np.add.at(out, rows_of(a), lens[np.asarray(a[2], dtype=np.int64)])
    return out


def regime(w, strategy=AUTO, lane_max=64, table_slots=1024, block_slots=8192):
    if strategy <= LANE and w <= lane_max:
        return LANE
    r = max(strategy, WAVE)
    if r == WAVE and w > table_slots // 2:
        r = BLOCK
    if r == BLOCK and w > block_slots // 2:
        r = GLOBAL
    return r


def regime_stats(a, b, strategy=AUTO, lane_max=64, table_slots=1024, block_slots=8192):
    """the regime entries of SpgemmProblem.stats()"""
    out = {name + suffix: 0 for name in REGIMES for suffix in ("_rows", "_products")}
    for w in work(a, b).tolist():
        name = REGIMES[regime(w, strategy, lane_max, table_slots, block_slots) - 1]
        out[name + "_rows"] += 1
        out[name + "_products"] += w
    return out


def lds_bytes(slots, values, waves=1):
    """a slot: the int32 key, and the int64 sum in a pass with values"""
    return (12 if values else 4) * waves * slots


def slot_words(cols):
    """64-bit words of a workgroup slot of the GLOBAL regime: a sum per column, then a bit per column"""
    return cols + (cols + 63) // 64


def global_slots(grid, scratch_mib, cols):
    return max(1, min(grid, (scratch_mib << 20) // (8 * slot_words(max(cols, 1)))))


def bound(a, b):
    """max over i of the sum over the entries (i, k, a) of |a| times the sum of |b| over row k, saturating at 2^63 - 1"""
    babs = np.zeros(b[0][0], dtype=object)
    for k, v in zip(rows_of(b).tolist(), np.abs(values_of(b)).tolist()):
        babs[k] += v
    rows = [0] * a[0][0]
    for i, k, v in zip(rows_of(a).tolist(), np.asarray(a[2]).tolist(), np.abs(values_of(a)).tolist()):
        rows[i] = min(SATURATED, rows[i] + min(SATURATED, v * int(babs[k])))
    return max(rows) if rows else 0


def fits(nnz, max_row_products):
    return 0 <= nnz <= INT_MAX and 0 <= max_row_products <= INT_MAX
