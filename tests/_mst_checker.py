"""Reference answer for the minimum spanning forest (numpy + Python, CPU).  TEST INFRASTRUCTURE: the CPU tests, the GPU tests
and tools/fuzz_mst.py compare the HIP primitive behind grx_mst_* with it.

The contract it restates: every CSR entry e = (u, v, w) with u != v is one undirected edge {u, v}; self-loops are ignored;
entries are ordered by (w as signed int32, then e).  Under that strict total order the forest is unique, and it is what
Kruskal returns when it takes the entries in that order."""
import numpy as np


def entry_rows(row_offsets):
    """row of every CSR entry"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    return np.repeat(np.arange(ro.shape[0] - 1, dtype=np.int64), np.diff(ro))


def kruskal(nodes, row_offsets, col_indices, weights):
    """(selected int32 0/1 per entry, total_weight, forest_edges)"""
    rows = entry_rows(row_offsets)
    cols = np.asarray(col_indices, dtype=np.int64)
    w = np.asarray(weights, dtype=np.int32)
    m = cols.shape[0]
    selected = np.zeros(m, dtype=np.int32)
    order = np.argsort(w, kind="stable")  # stable: equal weights stay in entry order, i.e. (w, e)
    order = order[rows[order] != cols[order]]
    parent = list(range(int(nodes)))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    us, vs = rows[order].tolist(), cols[order].tolist()
    total, count = 0, 0
    for k, e in enumerate(order.tolist()):
        a, b = find(us[k]), find(vs[k])
        if a != b:
            parent[a] = b
            selected[e] = 1
            total += int(w[e])
            count += 1
    return selected, total, count


def components(nodes, rows, cols):
    """number of connected components of the undirected graph with the given edge endpoints (scipy)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    g = coo_matrix((np.ones(rows.shape[0], dtype=np.int32), (rows, cols)), shape=(int(nodes), int(nodes))).tocsr()
    return int(connected_components(g, directed=True, connection="weak")[0])


def min_reduced_pairs(row_offsets, col_indices, weights):
    """the undirected simple graph underneath: one (lo, hi, min weight) per vertex pair, self-loops dropped -- what scipy's
    minimum_spanning_tree can be given (csr_matrix would SUM duplicates)"""
    rows = entry_rows(row_offsets)
    cols = np.asarray(col_indices, dtype=np.int64)
    w = np.asarray(weights, dtype=np.int64)
    keep = rows != cols
    lo, hi, w = np.minimum(rows, cols)[keep], np.maximum(rows, cols)[keep], w[keep]
    if lo.size == 0:
        return lo, hi, w
    key = lo * (int(hi.max()) + 1) + hi
    order = np.argsort(key, kind="stable")
    key, lo, hi, w = key[order], lo[order], hi[order], w[order]
    first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
    return lo[first], hi[first], np.minimum.reduceat(w, first)


def scipy_forest_weight(nodes, row_offsets, col_indices, weights):
    """total weight of a minimum spanning forest by scipy (weights must be positive: scipy reads 0 as "no edge")"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    lo, hi, w = min_reduced_pairs(row_offsets, col_indices, weights)
    assert (w > 0).all(), "scipy treats weight 0 as a missing edge"
    g = csr_matrix((w.astype(np.float64), (lo, hi)), shape=(int(nodes), int(nodes)))
    return int(round(minimum_spanning_tree(g).sum()))
