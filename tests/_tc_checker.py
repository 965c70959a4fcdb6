"""Numpy restatements of triangle counting (grx_tc_*), two independent forms that must agree.

The CSR is read as an undirected simple graph: u and v are neighbours when either row holds the other, self-loops ignored,
unsorted rows, duplicates and one-way edges allowed.

  oriented(...)   orient every edge from the endpoint with the smaller (d, id) to the larger; a triangle is an oriented edge
                  (u, v) plus an out-neighbour w of v with (u, w) an oriented edge, tested by searchsorted over u * n + w keys
  by_matrix(...)  ((A A) o A).sum(axis=1) / 2 with scipy.sparse (None where scipy is absent)
"""
import numpy as np


def simple_edges(nodes, row_offsets, col_indices):
    """(a, b) int64 arrays, a < b, every edge of the simple undirected graph once, sorted by (a, b)"""
    n = int(nodes)
    ro = np.asarray(row_offsets, dtype=np.int64)
    ci = np.asarray(col_indices, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    keep = rows != ci
    lo, hi = np.minimum(rows[keep], ci[keep]), np.maximum(rows[keep], ci[keep])
    keys = np.unique(lo * n + hi)
    return keys // n, keys % n


def degrees(nodes, a, b):
    return np.bincount(a, minlength=nodes) + np.bincount(b, minlength=nodes)


def neighbour_csr(nodes, a, b):
    """the symmetric CSR of the simple graph, rows ascending"""
    src = np.concatenate([a, b])
    dst = np.concatenate([b, a])
    order = np.lexsort((dst, src))
    nro = np.zeros(nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=nodes), out=nro[1:])
    return nro, dst[order]


def _ranges(starts, lengths):
    """concatenation of arange(s, s + l) over the pairs"""
    total = int(lengths.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    ends = np.cumsum(lengths)
    return np.arange(total, dtype=np.int64) - np.repeat(ends - lengths, lengths) + np.repeat(starts, lengths)


def oriented(nodes, row_offsets, col_indices, chunk_wedges=1 << 22):
    """(triangles int64[n], total, degrees int64[n], the largest out-row, wedges checked)"""
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    d = degrees(n, a, b)
    a_first = d[a] <= d[b]  # a < b: equal degrees go by id
    src, dst = np.where(a_first, a, b), np.where(a_first, b, a)
    keys = np.sort(src * n + dst)
    src, dst = keys // n, keys % n
    m = keys.shape[0]
    oro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=oro[1:])
    out_len = np.diff(oro)
    tri = np.zeros(n, dtype=np.int64)
    total = 0
    checked = 0
    if m:
        work = np.concatenate([[0], np.cumsum(out_len[dst])])
        e0 = 0
        while e0 < m:
            e1 = int(np.searchsorted(work, work[e0] + chunk_wedges, side="right"))
            e1 = min(max(e1 - 1, e0 + 1), m)
            lens = out_len[dst[e0:e1]]
            edge = np.repeat(np.arange(e0, e1, dtype=np.int64), lens)
            w = dst[_ranges(oro[dst[e0:e1]], lens)]
            query = src[edge] * n + w
            at = np.minimum(np.searchsorted(keys, query), m - 1)
            hit = keys[at] == query
            checked += int(query.shape[0])
            total += int(hit.sum())
            tri += (np.bincount(src[edge][hit], minlength=n) + np.bincount(dst[edge][hit], minlength=n)
                    + np.bincount(w[hit], minlength=n))
            e0 = e1
    return tri, total, d, int(out_len.max()) if n else 0, checked


def by_matrix(nodes, row_offsets, col_indices):
    """(triangles int64[n], total) from the adjacency matrix, or None without scipy"""
    try:
        import scipy.sparse as sp
    except ImportError:
        return None
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    ones = np.ones(2 * a.shape[0], dtype=np.int64)
    A = sp.csr_matrix((ones, (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n))
    twice = np.asarray((A @ A).multiply(A).sum(axis=1)).ravel().astype(np.int64)
    assert not (twice & 1).any()
    tri = twice // 2
    assert int(tri.sum()) % 3 == 0
    return tri, int(tri.sum()) // 3


def clustering(tri, d, total):
    """(coefficients float64[n], transitivity): each one IEEE double division of two exactly representable integers"""
    tri = np.asarray(tri, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64)
    denom = d * (d - 1)
    coeff = np.zeros(tri.shape[0], dtype=np.float64)
    big = d >= 2
    coeff[big] = (2 * tri[big]).astype(np.float64) / denom[big].astype(np.float64)
    wedges = int((denom // 2).sum())
    transitivity = float(np.float64(3 * int(total)) / np.float64(wedges)) if wedges else 0.0
    return coeff, transitivity


def local_count(nro, nci, v, mark):
    """triangles[v] = 1/2 sum over u in N(v) of |N(u) ^ N(v)| from the neighbour CSR; mark: a zeroed bool[n] scratch"""
    nv = nci[nro[v]:nro[v + 1]]
    mark[nv] = True
    both = int(mark[nci[_ranges(nro[nv], nro[nv + 1] - nro[nv])]].sum())
    mark[nv] = False
    assert both % 2 == 0
    return both // 2


def csr_of(nodes, rows, cols):
    """CSR of the (row, col) tuples as given (no mirroring, no clean-up), rows in tuple order"""
    rows = np.asarray(rows, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    ro = np.zeros(nodes + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=nodes), out=ro[1:])
    return ro, np.asarray(cols, dtype=np.int32)[order]


def complete(n):
    r, c = np.nonzero(~np.eye(n, dtype=bool))
    return csr_of(n, r, c)


def hub_and_cliques(cliques=24, size=40, hub_degree=6000, seed=7):
    """cliques of `size` vertices, one hub joined to `hub_degree` vertices (all clique members first), and a long tail of
    leaves on the hub: out-rows from 0 to ~size, one vertex of huge degree and many triangles through it"""
    rng = np.random.default_rng(seed)
    n = 1 + max(cliques * size, hub_degree) + 64
    rows, cols = [], []
    for k in range(cliques):
        base = 1 + k * size
        r, c = np.nonzero(np.triu(np.ones((size, size), dtype=bool), 1))
        rows.append(base + r)
        cols.append(base + c)
    rows.append(np.zeros(hub_degree, dtype=np.int64))
    cols.append(1 + np.arange(hub_degree, dtype=np.int64))
    extra = rng.integers(1, n, (4 * n, 2))
    rows.append(extra[:, 0])
    cols.append(extra[:, 1])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    ro, ci = csr_of(n, np.concatenate([rows, cols]), np.concatenate([cols, rows]))
    return n, ro, ci
