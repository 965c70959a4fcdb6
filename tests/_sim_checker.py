"""CPU restatements of vertex similarity (grx_sim_*), two independent forms that must agree, a third witness and closed forms.

The CSR is read as an undirected simple graph: u and v are neighbours when either row holds the other, self-loops ignored, unsorted
rows, duplicates and one-way entries allowed.  d(v) is the degree, c(u, v) = |N(u) ^ N(v)|, c(u, u) = d(u).  A metric is the exact
fraction num / den of fraction(); den = 0 (an isolated endpoint) reports 0 / 0 and the score 0.0; the score is numpy's num / den.

  Dense(...)  c from the dense product A A over _tc_checker.simple_edges (float64 on BLAS, exact: no entry exceeds n < 2^53); the
              ranking by integer cross products (a comparison function).  For n up to about 2000.
  Sets(...)   c from one Python set per vertex; the ranking by fractions.Fraction keys.
  networkx    nx_pairs(): common_neighbors and jaccard_coefficient where networkx is installed.
Top-k: the candidates of u are the w != u with c(u, w) >= 1, without those in N(u) under skip_neighbors; ranked by score descending,
then id ascending; a row of k with ids -1 and everything else 0 beyond the end, count = min(k, candidates) and the candidates.
Wd(u) = the sum of d(v) over v in N(u): the wedges a top-k of u walks.
"""
from fractions import Fraction
from functools import cmp_to_key

import numpy as np

from _tc_checker import degrees, simple_edges

COMMON, JACCARD, OVERLAP, SORENSEN = 0, 1, 2, 3
METRICS = (COMMON, JACCARD, OVERLAP, SORENSEN)


def fraction(metric, c, du, dv):
    """(num, den) as Python ints"""
    c, du, dv = int(c), int(du), int(dv)
    if metric == COMMON:
        num, den = c, 1
    elif metric == JACCARD:
        num, den = c, du + dv - c
    elif metric == OVERLAP:
        num, den = c, min(du, dv)
    else:
        num, den = 2 * c, du + dv
    return (0, 0) if den == 0 else (num, den)


def score_of(num, den):
    """numpy's float64 num / den, 0.0 where den is 0"""
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _pairs_result(metric, cs, dus, dvs):
    fr = [fraction(metric, c, du, dv) for c, du, dv in zip(cs, dus, dvs)]
    num = np.array([f[0] for f in fr], dtype=np.int64)
    den = np.array([f[1] for f in fr], dtype=np.int64)
    return {"common": np.array(cs, dtype=np.int32), "num": num, "den": den, "score": score_of(num, den)}


def _topk_result(rows, k):
    """rows: per source the ranked list of (w, c, num, den), all candidates"""
    s = len(rows)
    out = {"ids": np.full((s, k), -1, dtype=np.int32), "common": np.zeros((s, k), dtype=np.int32), "num": np.zeros((s, k), dtype=np.int64),
           "den": np.zeros((s, k), dtype=np.int64), "count": np.zeros(s, dtype=np.int32), "candidates": np.zeros(s, dtype=np.int32)}
    for i, ranked in enumerate(rows):
        out["candidates"][i] = len(ranked)
        out["count"][i] = min(k, len(ranked))
        for j, (w, c, num, den) in enumerate(ranked[:k]):
            out["ids"][i, j], out["common"][i, j], out["num"][i, j], out["den"][i, j] = w, c, num, den
    out["score"] = score_of(out["num"], out["den"])
    return out


def _before(x, y):
    """the comparison of two candidates (w, c, num, den): the larger fraction by cross products, then the smaller id"""
    l, r = x[2] * y[3], y[2] * x[3]
    return -1 if l > r or (l == r and x[0] < y[0]) else 1


class Dense:
    def __init__(self, nodes, row_offsets, col_indices):
        n = self.n = int(nodes)
        self.a, self.b = simple_edges(n, row_offsets, col_indices)
        A = np.zeros((n, n), dtype=np.float64)
        A[self.a, self.b] = 1.0
        A[self.b, self.a] = 1.0
        self.A = A.astype(bool)
        self.C = (A @ A).astype(np.int64)  # C[u, u] = d(u)
        self.d = np.diag(self.C).copy()
        self.wd = (A @ self.d.astype(np.float64)).astype(np.int64)

    def pairs(self, u, v, metric):
        u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
        return _pairs_result(metric, self.C[u, v].tolist(), self.d[u].tolist(), self.d[v].tolist())

    def candidates(self, u, metric, skip_neighbors=False):
        """all candidates of u, ranked: (w, c, num, den)"""
        row = self.C[u].copy()
        row[u] = 0
        if skip_neighbors:
            row[self.A[u]] = 0
        du = int(self.d[u])
        cand = [(int(w), int(row[w])) + fraction(metric, row[w], du, self.d[w]) for w in np.flatnonzero(row).tolist()]
        return sorted(cand, key=cmp_to_key(_before))

    def topk(self, sources, k, metric, skip_neighbors=False):
        return _topk_result([self.candidates(int(u), metric, skip_neighbors) for u in sources], k)


class Sets:
    def __init__(self, nodes, row_offsets, col_indices):
        n = self.n = int(nodes)
        ro = np.asarray(row_offsets, dtype=np.int64).tolist()
        ci = np.asarray(col_indices, dtype=np.int64).tolist()
        self.N = [set() for _ in range(n)]
        for r in range(n):
            for c in ci[ro[r]:ro[r + 1]]:
                if c != r:
                    self.N[r].add(c)
                    self.N[c].add(r)
        self.wd = np.array([sum(len(self.N[v]) for v in self.N[u]) for u in range(n)], dtype=np.int64)

    def pairs(self, u, v, metric):
        u, v = [int(x) for x in u], [int(x) for x in v]
        return _pairs_result(metric, [len(self.N[x] & self.N[y]) for x, y in zip(u, v)], [len(self.N[x]) for x in u], [len(self.N[y]) for y in v])

    def candidates(self, u, metric, skip_neighbors=False):
        ends = {}
        for v in self.N[u]:
            for w in self.N[v]:
                if w != u and not (skip_neighbors and w in self.N[u]):
                    ends[w] = ends.get(w, 0) + 1
        cand = [(w, c) + fraction(metric, c, len(self.N[u]), len(self.N[w])) for w, c in ends.items()]
        return sorted(cand, key=lambda x: (-Fraction(x[2], x[3]), x[0]))

    def topk(self, sources, k, metric, skip_neighbors=False):
        return _topk_result([self.candidates(int(u), metric, skip_neighbors) for u in sources], k)


def same(got, want, keys=None):
    """every array of `want` (or of `keys`) equal in `got`: integers with array_equal, the score by its float64 bits; the name of the
    first that differs, or None"""
    for key in keys or want:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.shape != w.shape or g.dtype != w.dtype:
            return key + " (shape or dtype)"
        if key == "score":
            if g.tobytes() != w.tobytes():
                return key
        elif not np.array_equal(g, w):
            return key
    return None


def nx_pairs(nodes, row_offsets, col_indices, u, v):
    """(common int list, jaccard float list) by networkx, or None without it; jaccard of a pair without a neighbour is 0"""
    try:
        import networkx as nx
    except ImportError:
        return None
    a, b = simple_edges(int(nodes), row_offsets, col_indices)
    g = nx.Graph()
    g.add_nodes_from(range(int(nodes)))
    g.add_edges_from(zip(a.tolist(), b.tolist()))
    pairs = [(int(x), int(y)) for x, y in zip(u, v)]
    common = [len(list(nx.common_neighbors(g, x, y))) if x != y else g.degree(x) for x, y in pairs]
    jaccard = [p for _, _, p in nx.jaccard_coefficient(g, pairs)]
    return common, jaccard


# ---- the regimes, restated ----

AUTO, LANE, WAVE, BLOCK, GLOBAL = 0, 1, 2, 3, 4


def pair_regime(rows, strategy=AUTO, lane_max=64):
    return LANE if strategy <= LANE and rows <= lane_max else WAVE


def topk_regime(wd, strategy=AUTO, table_slots=1024, block_slots=8192):
    r = max(strategy, WAVE)
    if r == WAVE and wd > table_slots // 2:
        r = BLOCK
    if r == BLOCK and wd > block_slots // 2:
        r = GLOBAL
    return r


# ---- graphs: (n, rows, cols), every edge once (more in _c4_checker) ----

def star(m):
    """hub 0 and m leaves"""
    return 1 + m, np.zeros(m, np.int64), 1 + np.arange(m, dtype=np.int64)


def path(n):
    v = np.arange(n - 1, dtype=np.int64)
    return n, v, v + 1


def _fans(du, fans):
    """source 0 with the neighbours 1 .. du; per fan (c, leaves) one vertex joined to the first c of them and to `leaves` vertices of
    its own.  Returns (graph, the fans' ids): the fans are the only candidates of 0, c common neighbours and degree c + leaves each."""
    rows, cols, ids, at = [np.zeros(du, np.int64)], [1 + np.arange(du, dtype=np.int64)], [], 1 + du + len(fans)
    for i, (c, leaves) in enumerate(fans):
        w = 1 + du + i
        ids.append(w)
        rows += [np.full(c, w, np.int64), np.full(leaves, w, np.int64)]
        cols += [1 + np.arange(c, dtype=np.int64), at + np.arange(leaves, dtype=np.int64)]
        at += leaves
    return (at, np.concatenate(rows), np.concatenate(cols)), ids


def rational_tie():
    """(graph, first, second): the Jaccard candidates of source 0 are `first` with 2 / 6 and `second` with 1 / 3 -- equal, so the smaller
    id comes first.  d(0) = 2; 2 / (2 + 6 - 2) and 1 / (2 + 2 - 1)."""
    graph, (first, second) = _fans(2, [(2, 4), (1, 1)])
    return graph, first, second


def near_tie_m(start=3000):
    """the first m >= start for which m / (2 m + 1) > (m - 1) / (2 m - 1) -- the cross products differ by exactly 1 -- are one float32,
    whether the division is done in float32 or rounded from float64"""
    for m in range(start, 4 * start):
        assert m * (2 * m - 1) - (m - 1) * (2 * m + 1) == 1
        if np.float32(m) / np.float32(2 * m + 1) == np.float32(m - 1) / np.float32(2 * m - 1) and \
                np.float32(m / (2 * m + 1)) == np.float32((m - 1) / (2 * m - 1)) and m / (2 * m + 1) != (m - 1) / (2 * m - 1):
            return m
    raise AssertionError("no near tie found")


def near_tie():
    """(graph, first, second, m): the Jaccard candidates of source 0, d(0) = m, are `second` (the smaller id) with (m - 1) / (2 m - 1) and
    `first` with m / (2 m + 1): equal as float32, so a float comparison ranks them by id, the wrong way round"""
    m = near_tie_m()
    graph, (second, first) = _fans(m, [(m - 1, m - 1), (m, m + 1)])
    return graph, first, second, m
