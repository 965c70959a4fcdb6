"""CPU restatements of 4-cycle (butterfly) counting (grx_c4_*), two independent forms that must agree, and closed forms.

The CSR is read as an undirected simple graph: u and v are neighbours when either row holds the other, self-loops ignored, unsorted
rows, duplicates and one-way entries allowed.  A 4-cycle is four distinct vertices a, b, c, d with the edges ab, bc, cd, da, counted as
a subgraph (chords allowed: K_4 holds three).

  dense(...)   P = A A (2-paths).  cycles[v] = sum over w != v of C(P[v, w], 2): w is the vertex opposite v.  For an edge ab the
               cycles a-b-c-d are a neighbour c != a of b and a common neighbour d != b of a and c: (P A)[a, b] - d(a) - d(b) + 1.
               The products run in float64 on BLAS and are exact: no entry exceeds n^2 < 2^53.  For n up to about 2000.
  ranked(...)  the library's algorithm in plain Python dicts: rank by (degree, id); a wedge of u is u-v-w with v and w below u in
               rank; c(u, w) wedges end in w; every 4-cycle is a pair of wedges of its highest-ranked vertex with the same end.  Also
               gives W(u), the wedges and the overflow bound sum of W(u) (dlow(u) - 1) / 2.
Both return per-vertex counts, per-edge counts in the canonical edge order of _tc_checker.simple_edges, and the total, as int64.
"""
from math import comb

import numpy as np

from _tc_checker import csr_of, degrees, simple_edges


def dense(nodes, row_offsets, col_indices):
    """(cycles int64[n], edge_cycles int64[M], total)"""
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    A = np.zeros((n, n), dtype=np.float64)
    A[a, b] = 1.0
    A[b, a] = 1.0
    P = A @ A
    d = np.diag(P).astype(np.int64)
    assert n * n < 2 ** 53
    Q = P @ A
    np.fill_diagonal(P, 0.0)
    Pi = P.astype(np.int64)
    cycles = (Pi * (Pi - 1) // 2).sum(axis=1)
    edge = Q[a, b].astype(np.int64) - d[a] - d[b] + 1
    assert int(cycles.sum()) % 4 == 0
    return cycles, edge, int(cycles.sum()) // 4


def ranked(nodes, row_offsets, col_indices):
    """{"cycles", "edge_cycles", "total", "W" (per vertex, by original id), "dlow", "wedges", "bound", "src", "dst"}"""
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    d = degrees(n, a, b)
    order = np.lexsort((np.arange(n), d))  # by (degree, id)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    rows = [[] for _ in range(n)]  # by rank: (neighbour's rank, edge id), ascending
    for e, (x, y) in enumerate(zip(rank[a].tolist(), rank[b].tolist())):
        rows[x].append((y, e))
        rows[y].append((x, e))
    for r in rows:
        r.sort()
    cycles, edge = [0] * n, [0] * a.shape[0]
    W, dlow = [0] * n, [0] * n
    total, bound = 0, 0.0
    for u in range(n):
        lower = [(v, e) for v, e in rows[u] if v < u]
        dlow[u] = len(lower)
        ends = {}
        wedges = []
        for v, e_uv in lower:
            for w, e_vw in rows[v]:
                if w >= u:
                    break
                ends[w] = ends.get(w, 0) + 1
                wedges.append((v, e_uv, w, e_vw))
        W[u] = len(wedges)
        if lower:
            bound += W[u] * (len(lower) - 1) / 2.0
        for v, e_uv, w, e_vw in wedges:
            c = ends[w]
            cycles[v] += c - 1
            edge[e_uv] += c - 1
            edge[e_vw] += c - 1
        for w, c in ends.items():
            pairs = c * (c - 1) // 2
            cycles[u] += pairs
            cycles[w] += pairs
            total += pairs
    by_id = lambda x: np.asarray(x, dtype=np.int64)[rank]
    return {"cycles": by_id(cycles), "edge_cycles": np.asarray(edge, dtype=np.int64), "total": total, "W": by_id(W), "dlow": by_id(dlow),
            "wedges": int(sum(W)), "bound": bound, "src": a, "dst": b}


# ---- graphs: (n, rows, cols), every edge once ----

def mirrored(graph):
    """(n, ro, ci) of the clean symmetric CSR"""
    n, r, c = graph
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    ro, ci = csr_of(n, np.concatenate([r, c]), np.concatenate([c, r]))
    return n, ro, ci


def union(*graphs):
    """the disjoint union, vertices renumbered in order"""
    rows, cols, base = [], [], 0
    for n, r, c in graphs:
        rows.append(np.asarray(r, dtype=np.int64) + base)
        cols.append(np.asarray(c, dtype=np.int64) + base)
        base += n
    return base, np.concatenate(rows), np.concatenate(cols)


def complete_bipartite(p, q):
    r, c = np.nonzero(np.ones((p, q), dtype=bool))
    return p + q, r, p + c


def complete(n):
    r, c = np.nonzero(np.triu(np.ones((n, n), dtype=bool), 1))
    return n, r, c


def hypercube(d):
    v = np.arange(1 << d, dtype=np.int64)
    r = np.concatenate([v[(v >> k) & 1 == 0] for k in range(d)]) if d else v[:0]
    c = np.concatenate([v[(v >> k) & 1 == 0] | (1 << k) for k in range(d)]) if d else v[:0]
    return 1 << d, r, c


def grid(p, q):
    idx = np.arange(p * q, dtype=np.int64).reshape(p, q)
    return p * q, np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]), np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])


def theta(t):
    """two poles (0 and 1) joined by t paths of length 2: C(t, 2) 4-cycles"""
    mid = 2 + np.arange(t, dtype=np.int64)
    return 2 + t, np.concatenate([np.zeros(t, np.int64), np.ones(t, np.int64)]), np.concatenate([mid, mid])


def spider(t):
    """a centre (0) with t legs of length 2: a tree"""
    knee = 1 + np.arange(t, dtype=np.int64)
    return 1 + 2 * t, np.concatenate([np.zeros(t, np.int64), knee]), np.concatenate([knee, knee + t])


def cycle(n):
    v = np.arange(n, dtype=np.int64)
    return n, v, (v + 1) % n


def petersen():
    v = np.arange(5, dtype=np.int64)
    return 10, np.concatenate([v, v, 5 + v]), np.concatenate([(v + 1) % 5, 5 + v, 5 + (v + 2) % 5])


def random_tree(n, seed):
    rng = np.random.default_rng(seed)
    child = np.arange(1, n, dtype=np.int64)
    return n, (rng.random(n - 1) * child).astype(np.int64), child


def edgeless(n):
    return n, np.zeros(0, np.int64), np.zeros(0, np.int64)


# ---- closed forms: (total, per vertex or None, per edge or None) ----

def complete_bipartite_counts(p, q):
    per_vertex = np.array([(p - 1) * comb(q, 2)] * p + [(q - 1) * comb(p, 2)] * q, dtype=np.int64)
    return comb(p, 2) * comb(q, 2), per_vertex, np.full(p * q, (p - 1) * (q - 1), dtype=np.int64)


def complete_counts(n):
    return 3 * comb(n, 4), np.full(n, 3 * comb(n - 1, 3), dtype=np.int64), np.full(comb(n, 2), 2 * comb(max(n - 2, 0), 2), dtype=np.int64)


def hypercube_counts(d):
    return (comb(d, 2) << d) // 4, np.full(1 << d, comb(d, 2), dtype=np.int64), np.full(d << (d - 1) if d else 0, d - 1, dtype=np.int64)


def grid_total(p, q):
    return (p - 1) * (q - 1)


def theta_total(t):
    return comb(t, 2)


def entry_forms(graph, rng):
    """the same simple graph as CSRs of different entry lists: {"mirrored", "one-way", "shuffled", "dirty"}"""
    n, r, c = graph
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    both_r, both_c = np.concatenate([r, c]), np.concatenate([c, r])
    flip = rng.random(r.shape[0]) < 0.5
    shuffle = rng.permutation(both_r.shape[0])
    dup = rng.integers(0, max(r.shape[0], 1), r.shape[0] // 3 + 1 if r.shape[0] else 0)
    loops = rng.integers(0, n, n // 4 + 1)
    return {"mirrored": csr_of(n, both_r, both_c),
            "one-way": csr_of(n, np.where(flip, c, r), np.where(flip, r, c)),
            "shuffled": csr_of(n, both_r[shuffle], both_c[shuffle]),
            "dirty": csr_of(n, np.concatenate([loops, both_r, c[dup], loops]), np.concatenate([loops, both_c, r[dup], loops]))}
