"""Restatements of per-edge triangle support and the k-truss decomposition (grx_truss_*), independent forms that must agree.

The CSR is read as an undirected simple graph: u and v are neighbours when either row holds the other, self-loops ignored,
unsorted rows, duplicates and one-way edges allowed.  Edges are numbered in the canonical order of _tc_checker.simple_edges:
(a, b) with a < b, sorted by (a, b).

  peel(...)         the synchronous peel in numpy over an explicit triangle list: per level k every live edge with support <= k - 2
                    leaves at once, every live triangle that holds a leaver dies and takes one off its edges that stay, repeat
                    until nobody is at the level; the next level is the smallest live support.  The triangles are indexed by
                    edge, so a sub-round touches only the triangles of its leavers
  sequential(...)   one edge at a time by smallest current support (a lazy heap), its triangles recounted over adjacency sets
                    (a different algorithm; a Python loop)
  by_networkx(...)  nx.k_truss(G, k).number_of_edges() for given k (None where networkx is absent)
"""
import heapq

import numpy as np

from _kcore_checker import clique_ladder, complete_bipartite, grid, path, star, _undirected  # noqa: F401
from _tc_checker import complete, csr_of, hub_and_cliques, simple_edges, _ranges  # noqa: F401


def triangles(nodes, a, b, chunk=1 << 22):
    """int64[T, 3]: the canonical edge ids of the three edges of every triangle, once.  Found through the degree orientation of
    _tc_checker.oriented (out-rows stay short on skewed graphs): an oriented edge (u, v) plus an out-neighbour w of v with
    (u, w) an oriented edge"""
    n, m = int(nodes), int(a.shape[0])
    if m == 0:
        return np.zeros((0, 3), dtype=np.int64)
    ckeys = a * n + b
    d = np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    a_first = d[a] <= d[b]
    okeys = np.sort(np.where(a_first, a, b) * n + np.where(a_first, b, a))
    src, dst = okeys // n, okeys % n
    oro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=oro[1:])
    lens = oro[dst + 1] - oro[dst]
    work = np.concatenate([[0], np.cumsum(lens)])
    out = []
    e0 = 0
    while e0 < m:
        e1 = int(np.searchsorted(work, work[e0] + chunk, side="right"))
        e1 = min(max(e1 - 1, e0 + 1), m)
        euv = np.repeat(np.arange(e0, e1, dtype=np.int64), lens[e0:e1])
        evw = _ranges(oro[dst[e0:e1]], lens[e0:e1])
        query = src[euv] * n + dst[evw]
        euw = np.minimum(np.searchsorted(okeys, query), m - 1)
        hit = okeys[euw] == query
        out.append(np.stack([euv[hit], evw[hit], euw[hit]], axis=1))
        e0 = e1
    tri = np.concatenate(out)
    canonical = np.searchsorted(ckeys, np.minimum(src, dst) * n + np.maximum(src, dst))  # oriented rank -> canonical id
    return canonical[tri]


def support_of(edges, tri):
    return np.bincount(tri.ravel(), minlength=edges).astype(np.int32)


def peel(nodes, row_offsets, col_indices):
    """(a, b, triangles int64[T, 3], support int32[M], truss int32[M], non-empty levels, sub-rounds)"""
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    m = int(a.shape[0])
    tri = triangles(n, a, b)
    support = support_of(m, tri)
    # the triangles of every edge
    flat = tri.ravel()
    order = np.argsort(flat, kind="stable")
    of_edge = order // 3
    ero = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=m), out=ero[1:])
    val = support.astype(np.int64)
    truss = np.zeros(m, dtype=np.int32)
    edge_alive = np.ones(m, dtype=bool)
    tri_alive = np.ones(tri.shape[0], dtype=bool)
    levels = sub_rounds = 0
    left = m
    while left:
        s = int(val[edge_alive].min())
        levels += 1
        leave = np.flatnonzero(edge_alive & (val <= s))
        while leave.shape[0]:
            sub_rounds += 1
            truss[leave] = s + 2
            edge_alive[leave] = False
            left -= int(leave.shape[0])
            dying = np.unique(of_edge[_ranges(ero[leave], ero[leave + 1] - ero[leave])])
            dying = dying[tri_alive[dying]]
            tri_alive[dying] = False
            stay = tri[dying].ravel()
            stay = stay[edge_alive[stay]]
            touched, counts = np.unique(stay, return_counts=True)
            val[touched] -= counts
            leave = touched[val[touched] <= s]
    return a, b, tri, support, truss, levels, sub_rounds


def sequential(nodes, row_offsets, col_indices):
    """truss int32[M]: edges taken one at a time by smallest current support"""
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    m = int(a.shape[0])
    adj = [set() for _ in range(n)]
    eid = {}
    for e, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
        adj[x].add(y)
        adj[y].add(x)
        eid[(x, y)] = e
    ends = list(zip(a.tolist(), b.tolist()))
    sup = [len(adj[x] & adj[y]) for x, y in ends]
    heap = [(s, e) for e, s in enumerate(sup)]
    heapq.heapify(heap)
    done = [False] * m
    truss = np.zeros(m, dtype=np.int32)
    k = 2
    while heap:
        s, e = heapq.heappop(heap)
        if done[e] or s != sup[e]:
            continue
        done[e] = True
        k = max(k, s + 2)
        truss[e] = k
        x, y = ends[e]
        for w in adj[x] & adj[y]:
            for p, q in ((x, w), (y, w)):
                f = eid[(p, q) if p < q else (q, p)]
                sup[f] -= 1
                heapq.heappush(heap, (sup[f], f))
        adj[x].discard(y)
        adj[y].discard(x)
    return truss


def by_networkx(nodes, row_offsets, col_indices, ks):
    """{k: edges of nx.k_truss(G, k)} for the given k, or None without networkx"""
    try:
        import networkx as nx
    except ImportError:
        return None
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(a.tolist(), b.tolist()))
    return {int(k): int(nx.k_truss(g, int(k)).number_of_edges()) for k in ks}


def classes(truss):
    """int64[max_truss + 1]: the edges of every truss number (one zero entry without an edge: max_truss = 0)"""
    truss = np.asarray(truss)
    return np.bincount(truss, minlength=int(truss.max()) + 1 if truss.shape[0] else 1).astype(np.int64)


def members(nodes, truss, a, b, k):
    """(mask uint8[M] truss >= k, its edges, the vertices at one of them)"""
    mask = np.asarray(truss) >= k
    at = np.zeros(int(nodes), dtype=bool)
    at[a[mask]] = True
    at[b[mask]] = True
    return mask.astype(np.uint8), int(mask.sum()), int(at.sum())


def vertex_truss(nodes, truss, a, b):
    out = np.zeros(int(nodes), dtype=np.int32)
    np.maximum.at(out, a, truss)
    np.maximum.at(out, b, truss)
    return out


def vertex_triangles(nodes, support, a, b):
    """triangles[v] = half the sum of support over the edges at v"""
    twice = np.bincount(a, weights=support, minlength=int(nodes)) + np.bincount(b, weights=support, minlength=int(nodes))
    return (twice.astype(np.int64)) // 2


# ---- generators: (nodes, row_offsets, col_indices), both directions stored ----

def _clique_edges(vertices):
    v = np.asarray(vertices, dtype=np.int64)
    r, c = np.nonzero(np.triu(np.ones((v.shape[0], v.shape[0]), dtype=bool), 1))
    return v[r], v[c]


def diamond():
    """K4 minus the edge (2, 3): five edges, all truss 3"""
    return _undirected(4, [0, 0, 0, 1, 1], [1, 2, 3, 2, 3])


def clique_with_pendant(q):
    """K_q on 0 .. q - 1 and a vertex q joined to 0 and 1: the clique's edges have truss q, the two pendant edges truss 3"""
    r, c = _clique_edges(np.arange(q))
    return _undirected(q + 1, np.concatenate([r, [0, 1]]), np.concatenate([c, [q, q]]))
