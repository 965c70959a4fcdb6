"""Restatements of the k-core decomposition (grx_kcore_*), independent forms that must agree.

The CSR is read as an undirected simple graph: u and v are neighbours when either row holds the other, self-loops ignored,
unsorted rows, duplicates and one-way edges allowed.

  peel(...)         the synchronous peel in numpy: per level k every live vertex with deg <= k leaves at once, a bincount of the
                    leavers' neighbours comes off the degrees, repeat until nobody is at the level; the next level is the
                    smallest live degree
  buckets(...)      the sequential Batagelj-Zaversnik algorithm: vertices bin-sorted by degree, taken in order, each taking one
                    off its larger neighbours and moving them one bin down (a different algorithm; a Python loop)
  by_networkx(...)  networkx.core_number (None where networkx is absent)
"""
import numpy as np

from _tc_checker import complete, csr_of, degrees, hub_and_cliques, neighbour_csr, simple_edges, _ranges  # noqa: F401


def peel(nodes, row_offsets, col_indices):
    """(core int32[n], degrees int64[n], non-empty levels, sub-rounds); the vertices without a neighbour are level 0, one sub-round"""
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    d = degrees(n, a, b)
    nro, nci = neighbour_csr(n, a, b)
    deg = d.copy()
    core = np.zeros(n, dtype=np.int32)
    alive = np.ones(n, dtype=bool)
    levels = sub_rounds = 0
    while alive.any():
        k = int(deg[alive].min())
        levels += 1
        while True:
            leave = np.flatnonzero(alive & (deg <= k))
            if leave.shape[0] == 0:
                break
            sub_rounds += 1
            core[leave] = k
            alive[leave] = False
            nb = nci[_ranges(nro[leave], nro[leave + 1] - nro[leave])]
            deg -= np.bincount(nb, minlength=n)
    return core, d, levels, sub_rounds


def buckets(nodes, row_offsets, col_indices):
    """core int32[n] by Batagelj and Zaversnik's O(m) algorithm"""
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    d = degrees(n, a, b)
    nro, nci = neighbour_csr(n, a, b)
    nro, nci = nro.tolist(), nci.tolist()
    deg = d.tolist()
    md = max(deg) if n else 0
    start = [0] * (md + 2)  # start[c]: where bin c begins in vert
    for x in deg:
        start[x + 1] += 1
    for c in range(1, md + 2):
        start[c] += start[c - 1]
    fill = start[:]
    vert, pos = [0] * n, [0] * n
    for v in range(n):
        pos[v] = fill[deg[v]]
        vert[pos[v]] = v
        fill[deg[v]] += 1
    for i in range(n):
        v = vert[i]
        for u in nci[nro[v]:nro[v + 1]]:
            if deg[u] > deg[v]:
                du, pu = deg[u], pos[u]
                pw = start[du]
                w = vert[pw]
                if u != w:  # u to the front of its bin, then the bin gives it up
                    pos[u], pos[w] = pw, pu
                    vert[pu], vert[pw] = w, u
                start[du] += 1
                deg[u] -= 1
    return np.array(deg, dtype=np.int32).reshape(n)


def by_networkx(nodes, row_offsets, col_indices):
    """core int32[n] from networkx.core_number, or None without networkx"""
    try:
        import networkx as nx
    except ImportError:
        return None
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(a.tolist(), b.tolist()))
    cn = nx.core_number(g)
    return np.array([cn[v] for v in range(n)], dtype=np.int32)


def members(core, a, b, k):
    """(mask uint8[n] core >= k, its vertices, the edges (a, b) with both ends in it)"""
    mask = np.asarray(core) >= k
    return mask.astype(np.uint8), int(mask.sum()), int((mask[a] & mask[b]).sum())


def shells(core):
    """int64[degeneracy + 1]: the vertices of every core number"""
    core = np.asarray(core)
    return np.bincount(core, minlength=int(core.max()) + 1 if core.shape[0] else 1).astype(np.int64)


# ---- generators: (nodes, row_offsets, col_indices), both directions stored ----

def _undirected(n, r, c):
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    ro, ci = csr_of(n, np.concatenate([r, c]), np.concatenate([c, r]))
    return n, ro, ci


def path(n):
    return _undirected(n, np.arange(n - 1), np.arange(1, n))


def cycle(n):
    return _undirected(n, np.arange(n), (np.arange(n) + 1) % n)


def star(n):
    """vertex 0 joined to the n - 1 others"""
    return _undirected(n, np.zeros(n - 1, np.int64), np.arange(1, n))


def grid(r, c):
    v = np.arange(r * c).reshape(r, c)
    return _undirected(r * c, np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]), np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()]))


def complete_bipartite(a, b):
    return _undirected(a + b, np.repeat(np.arange(a), b), a + np.tile(np.arange(b), a))


def clique_ladder(q):
    """disjoint cliques K_2 .. K_q, consecutive ones joined by one bridge edge (last vertex of K_j to first of K_{j+1}): the
    members of K_j have core j - 1, q - 1 distinct levels on 2 + 3 + .. + q vertices"""
    rows, cols, base, last = [], [], 0, -1
    for j in range(2, q + 1):
        r, c = np.nonzero(np.triu(np.ones((j, j), dtype=bool), 1))
        rows.append(base + r)
        cols.append(base + c)
        if last >= 0:
            rows.append(np.array([last]))
            cols.append(np.array([base]))
        last = base + j - 1
        base += j
    return _undirected(base, np.concatenate(rows), np.concatenate(cols))


def ladder_cores(q):
    return np.concatenate([np.full(j, j - 1, dtype=np.int32) for j in range(2, q + 1)])
