"""CPU answers for the multi-source BFS: three independent forms of depth[source][vertex] that must agree (a frontier-matrix BFS in
numpy, one bit column per source and one OR-reduction per level; scipy's csgraph.shortest_path(unweighted=True); networkx), numpy
restatements of the per-source and per-vertex summaries and of closeness in its one fixed formula, the literal of a graph over all
its sources, and the generators the tests share.  The CSR is read as a directed multigraph: duplicates and self-loops change
nothing, rows may be unsorted.  depth is int32, 0 at the source and -1 where unreachable, as the single-source BFS labels."""
import numpy as np

from _scc_checker import bowtie, complete_digraph, dicycle, dipath, from_edges  # noqa: F401 (the directed generators are shared)


def _arrays(ro, ci):
    return np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)


def depths(nodes, ro, ci, sources):
    """int32 [k, nodes] by a frontier-matrix BFS: 64 sources share a uint64 per vertex; a level ORs the frontier words of the
    in-neighbours of every vertex (edges sorted by target, one bitwise_or.reduceat)"""
    ro, ci = _arrays(ro, ci)
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    k = sources.shape[0]
    src = np.repeat(np.arange(nodes), np.diff(ro))
    order = np.argsort(ci, kind="stable")
    src, dst = src[order], ci[order]
    starts = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]]) if dst.shape[0] else np.zeros(0, np.int64)
    targets = dst[starts]
    out = np.full((k, nodes), -1, dtype=np.int32)
    for first in range(0, k, 64):
        batch = sources[first:first + 64]
        bit = np.arange(batch.shape[0], dtype=np.uint64)
        seen = np.zeros(nodes, dtype=np.uint64)
        np.bitwise_or.at(seen, batch, np.uint64(1) << bit)
        frontier = seen.copy()
        out[first + np.arange(batch.shape[0]), batch] = 0
        level = 0
        while frontier.any() and dst.shape[0]:
            level += 1
            got = np.zeros(nodes, dtype=np.uint64)
            got[targets] = np.bitwise_or.reduceat(frontier[src], starts)
            frontier = got & ~seen
            seen |= frontier
            at = np.flatnonzero(frontier)
            b, v = np.nonzero((frontier[at][None, :] >> bit[:, None]) & np.uint64(1))
            out[first + b, at[v]] = level
    return out


def by_scipy(nodes, ro, ci, sources):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    ro, ci = _arrays(ro, ci)
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    m = csr_matrix((np.ones(ci.shape[0], dtype=np.float64), ci.astype(np.int32), ro.astype(np.int32)), shape=(nodes, nodes))
    d = shortest_path(m, method="D", directed=True, unweighted=True, indices=np.unique(sources))
    d = d[np.searchsorted(np.unique(sources), sources)]
    return np.where(np.isinf(d), -1, d).astype(np.int32)


def by_networkx(nodes, ro, ci, sources):
    import networkx as nx
    ro, ci = _arrays(ro, ci)
    g = nx.DiGraph()
    g.add_nodes_from(range(nodes))
    g.add_edges_from(zip(np.repeat(np.arange(nodes), np.diff(ro)).tolist(), ci.tolist()))
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    out = np.full((sources.shape[0], nodes), -1, dtype=np.int32)
    for i, s in enumerate(sources.tolist()):
        found = nx.single_source_shortest_path_length(g, s)
        out[i, list(found.keys())] = list(found.values())
    return out


def source_summary(depth):
    """(reached int64, dist_sum int64, ecc int32) per source"""
    depth = np.asarray(depth)
    finite = depth >= 0
    return (finite.sum(axis=1).astype(np.int64), np.where(finite, depth, 0).sum(axis=1, dtype=np.int64),
            np.where(finite, depth, 0).max(axis=1).astype(np.int32))


def vertex_summary(depth):
    """(sources_reaching int32, in_dist_sum int64) per vertex"""
    depth = np.asarray(depth)
    finite = depth >= 0
    return finite.sum(axis=0).astype(np.int32), np.where(finite, depth, 0).sum(axis=0, dtype=np.int64)


def closeness(nodes, sources, sources_reaching, in_dist_sum, wf_improved=True):
    """The one formula (networkx.closeness_centrality on incoming distances): r = the sources other than v itself that reach v,
    r / in_dist_sum (0 where the sum is 0), times r / (nodes - 1) with wf_improved.  float64, in this order of operations."""
    own = np.bincount(np.asarray(sources, dtype=np.int64).reshape(-1), minlength=int(nodes))
    r = (np.asarray(sources_reaching, dtype=np.int64) - own).astype(np.float64)
    total = np.asarray(in_dist_sum, dtype=np.int64).astype(np.float64)
    c = np.zeros(int(nodes), dtype=np.float64)
    some = total > 0
    c[some] = r[some] / total[some]
    if wf_improved and nodes > 1:
        c *= r / (float(nodes) - 1.0)
    return c


def all_sources(nodes, ro, ci, chunk=512):
    """(reached, dist_sum, ecc, sources_reaching, in_dist_sum) with every vertex as a source, `chunk` rows of depths at a time"""
    reached, dist_sum, ecc = [], [], []
    reaching, in_dist_sum = np.zeros(nodes, dtype=np.int32), np.zeros(nodes, dtype=np.int64)
    for first in range(0, nodes, chunk):
        d = depths(nodes, ro, ci, np.arange(first, min(first + chunk, nodes)))
        r, s, e = source_summary(d)
        reached.append(r), dist_sum.append(s), ecc.append(e)
        a, b = vertex_summary(d)
        reaching += a
        in_dist_sum += b
    return np.concatenate(reached), np.concatenate(dist_sum), np.concatenate(ecc), reaching, in_dist_sum


def literal(nodes, ro, ci):
    """(n, entries, reachable ordered pairs excluding self, sum of all finite distances, largest eccentricity) over all sources"""
    reached, dist_sum, ecc, _, _ = all_sources(nodes, ro, ci)
    return int(nodes), int(np.asarray(ci).shape[0]), int(reached.sum()) - int(nodes), int(dist_sum.sum()), int(ecc.max())


# ---------------- generators: (nodes, row_offsets int32, col_indices int32) ----------------

def symmetric(nodes, a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return from_edges(nodes, np.concatenate([a, b]), np.concatenate([b, a]))


def path(n):
    v = np.arange(n - 1)
    return symmetric(n, v, v + 1)


def cycle(n):
    v = np.arange(n)
    return symmetric(n, v, (v + 1) % n) if n > 2 else path(n)


def star(leaves):
    """vertex 0 is the hub"""
    return symmetric(leaves + 1, np.zeros(leaves, dtype=np.int64), 1 + np.arange(leaves))


def complete(n):
    return complete_digraph(n)


def two_components(a, b):
    """an undirected path of `a` vertices and an undirected cycle of `b` vertices, no edge between them"""
    u, v = np.arange(a - 1), a + np.arange(b)
    return symmetric(a + b, np.concatenate([u, v]), np.concatenate([u + 1, a + (np.arange(b) + 1) % b]))

