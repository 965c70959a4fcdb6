"""Numpy / pure-Python restatement of k-clique counting (grx_clique_*) and the closed forms it must agree with.

The CSR is read as an undirected simple graph: u and v are neighbours when either row holds the other, self-loops ignored,
unsorted rows, duplicates and one-way edges allowed.

  count(n, ro, ci, k)      neighbour sets of the simple graph (one Python int per vertex: the bits of its larger-id neighbours), then
                           recursion over ascending members; the order is by id, not the library's (rank, d, id)
  work_estimate(...)       sum over v and j = 1 .. k - 2 of C(d+(v), j) under the (d, id) orientation: at least the number of cliques
                           of 2 .. k - 1 vertices, which is the number of calls of count()'s recursion under any order
  complete_counts          K_n: total C(n, k), per vertex C(n - 1, k - 1)
  multipartite_counts      complete multipartite with parts p_1 .. p_t: total e_k(p), the elementary symmetric polynomial; a vertex of
                           part a gets e_(k-1) of the other parts
  union(...)               disjoint unions add
Grids, trees and bipartite graphs have no odd cycle or no triangle: all zeros for k >= 3.
"""
from math import comb

import numpy as np

from _tc_checker import csr_of, degrees, simple_edges


def _popcount(x):
    return bin(x).count("1")


def upper_sets(nodes, row_offsets, col_indices):
    """hi[v]: a Python int whose bit w is set iff w > v and {v, w} is an edge of the simple graph"""
    a, b = simple_edges(nodes, row_offsets, col_indices)
    hi = [0] * int(nodes)
    for x, y in zip(a.tolist(), b.tolist()):
        hi[x] |= 1 << y
    return hi


def count(nodes, row_offsets, col_indices, k):
    """(cliques int64[n], total): the k-cliques through every vertex and their number, k >= 2"""
    n, k = int(nodes), int(k)
    hi = upper_sets(n, row_offsets, col_indices)
    cl = [0] * n
    last = {}  # candidate set of a last level -> how often it came up: each of its bits closes that many cliques

    def rec(p, remain):
        if remain == 1:
            if p:
                last[p] = last.get(p, 0) + 1
            return _popcount(p)
        s = 0
        while p:
            low = p & -p
            p ^= low
            j = low.bit_length() - 1
            c = rec(p & hi[j], remain - 1)  # (p has lost every bit up to j; hi[j] holds larger ids only)
            cl[j] += c
            s += c
        return s

    total = 0
    for v in range(n):
        c = rec(hi[v], k - 1)
        cl[v] += c
        total += c
    for p, c in last.items():
        while p:
            low = p & -p
            p ^= low
            cl[low.bit_length() - 1] += c
    return np.array(cl, dtype=np.int64), total


def work_estimate(nodes, row_offsets, col_indices, k):
    n = int(nodes)
    a, b = simple_edges(n, row_offsets, col_indices)
    d = degrees(n, a, b)
    src = np.where(d[a] <= d[b], a, b)
    return sum(comb(int(r), j) for r in np.bincount(src, minlength=n) for j in range(1, int(k) - 1))


def elementary(parts, k):
    """e_k(parts)"""
    e = [1] + [0] * int(k)
    for p in parts:
        for j in range(int(k), 0, -1):
            e[j] += e[j - 1] * int(p)
    return e[int(k)]


def complete_counts(n, k):
    return np.full(n, comb(n - 1, k - 1), dtype=np.int64), comb(n, k)


def multipartite_counts(parts, k):
    parts = list(parts)
    per = [elementary(parts[:i] + parts[i + 1:], k - 1) for i in range(len(parts))]
    return np.repeat(np.array(per, dtype=np.int64), parts), elementary(parts, k)


# ---- graphs (CSRs as int32 arrays) ----

def mirrored(nodes, a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return csr_of(nodes, np.concatenate([a, b]), np.concatenate([b, a]))


def complete_graph(n):
    a, b = np.nonzero(np.triu(np.ones((n, n), dtype=bool), 1))
    return mirrored(n, a, b)


def multipartite_graph(parts):
    parts = list(parts)
    label = np.repeat(np.arange(len(parts)), parts)
    a, b = np.nonzero(np.triu(label[:, None] != label[None, :], 1))
    return int(label.shape[0]), mirrored(label.shape[0], a, b)


def union(graphs):
    """disjoint union of (n, (ro, ci)) graphs: (n, (ro, ci))"""
    base, ros, cis = 0, [np.zeros(1, np.int32)], []
    for n, (ro, ci) in graphs:
        ros.append(ro[1:] + ros[-1][-1])
        cis.append(ci + base)
        base += n
    return base, (np.concatenate(ros).astype(np.int32), np.concatenate(cis).astype(np.int32) if cis else np.zeros(0, np.int32))


def grid_graph(side):
    v = np.arange(side * side).reshape(side, side)
    a = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    b = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return side * side, mirrored(side * side, a, b)


def tree_graph(n, seed=0):
    rng = np.random.default_rng(seed)
    child = np.arange(1, n)
    parent = (rng.random(n - 1) * child).astype(np.int64)
    return n, mirrored(n, parent, child)


def bipartite_graph(left, right, p, seed=0):
    rng = np.random.default_rng(seed)
    a, b = np.nonzero(rng.random((left, right)) < p)
    return left + right, mirrored(left + right, a, left + b)
