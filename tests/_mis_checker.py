"""Host checker of the maximal independent set / greedy colourings (numpy only: no GPU, no oracle).

The input CSR is read as an undirected simple graph; vertices are ordered by key(v) = (prio(v), v); H(v) = the neighbours of v
with a larger key.  `prio_or_seed` is an int32 array of caller priorities (compared as signed) or an int seed (hashed, compared
as unsigned: prio(v) = fmix32((uint32)v + seed * 0x9E3779B9)).

  greedy(...)  the sequential pass over the vertices in descending key (a Python loop: small and medium graphs)
  verify(...)  vectorised: does `ids` satisfy the mode's equation at every vertex?  Each equation has exactly one solution
               (induction down the key order), so verify == True means ids == greedy(...) bit for bit.
"""
import numpy as np

SET, COLOR_ROUNDS, COLOR_FIRST_FIT = 0, 1, 2
MODES = (SET, COLOR_ROUNDS, COLOR_FIRST_FIT)


def fmix32(h):
    """MurmurHash3's 32-bit finaliser over a uint64 array holding uint32 values"""
    m = np.uint64(0xFFFFFFFF)
    h = h & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def priorities(nodes, prio_or_seed):
    """prio as int64, so signed caller priorities and unsigned hashes compare the same way"""
    if isinstance(prio_or_seed, (int, np.integer)):
        mul = np.uint64((int(prio_or_seed) * 0x9E3779B9) & 0xFFFFFFFF)
        return fmix32(np.arange(nodes, dtype=np.uint64) + mul).astype(np.int64)
    prio = np.asarray(prio_or_seed)
    assert prio.shape[0] == nodes
    return prio.astype(np.int32).astype(np.int64)


def ranks(nodes, prio_or_seed):
    """rank[v] = position of v in ascending key order"""
    prio = priorities(nodes, prio_or_seed)
    order = np.lexsort((np.arange(nodes), prio))
    rank = np.empty(nodes, dtype=np.int64)
    rank[order] = np.arange(nodes)
    return rank


def entry_rows(row_offsets):
    ro = np.asarray(row_offsets, dtype=np.int64)
    return np.repeat(np.arange(ro.shape[0] - 1, dtype=np.int64), np.diff(ro))


def higher(nodes, row_offsets, col_indices, prio_or_seed):
    """(hv, hu, rank): the simple undirected graph, every edge once, as (endpoint of the smaller key, endpoint of the larger key),
    sorted by (hv, hu).  u is in H(v) exactly when (v, u) is listed."""
    rank = ranks(nodes, prio_or_seed)
    rows = entry_rows(row_offsets)
    cols = np.asarray(col_indices, dtype=np.int64)
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    low = rank[rows] < rank[cols]
    hv, hu = np.where(low, rows, cols), np.where(low, cols, rows)
    pair = np.unique(hv * np.int64(nodes) + hu)
    return pair // nodes, pair % nodes, rank


def greedy(nodes, row_offsets, col_indices, prio_or_seed, mode):
    hv, hu, rank = higher(nodes, row_offsets, col_indices, prio_or_seed)
    start = np.searchsorted(hv, np.arange(nodes + 1))
    ids = np.zeros(nodes, dtype=np.int32)
    for v in np.argsort(-rank, kind="stable"):
        seen = ids[hu[start[v]:start[v + 1]]]  # all of H(v) comes earlier in the pass
        if mode == SET:
            ids[v] = 0 if (seen == 1).any() else 1
        elif mode == COLOR_ROUNDS:
            ids[v] = 1 + (int(seen.max()) if seen.shape[0] else 0)
        else:
            taken = set(seen.tolist())
            c = 1
            while c in taken:
                c += 1
            ids[v] = c
    return ids


def expected_from(nodes, hv, hu, mode, ids):
    """the right-hand side of the mode's equation at every vertex, computed from `ids` itself"""
    ids = np.asarray(ids).astype(np.int64)
    seen = ids[hu]
    if mode == SET:
        return (np.bincount(hv, weights=(seen == 1), minlength=nodes) == 0).astype(np.int64)
    start = np.searchsorted(hv, np.arange(nodes + 1))
    some = np.flatnonzero(start[1:] > start[:-1])  # vertices with a non-empty H
    if mode == COLOR_ROUNDS:
        out = np.ones(nodes, dtype=np.int64)
        if some.shape[0]:
            out[some] = 1 + np.maximum.reduceat(seen, start[some])
        return out
    # first-fit: the distinct colours of H(v) in ascending order; the first position j (from 0) whose colour is not j + 1
    # marks the gap j + 1; no such position: one more than their number
    big = np.int64(max(int(seen.max()) + 2, 2)) if seen.shape[0] else np.int64(2)
    pair = np.unique(hv * big + np.clip(seen, 0, big - 1))
    pv, pc = pair // big, pair % big
    pstart = np.searchsorted(pv, np.arange(nodes + 1))
    out = (pstart[1:] - pstart[:-1]) + 1
    index = np.arange(pv.shape[0]) - pstart[pv]
    gap = np.flatnonzero(pc != index + 1)
    first_v, first_at = np.unique(pv[gap], return_index=True)
    out[first_v] = index[gap[first_at]] + 1
    return out


def verify(nodes, row_offsets, col_indices, prio_or_seed, mode, ids, graph=None):
    """True when ids satisfies the mode's equation everywhere; `graph` = a higher(...) result to reuse across modes"""
    ids = np.asarray(ids)
    if ids.shape[0] != nodes:
        return False
    if mode == SET and not np.isin(ids, (0, 1)).all():
        return False
    if mode != SET and not (ids >= 1).all():
        return False
    hv, hu, _ = graph if graph is not None else higher(nodes, row_offsets, col_indices, prio_or_seed)
    return bool(np.array_equal(expected_from(nodes, hv, hu, mode, ids), ids.astype(np.int64)))


def reference_rounds(nodes, row_offsets, col_indices, prio_or_seed):
    """A literal restatement of the reference's synchronous iteration (mis_enactor.cuh:234-363, mis_functor.cuh:84-89) run to
    the end with distinct labels: every iteration, each uncoloured vertex takes the largest label among its uncoloured
    neighbours (MAX-reducing advance over a snapshot), and is coloured `iteration + 1` when its own label is at least that."""
    rank = ranks(nodes, prio_or_seed)  # distinct labels in key order
    rows = entry_rows(row_offsets)
    cols = np.asarray(col_indices, dtype=np.int64)
    keep = rows != cols
    a, b = np.concatenate([rows[keep], cols[keep]]), np.concatenate([cols[keep], rows[keep]])
    ids = np.full(nodes, -1, dtype=np.int32)
    iteration = 0
    while (ids < 0).any():
        live = (ids[a] < 0) & (ids[b] < 0)
        reduced = np.full(nodes, -1, dtype=np.int64)
        np.maximum.at(reduced, a[live], rank[b[live]])
        win = (ids < 0) & (rank >= reduced)
        ids[win] = iteration + 1
        iteration += 1
    return ids
