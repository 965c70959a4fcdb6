"""CPU checker of the neighbourhood sampling (grx_sample_*), in two independent forms of the definition in
include/gunrock/gunrock_mi355x.h:

scalar(...)      the definition transcribed into plain Python: one hop after the other, one frontier vertex after the other, one slot
                 after the other; _rw_checker's own splitmix64 in Python integers, the earlier picks of a row in a list, the local ids
                 in a dict, the new vertices of a hop in a set.
vectorised(...)  numpy, a hop at a time: the draws of all rows and slots from ga.rw_draw as one matrix, the collision rule one slot at a
                 time over all rows, the weighted choice as one searchsorted over the running sum of ALL sorted weights, the new
                 vertices by np.unique, the local ids in an array.

Both return {"vertices", "vertex_ptr", "offsets", "cols", "eids", "edge_ptr"}.  `weights` are what Init was given (they order the
rows even when the picks do not consult them); `weighted` is the option.  Not a test module."""
import numpy as np

import gunrockinst_amd as ga
import _rw_checker as rk

KEYS = ("vertices", "vertex_ptr", "offsets", "cols", "eids", "edge_ptr")

# generators: _rw_checker's
csr, path, star, complete, cycle_with_tail, gnp, row_col_weights, shuffled_rows = (
    rk.csr, rk.path, rk.star, rk.complete, rk.cycle_with_tail, rk.gnp, rk.row_col_weights, rk.shuffled_rows)


def sorted_copy(n, ro, ci, w):
    """every row sorted by (column, weight, entry): (ro, columns, weights, entries)"""
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    wt = np.zeros(ci.shape[0], dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    order = np.lexsort((np.arange(ci.shape[0]), wt, ci, rows))
    return ro, ci[order], wt[order], order.astype(np.int64)


def floyd(seed, v, hop, d, f):
    """the picks of a row of d > f entries without replacement, plain integers"""
    picks = []
    for s in range(f):
        i = d - f + s
        t = ((rk.draw(seed, v, hop, s) >> 32) * (i + 1)) >> 32
        picks.append(i if t in picks else t)
    return picks


def _pack(vertices, vertex_ptr, offsets, cols, eids, edge_ptr):
    return {"vertices": np.asarray(vertices, dtype=np.int32), "vertex_ptr": np.asarray(vertex_ptr, dtype=np.int64),
            "offsets": np.asarray(offsets, dtype=np.int64), "cols": np.asarray(cols, dtype=np.int32), "eids": np.asarray(eids, dtype=np.int32),
            "edge_ptr": np.asarray(edge_ptr, dtype=np.int64)}


# ---------------- the scalar form ----------------

def scalar(n, ro, ci, seeds, fanouts, weights=None, replace=False, weighted=False, seed=0):
    assert not (weighted and not replace) and not (weighted and weights is None)
    ro, sci, sw, sent = sorted_copy(n, ro, ci, weights)
    ro, sci, sw, sent = [int(x) for x in ro], [int(x) for x in sci], [int(x) for x in sw], [int(x) for x in sent]

    def picks_of(v, hop, f):
        b, d = ro[v], ro[v + 1] - ro[v]
        if f == -1:
            return list(range(d))
        if not replace:
            return list(range(d)) if d <= f else floyd(seed, v, hop, d, f)
        if d == 0:
            return []
        if not weighted:
            return [((rk.draw(seed, v, hop, s) >> 32) * d) >> 32 for s in range(f)]
        prefix, run = [], 0
        for i in range(b, b + d):
            run += sw[i]
            prefix.append(run)
        if run == 0:
            return []
        out = []
        for s in range(f):
            t = (rk.draw(seed, v, hop, s) * run) >> 64
            lo, hi = 0, d - 1
            while lo < hi:
                mid = (lo + hi) // 2
                if prefix[mid] > t:
                    hi = mid
                else:
                    lo = mid + 1
            out.append(lo)
        return out

    vertices = [int(s) for s in seeds]
    local = {v: i for i, v in enumerate(vertices)}
    assert len(local) == len(vertices), "the seeds are distinct"
    vertex_ptr, edge_ptr, offsets, cols, eids = [0, len(vertices)], [0], [0], [], []
    lo, hi = 0, len(vertices)
    for hop, f in enumerate(fanouts):
        new = set()
        for lid in range(lo, hi):
            v = vertices[lid]
            for k in picks_of(v, hop, f):
                c = sci[ro[v] + k]
                cols.append(c)
                eids.append(sent[ro[v] + k])
                if c not in local:
                    new.add(c)
            offsets.append(len(cols))
        for c in sorted(new):
            local[c] = len(vertices)
            vertices.append(c)
        lo, hi = hi, len(vertices)
        vertex_ptr.append(len(vertices))
        edge_ptr.append(len(cols))
    offsets += [len(cols)] * (len(vertices) + 1 - len(offsets))
    return _pack(vertices, vertex_ptr, offsets, [local[c] for c in cols], eids, edge_ptr)


# ---------------- the vectorised form ----------------

def vectorised(n, ro, ci, seeds, fanouts, weights=None, replace=False, weighted=False, seed=0):
    assert not (weighted and not replace) and not (weighted and weights is None)
    ro, sci, sw, sent = sorted_copy(n, ro, ci, weights)
    deg = np.diff(ro)
    running = np.cumsum(sw).astype(np.uint64)
    before = np.concatenate([[0], running])[ro[:-1]].astype(np.uint64)
    total = np.concatenate([[0], running])[ro[1:]].astype(np.uint64) - before
    u32 = np.uint64(32)

    local = np.full(n, -1, dtype=np.int64)
    frontier = np.asarray(seeds, dtype=np.int64).reshape(-1)
    local[frontier] = np.arange(frontier.shape[0])
    parts_v, parts_c, parts_e, row_counts = [frontier], [], [], []
    count_v, count_e = frontier.shape[0], 0
    vertex_ptr, edge_ptr = [0, count_v], [0]
    for hop, f in enumerate(fanouts):
        v, d = frontier, deg[frontier]
        if f == -1:
            counts = d
        elif not replace:
            counts = np.minimum(d, f)
        else:
            counts = np.where((total[v] > 0) if weighted else (d > 0), f, 0)
        width = int(counts.max()) if counts.shape[0] else 0
        k = np.broadcast_to(np.arange(width, dtype=np.int64), (v.shape[0], width)).copy()  # whole rows: the positions in order
        if f != -1 and width:
            slots = np.arange(f, dtype=np.uint64)
            if not replace:
                rows = np.nonzero(d > f)[0]
                if rows.shape[0]:
                    r = ga.rw_draw(seed, v[rows].astype(np.uint64)[:, None], hop, slots[None, :])
                    i = (d[rows] - f)[:, None] + np.arange(f, dtype=np.int64)[None, :]
                    t = (((r >> u32) * (i + 1).astype(np.uint64)) >> u32).astype(np.int64)
                    for s in range(1, f):
                        seen = (t[:, :s] == t[:, s:s + 1]).any(axis=1)  # t[:, :s] holds the resolved picks
                        t[seen, s] = i[seen, s]
                    k[rows] = t
            else:
                rows = np.nonzero(counts > 0)[0]
                if rows.shape[0]:
                    r = ga.rw_draw(seed, v[rows].astype(np.uint64)[:, None], hop, slots[None, :])
                    if not weighted:
                        k[rows] = (((r >> u32) * d[rows].astype(np.uint64)[:, None]) >> u32).astype(np.int64)
                    else:
                        at = before[v[rows]][:, None] + rk.mulhi(r, np.broadcast_to(total[v[rows]][:, None], r.shape).copy())
                        k[rows] = np.searchsorted(running, at, side="right").astype(np.int64) - ro[v[rows]][:, None]
        keep = np.arange(width)[None, :] < counts[:, None]
        pos = (ro[v][:, None] + k)[keep]  # row-major: frontier order, then slot order
        cols_v = sci[pos]
        new = np.unique(cols_v[local[cols_v] < 0])
        local[new] = count_v + np.arange(new.shape[0])
        parts_v.append(new)
        parts_c.append(cols_v)
        parts_e.append(sent[pos])
        row_counts.append(counts)
        count_v += new.shape[0]
        count_e += pos.shape[0]
        vertex_ptr.append(count_v)
        edge_ptr.append(count_e)
        frontier = new
    vertices = np.concatenate(parts_v)
    cols_v = np.concatenate(parts_c) if parts_c else np.zeros(0, dtype=np.int64)
    per_row = np.zeros(count_v, dtype=np.int64)
    expanded = np.concatenate(row_counts) if row_counts else np.zeros(0, dtype=np.int64)
    per_row[:expanded.shape[0]] = expanded
    offsets = np.concatenate([[0], np.cumsum(per_row)])
    return _pack(vertices, vertex_ptr, offsets, local[cols_v], np.concatenate(parts_e) if parts_e else [], edge_ptr)


def same(a, b, keys=KEYS):
    return all(a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]) for key in keys)
