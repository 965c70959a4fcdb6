"""CPU checker for the heavy-edge matching and its contraction (grx_matching_*).

The CSR is an undirected simple graph: either row may hold the edge, self-loops are ignored, duplicates are allowed.  The M canonical
pairs {a < b} are sorted by (a, b); the weight w(i) of pair i is the largest of its entries (None: 1 each); pairs are strictly ordered
by key(i) = ((uint32)w(i) ^ 0x80000000) << 32 | fmix32((uint32)i + seed * 0x9E3779B9), and in_matching[i] = 1 iff no pair j that
shares an end with i and has key(j) > key(i) has in_matching[j] = 1.  Three forms that must agree:
  greedy   the sequential pass over the pairs in descending key order, in plain Python
  rounds   mutual-best rounds in numpy: every vertex with a live pair (both ends unmatched) names its largest-keyed one, a pair named
           by both ends is matched; it also returns its round count
  verify   vectorised, for large graphs: the equation per pair, mate / medge consistency and maximality
networkx validates (is_matching, is_maximal_matching, and on small graphs the half-approximation of max_weight_matching).  The
contraction comes as the numpy restatement of the definition and as P.T @ A @ P in scipy.sparse with the diagonal dropped."""
import numpy as np

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1


class Overflow(ArithmeticError):
    """a coarse pair weight or vertex weight outside int32 (contract's -5)"""


def fmix32(h):
    h = np.asarray(h, np.uint64) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(16))


def pairs_of(nodes, row_offsets, col_indices, weights=None):
    """(a, b, w) as int32: the canonical pairs and their weights"""
    ro = np.asarray(row_offsets, np.int64)
    v = np.asarray(col_indices, np.int64)
    u = np.repeat(np.arange(nodes, dtype=np.int64), np.diff(ro)) if nodes else np.zeros(0, np.int64)
    w = np.ones(v.shape[0], np.int64) if weights is None else np.asarray(weights, np.int64)
    keep = u != v
    u, v, w = u[keep], v[keep], w[keep]
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    keys, inverse = np.unique(lo * max(nodes, 1) + hi, return_inverse=True)
    pw = np.full(keys.shape[0], INT_MIN, np.int64)
    np.maximum.at(pw, inverse.reshape(-1), w)
    return (keys // max(nodes, 1)).astype(np.int32), (keys % max(nodes, 1)).astype(np.int32), pw.astype(np.int32)


def keys_of(w, seed=0):
    """key(i) as uint64 for the pair weights w (int32, in canonical order)"""
    w = np.asarray(w, np.int64)
    hi = ((w & 0xFFFFFFFF) ^ 0x80000000).astype(np.uint64)
    i = np.arange(w.shape[0], dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)
    return (hi << np.uint64(32)) | fmix32(i)


def _result(nodes, a, b, w, chosen):
    in_matching = np.zeros(a.shape[0], np.uint8)
    in_matching[chosen] = 1
    mate = np.full(nodes, -1, np.int32)
    medge = np.full(nodes, -1, np.int32)
    sel = np.flatnonzero(in_matching)
    mate[a[sel]], mate[b[sel]] = b[sel], a[sel]
    medge[a[sel]] = medge[b[sel]] = sel
    deg = np.bincount(np.concatenate([a, b]), minlength=nodes)
    matched = int(sel.shape[0])
    summary = {"pairs": int(a.shape[0]), "matched": matched, "weight": int(w[sel].astype(np.int64).sum()), "unmatched": nodes - 2 * matched,
               "unmatched_with_neighbours": int((deg > 0).sum()) - 2 * matched}
    return {"in_matching": in_matching, "mate": mate, "medge": medge, "summary": summary}


def greedy(nodes, a, b, w, seed=0):
    """the sequential pass in descending key order, plain Python"""
    key = keys_of(w, seed)
    order = np.argsort(key)[::-1].tolist()
    al, bl = a.tolist(), b.tolist()
    used = [False] * nodes
    chosen = []
    for i in order:
        if not used[al[i]] and not used[bl[i]]:
            used[al[i]] = used[bl[i]] = True
            chosen.append(i)
    return _result(nodes, a, b, w, np.array(chosen, np.int64))


def rounds(nodes, a, b, w, seed=0):
    """(result, rounds): mutual-best rounds until no pair has two unmatched ends"""
    key = keys_of(w, seed)
    order = np.argsort(key)  # ascending: the last write of a scatter in this order is the largest key
    free = np.ones(nodes, bool)
    chosen = []
    count = 0
    live, al, bl = order, a[order].astype(np.int64), b[order].astype(np.int64)
    best = np.full(nodes, -1, np.int64)  # (only the entries a round has just written are read)
    while True:
        keep = free[al] & free[bl]
        live, al, bl = live[keep], al[keep], bl[keep]
        if live.shape[0] == 0:
            break
        count += 1
        ends = np.empty(2 * live.shape[0], np.int64)
        ends[0::2], ends[1::2] = al, bl
        best[ends] = np.repeat(live, 2)  # (ascending key order, and a repeated index keeps its last value: the largest wins)
        mutual = (best[al] == live) & (best[bl] == live)
        chosen.append(live[mutual])
        free[al[mutual]] = free[bl[mutual]] = False
    chosen = np.concatenate(chosen) if chosen else np.zeros(0, np.int64)
    return _result(nodes, a, b, w, chosen), count


def verify(nodes, a, b, w, seed, in_matching, mate, medge):
    """a list of what is wrong (empty: all right): the equation per pair, mate / medge, maximality"""
    bad = []
    key = keys_of(w, seed)
    M = a.shape[0]
    in_matching = np.asarray(in_matching)
    if in_matching.shape[0] != M or not np.isin(in_matching, (0, 1)).all():
        return ["in_matching is no 0/1 array of M entries"]
    sel = np.flatnonzero(in_matching)
    ends = np.concatenate([a[sel], b[sel]])
    if np.unique(ends).shape[0] != ends.shape[0]:
        return ["two matched pairs share an end"]
    # the key of the matched pair at every vertex (0 and no pair: nothing dominates there)
    at = np.zeros(nodes, np.uint64)
    has = np.zeros(nodes, bool)
    at[a[sel]] = at[b[sel]] = key[sel]
    has[ends] = True
    dominated = (has[a] & (at[a] > key)) | (has[b] & (at[b] > key))
    if not np.array_equal(in_matching.astype(bool), ~dominated):
        bad.append("the equation fails at %d pairs" % int((in_matching.astype(bool) != ~dominated).sum()))
    want_mate = np.full(nodes, -1, np.int32)
    want_medge = np.full(nodes, -1, np.int32)
    want_mate[a[sel]], want_mate[b[sel]] = b[sel], a[sel]
    want_medge[a[sel]] = want_medge[b[sel]] = sel
    if not np.array_equal(mate, want_mate):
        bad.append("mate")
    if not np.array_equal(medge, want_medge):
        bad.append("medge")
    if (~has[a] & ~has[b]).any():
        bad.append("not maximal")
    return bad


def solve(nodes, row_offsets, col_indices, weights=None, seed=0):
    """(a, b, w, result, rounds): greedy and the rounds form agree and pass verify, or AssertionError"""
    a, b, w = pairs_of(nodes, row_offsets, col_indices, weights)
    ref = greedy(nodes, a, b, w, seed)
    by_rounds, count = rounds(nodes, a, b, w, seed)
    for name in ("in_matching", "mate", "medge"):
        assert np.array_equal(ref[name], by_rounds[name]), "greedy and rounds differ in " + name
    assert ref["summary"] == by_rounds["summary"]
    assert not verify(nodes, a, b, w, seed, ref["in_matching"], ref["mate"], ref["medge"])
    return a, b, w, ref, count


def networkx_validate(nodes, a, b, w, ref):
    """is_matching, is_maximal_matching, and on graphs of <= 40 vertices with weights >= 0 the half-approximation"""
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(nodes))
    g.add_weighted_edges_from(zip(a.tolist(), b.tolist(), w.tolist()))
    sel = np.flatnonzero(ref["in_matching"])
    matching = set(zip(a[sel].tolist(), b[sel].tolist()))
    assert nx.is_matching(g, matching) and nx.is_maximal_matching(g, matching)
    if nodes <= 40 and (w >= 0).all():
        best = nx.max_weight_matching(g)
        assert 2 * ref["summary"]["weight"] >= sum(g[x][y]["weight"] for x, y in best)


def mismatches(p, nodes, a, b, w, ref):
    """what of a finished MatchingProblem differs from the checker's result"""
    bad = []
    src, dst, pw = p.pairs()
    if not (np.array_equal(src, a) and np.array_equal(dst, b) and np.array_equal(pw, w)):
        bad.append("pairs")
    got = p.extract()
    for name in ("in_matching", "mate", "medge"):
        if got[name].dtype != ref[name].dtype or not np.array_equal(got[name], ref[name]):
            bad.append(name)
    if p.summary() != ref["summary"]:
        bad.append("summary %s" % p.summary())
    return bad


# ---------------- the contraction ----------------

def contract(nodes, a, b, w, mate, vertex_weights=None):
    """(map, coarse_nodes, ro, ci, weights, vweight) as int32 by the definition; Overflow when a sum leaves int32"""
    v = np.arange(nodes, dtype=np.int64)
    rep = np.where(mate >= 0, np.minimum(v, mate), v)
    reps, cmap = np.unique(rep, return_inverse=True)
    cmap = cmap.reshape(-1)
    nc = int(reps.shape[0])
    vw = np.ones(nodes, np.int64) if vertex_weights is None else np.asarray(vertex_weights, np.int64)
    vweight = np.zeros(nc, np.int64)
    np.add.at(vweight, cmap, vw)
    ca, cb = cmap[a], cmap[b]
    keep = ca != cb
    lo, hi, pw = np.minimum(ca, cb)[keep], np.maximum(ca, cb)[keep], np.asarray(w, np.int64)[keep]
    keys, inverse = np.unique(lo * nc + hi, return_inverse=True)
    cw = np.zeros(keys.shape[0], np.int64)
    np.add.at(cw, inverse.reshape(-1), pw)
    if (vweight.size and (vweight.min() < INT_MIN or vweight.max() > INT_MAX)) or (cw.size and (cw.min() < INT_MIN or cw.max() > INT_MAX)):
        raise Overflow()
    x, y = keys // nc, keys % nc
    rows, cols, vals = np.concatenate([x, y]), np.concatenate([y, x]), np.concatenate([cw, cw])
    order = np.lexsort((cols, rows))
    ro = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=nc), out=ro[1:])
    return cmap.astype(np.int32), nc, ro.astype(np.int32), cols[order].astype(np.int32), vals[order].astype(np.int32), vweight.astype(np.int32)


def contract_sparse(nodes, a, b, w, mate, vertex_weights=None):
    """the same as P.T @ A @ P with the diagonal dropped: A the symmetric pair-weight matrix, P the indicator of map"""
    import scipy.sparse as sp
    v = np.arange(nodes, dtype=np.int64)
    rep = np.where(mate >= 0, np.minimum(v, mate), v)
    is_rep = rep == v
    cmap = (np.cumsum(is_rep) - 1)[rep]
    nc = int(is_rep.sum())
    P = sp.csr_matrix((np.ones(nodes, np.int64), (v, cmap)), shape=(nodes, nc))
    # (an explicit entry per pair: a pair of weight 0 is still a pair, so the structure is carried next to the values)
    wl = np.asarray(w, np.int64)
    A = sp.coo_matrix((np.concatenate([wl, wl]), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(nodes, nodes)).tocsr()
    S = sp.coo_matrix((np.ones(2 * a.shape[0], np.int64), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(nodes, nodes)).tocsr()
    C, T = (P.T @ A @ P).tocoo(), (P.T @ S @ P).tocoo()
    off = T.row != T.col
    rows, cols = T.row[off].astype(np.int64), T.col[off].astype(np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    # the values of C at the positions of T (a sum that is 0 may be missing from C)
    ckey = C.row.astype(np.int64) * nc + C.col.astype(np.int64)
    corder = np.argsort(ckey)
    ckey, cdata = ckey[corder], C.data[corder].astype(np.int64)
    at = np.minimum(np.searchsorted(ckey, rows * nc + cols), max(ckey.shape[0] - 1, 0))
    vals = np.where(ckey[at] == rows * nc + cols, cdata[at], 0) if ckey.shape[0] else np.zeros(rows.shape[0], np.int64)
    vw = np.ones(nodes, np.int64) if vertex_weights is None else np.asarray(vertex_weights, np.int64)
    vweight = np.asarray(P.T @ vw).reshape(-1)
    if (vweight.size and (vweight.min() < INT_MIN or vweight.max() > INT_MAX)) or (vals.size and (vals.min() < INT_MIN or vals.max() > INT_MAX)):
        raise Overflow()
    ro = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=nc), out=ro[1:])
    return cmap.astype(np.int32), nc, ro.astype(np.int32), cols.astype(np.int32), vals.astype(np.int32), vweight.astype(np.int32)


def same_coarse(x, y):
    return x[1] == y[1] and all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(x[:1] + x[2:], y[:1] + y[2:]))


# ---------------- graphs ----------------

def csr_from_pairs(nodes, rows, cols, weights=None, mirror=True, shuffle=None):
    """(ro, ci, w or None) as int32 from a list of entries; mirror adds the other direction; shuffle (a Generator) mixes each row"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    w = None if weights is None else np.asarray(weights, np.int64)
    if mirror:
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
        w = None if w is None else np.concatenate([w, w])
    tie = shuffle.random(rows.shape[0]) if shuffle is not None else cols
    order = np.lexsort((tie, rows))
    ro = np.zeros(nodes + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=nodes), out=ro[1:])
    return ro.astype(np.int32), cols[order].astype(np.int32), None if w is None else w[order].astype(np.int32)


def mod7_weights(nodes, row_offsets, col_indices):
    """(row + col) % 7 + 1 per entry"""
    ro = np.asarray(row_offsets, np.int64)
    rows = np.repeat(np.arange(nodes, dtype=np.int64), np.diff(ro))
    return ((rows + np.asarray(col_indices, np.int64)) % 7 + 1).astype(np.int32)


def path(n, weights=None):
    """the path 0 - 1 - ... - (n - 1), mirrored; weights per pair (a, a + 1)"""
    return csr_from_pairs(n, np.arange(n - 1), np.arange(1, n), weights)
