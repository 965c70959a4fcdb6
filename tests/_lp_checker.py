"""CPU checker for label propagation (grx_lp_*).

The CSR is an undirected simple graph exactly as _matching_checker.pairs_of reads it: canonical pairs {a < b} sorted by (a, b), the
weight of a pair the largest of its entries (None: 1 each), every weight at least 1.  L[v] is a label in [0, n); reset: L[v] = v or the
caller's start.  The vote of a vertex with a neighbour: score(l) = sum of w(v, u) over the neighbours with L[u] = l (an exact integer),
best = the largest score; the new label is L[v] if score(L[v]) == best, else the smallest l with score(l) == best.  Isolated vertices
keep their label.

  SYNC     L_{t+1} from L_t for all vertices at once
  CLASSES  classes[] is a proper colouring; a round is the sequential sweep in (class, id) order, in place

A vertex is visited at its turn iff it has never been visited since reset or a neighbour's label changed since its last visit;
visits counts the visits and entries_read sums d(v) over them.  After round r: nothing changed -> CONVERGED (the round is not
counted in rounds); SYNC, r >= 2 and L_r == L_{r-2} -> PERIOD2; r == max_rounds -> CAPPED.

Two independent forms that must agree (solve):
  run_python  a dict vote per vertex, plain Python lists, the sweep written out
  run_numpy   per step one np.lexsort over (row, label) of the visited rows' entries and np.add.reduceat over the groups
Both return {"labels", "state", "rounds", "visits", "entries_read"}; with keep=True also "history", the labels behind every round."""
import numpy as np

from _matching_checker import csr_from_pairs, mod7_weights, pairs_of, path  # noqa: F401  (the graphs the LP tests share)

SYNC, CLASSES = 0, 1
CONVERGED, PERIOD2, CAPPED = 0, 1, 2
INT_MAX = 2 ** 31 - 1


def rows_of(n, a, b, w):
    """(ro, ci, ew) as int64: the neighbour CSR of the pairs, rows ascending by neighbour"""
    a, b, w = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(w, np.int64)
    rows, cols, vals = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])
    order = np.lexsort((cols, rows))
    ro = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ro[1:])
    return ro, cols[order], vals[order]


def _ended(result, labels, state, rounds, visits, entries, history, keep):
    out = {"labels": np.asarray(labels, np.int32), "state": state, "rounds": rounds, "visits": visits, "entries_read": entries}
    if keep:
        out["history"] = history
    return out


def run_python(n, a, b, w, mode, classes=None, start=None, max_rounds=10 ** 9, keep=False):
    adj = [[] for _ in range(n)]
    for x, y, z in zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(w).tolist()):
        adj[x].append((y, z))
        adj[y].append((x, z))
    L = list(range(n)) if start is None else [int(x) for x in start]
    dirty = [True] * n
    order = list(range(n)) if mode == SYNC else sorted(range(n), key=lambda v: (int(classes[v]), v))
    visits = entries = rounds = 0
    history, before, before2 = [], None, None

    def vote(v, labels):
        score = {}
        for u, z in adj[v]:
            score[labels[u]] = score.get(labels[u], 0) + z
        best = max(score.values())
        if score.get(labels[v], 0) == best:
            return labels[v]
        return min(l for l, s in score.items() if s == best)

    r = 0
    while True:
        r += 1
        changed = []
        if mode == SYNC:
            before2, before = before, L
            new = list(L)
            turn = [v for v in order if dirty[v]]
            for v in turn:
                dirty[v] = False
                visits += 1
                entries += len(adj[v])
                if adj[v]:
                    new[v] = vote(v, L)
                    if new[v] != L[v]:
                        changed.append(v)
            L = new
            for v in changed:
                for u, _ in adj[v]:
                    dirty[u] = True
        else:
            for v in order:
                if not dirty[v]:
                    continue
                dirty[v] = False
                visits += 1
                entries += len(adj[v])
                if adj[v]:
                    nl = vote(v, L)
                    if nl != L[v]:
                        L[v] = nl
                        changed.append(v)
                        for u, _ in adj[v]:
                            dirty[u] = True
        if keep:
            history.append(np.asarray(L, np.int32))
        if not changed:
            return _ended(None, L, CONVERGED, rounds, visits, entries, history, keep)
        rounds += 1
        if mode == SYNC and r >= 2 and L == before2:
            return _ended(None, L, PERIOD2, rounds, visits, entries, history, keep)
        if r >= max_rounds:
            return _ended(None, L, CAPPED, rounds, visits, entries, history, keep)


def _votes(ro, ci, ew, L, turn):
    """the new labels of the vertices `turn` (all with a neighbour) from the labels L: lexsort over (row, label), reduceat"""
    deg = ro[turn + 1] - ro[turn]
    row = np.repeat(np.arange(turn.shape[0]), deg)
    at = np.repeat(ro[turn] - (np.cumsum(deg) - deg), deg) + np.arange(int(deg.sum()))
    lab, wt = L[ci[at]], ew[at]
    order = np.lexsort((lab, row))
    row, lab, wt = row[order], lab[order], wt[order]
    head = np.ones(row.shape[0], bool)
    head[1:] = (row[1:] != row[:-1]) | (lab[1:] != lab[:-1])
    starts = np.flatnonzero(head)
    score = np.add.reduceat(wt, starts)            # per (row, label) group
    grow, glab = row[starts], lab[starts]
    first = np.ones(grow.shape[0], bool)
    first[1:] = grow[1:] != grow[:-1]
    rstarts = np.flatnonzero(first)                # per row (every row of `turn` has a group)
    best = np.maximum.reduceat(score, rstarts)
    top = score == best[grow]
    cur = L[turn]
    keeps = np.zeros(turn.shape[0], bool)
    keeps[grow[top & (glab == cur[grow])]] = True
    smallest = np.minimum.reduceat(np.where(top, glab, np.int64(2) ** 62), rstarts)
    return np.where(keeps, cur, smallest)


def run_numpy(n, a, b, w, mode, classes=None, start=None, max_rounds=10 ** 9, keep=False):
    ro, ci, ew = rows_of(n, a, b, w)
    deg = np.diff(ro)
    L = np.arange(n, dtype=np.int64) if start is None else np.asarray(start, np.int64).copy()
    dirty = np.ones(n, bool)
    if mode == CLASSES:
        classes = np.asarray(classes, np.int64)
        members = [np.flatnonzero(classes == k) for k in range(int(classes.max()) + 1 if n else 0)]
    visits = entries = rounds = 0
    history, before, before2 = [], None, None

    def mark(changed):
        d = deg[changed]
        dirty[ci[np.repeat(ro[changed] - (np.cumsum(d) - d), d) + np.arange(int(d.sum()))]] = True

    r = 0
    while True:
        r += 1
        total_changed = 0
        steps = [None] if mode == SYNC else members
        if mode == SYNC:
            before2, before = before, L.copy()
        for group in steps:
            turn = np.flatnonzero(dirty) if group is None else group[dirty[group]]
            dirty[turn] = False
            visits += int(turn.shape[0])
            entries += int(deg[turn].sum())
            turn = turn[deg[turn] > 0]
            if turn.shape[0] == 0:
                continue
            new = _votes(ro, ci, ew, L, turn)
            changed = turn[new != L[turn]]
            L[turn] = new
            total_changed += int(changed.shape[0])
            if changed.shape[0]:
                mark(changed)
        if keep:
            history.append(L.astype(np.int32))
        if total_changed == 0:
            return _ended(None, L, CONVERGED, rounds, visits, entries, history, keep)
        rounds += 1
        if mode == SYNC and r >= 2 and np.array_equal(L, before2):
            return _ended(None, L, PERIOD2, rounds, visits, entries, history, keep)
        if r >= max_rounds:
            return _ended(None, L, CAPPED, rounds, visits, entries, history, keep)


FIELDS = ("state", "rounds", "visits", "entries_read")


def solve(n, a, b, w, mode, classes=None, start=None, max_rounds=10 ** 9, keep=False):
    """both forms agree, or AssertionError; returns the result"""
    x = run_python(n, a, b, w, mode, classes, start, max_rounds, keep)
    y = run_numpy(n, a, b, w, mode, classes, start, max_rounds, keep)
    assert np.array_equal(x["labels"], y["labels"]), "the two forms differ in labels"
    for name in FIELDS:
        assert x[name] == y[name], "the two forms differ in %s: %s against %s" % (name, x[name], y[name])
    return x


def community_of(labels):
    """(community int32 per vertex: the rank of its label among the labels in use, the count)"""
    used, inverse = np.unique(np.asarray(labels), return_inverse=True)
    return inverse.reshape(-1).astype(np.int32), int(used.shape[0])


def summary_of(n, a, b, w, labels):
    """{"size", "internal", "volume"} int64 per community and "W" """
    community, k = community_of(labels)
    a, b, w = np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(w, np.int64)
    size = np.bincount(community, minlength=k).astype(np.int64)
    inside = community[a] == community[b]
    internal = np.zeros(k, np.int64)
    np.add.at(internal, community[a[inside]], w[inside])
    wdeg = np.zeros(n, np.int64)
    np.add.at(wdeg, a, w)
    np.add.at(wdeg, b, w)
    volume = np.zeros(k, np.int64)
    np.add.at(volume, community, wdeg)
    return {"size": size, "internal": internal, "volume": volume, "W": int(w.sum())}


def modularity(summary):
    """float64: sum(internal / W - (volume / (2 W))^2)"""
    W = float(summary["W"])
    if W == 0:
        return 0.0
    return float(np.sum(summary["internal"].astype(np.float64) / W - (summary["volume"].astype(np.float64) / (2.0 * W)) ** 2))


def networkx_modularity(n, a, b, w, labels):
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_weighted_edges_from(zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(w).tolist()))
    groups = {}
    for v, l in enumerate(np.asarray(labels).tolist()):
        groups.setdefault(l, set()).add(v)
    return nx.community.modularity(g, list(groups.values()), weight="weight")


def is_proper(a, b, classes):
    classes = np.asarray(classes)
    return bool((classes[np.asarray(a)] != classes[np.asarray(b)]).all())


def greedy_classes(n, a, b):
    """the id-order greedy colouring: every vertex takes the smallest class none of its smaller neighbours has"""
    adj = [[] for _ in range(n)]
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        adj[y].append(x)  # (x < y)
    classes = [0] * n
    for v in range(n):
        taken = {classes[u] for u in adj[v]}
        k = 0
        while k in taken:
            k += 1
        classes[v] = k
    return np.asarray(classes, np.int32)


# ---------------- graphs ----------------

def complete_bipartite(p, q):
    rows = np.repeat(np.arange(p), q)
    cols = p + np.tile(np.arange(q), p)
    return csr_from_pairs(p + q, rows, cols)[:2]


def star(leaves):
    return csr_from_pairs(leaves + 1, np.zeros(leaves, np.int64), np.arange(1, leaves + 1))[:2]


def clique_ring(c, s):
    """c cliques of s vertices; the last vertex of every clique is joined to the first of the next"""
    rows, cols = [], []
    for k in range(c):
        base = k * s
        for i in range(s):
            for j in range(i + 1, s):
                rows.append(base + i)
                cols.append(base + j)
        rows.append(base + s - 1)
        cols.append(((k + 1) % c) * s)
    return csr_from_pairs(c * s, rows, cols)[:2]
