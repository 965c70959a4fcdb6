"""CPU restatements of colour refinement (1-WL) for the tests of the wl primitive.

The graph is the CSR as given: a row is the multiset of its entries.  A round maps c to c' with c'(u) = c'(v) iff c(u) = c(v) and the
multisets of c over row(u) and row(v) are equal.  Two independent routes to the coarsest equitable partition that refines the labels:
  rounds()    the round as defined, sorted tuples in a dict, until one splits nothing (or for max_rounds rounds)
  splitters() a splitter queue, Paige-Tarjan style: every class is split by its vertices' counts of entries into one splitter class,
              until no splitter splits
Both number the classes 0 .. count - 1 by ascending smallest member (number()); is_equitable() is the predicate both must meet."""
from collections import deque

import numpy as np

STABLE, CAPPED = 0, 1


def csr_of(n, rows, cols, shuffle=None):
    """CSR of the entries (rows[i], cols[i]) as they are: duplicates and loops kept; rows in input order or shuffled by the generator"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if shuffle is not None and rows.shape[0]:
        perm = shuffle.permutation(rows.shape[0])
        rows, cols = rows[perm], cols[perm]
    order = np.argsort(rows, kind="stable")
    ro = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int32)
    return ro, cols[order].astype(np.int32)


def mirrored(n, pairs):
    """the symmetric CSR of the undirected pairs"""
    a = np.array([p[0] for p in pairs] + [p[1] for p in pairs], dtype=np.int64)
    b = np.array([p[1] for p in pairs] + [p[0] for p in pairs], dtype=np.int64)
    return csr_of(n, a, b)


def number(keys):
    """dense ids by ascending smallest member: the classes of equal keys in the order of their first vertex"""
    ids = {}
    return np.array([ids.setdefault(k, len(ids)) for k in keys], dtype=np.int32)


def start(n, labels=None):
    return np.zeros(n, np.int32) if labels is None else number([int(x) for x in labels])


def one_round(n, ro, ci, c):
    return number([(int(c[v]), tuple(sorted(c[ci[ro[v]:ro[v + 1]]].tolist()))) for v in range(n)])


def rounds(n, ro, ci, labels=None, max_rounds=-1):
    """{"colour", "rounds" (those that split a class), "state", "history" (the colouring behind round 0 .. rounds), "trace" (their classes)}"""
    ro, ci = np.asarray(ro), np.asarray(ci)
    c = start(n, labels)
    history = [c]
    state = STABLE
    while max_rounds < 0 or len(history) - 1 < max_rounds:
        fresh = one_round(n, ro, ci, c)
        if int(fresh.max()) == int(c.max()):  # (a round only splits: the same count is the same partition)
            assert np.array_equal(fresh, c)
            break
        c = fresh
        history.append(c)
    else:
        state = CAPPED
    return {"colour": c, "rounds": len(history) - 1, "state": state, "history": history, "trace": [int(h.max()) + 1 for h in history]}


def splitters(n, ro, ci, labels=None):
    """the coarsest equitable partition by a splitter queue: the dense colouring"""
    ro, ci = np.asarray(ro), np.asarray(ci)
    into = [[] for _ in range(n)]  # into[w]: the rows that hold w, once per entry
    for v in range(n):
        for w in ci[ro[v]:ro[v + 1]].tolist():
            into[w].append(v)
    c = start(n, labels)
    cls = {}
    for v in range(n):
        cls.setdefault(int(c[v]), set()).add(v)
    of = {v: int(c[v]) for v in range(n)}
    fresh_id = len(cls)
    queue = deque(sorted(cls))
    queued = set(queue)
    while queue:
        s = queue.popleft()
        queued.discard(s)
        count = {}
        for w in cls[s]:
            for v in into[w]:
                count[v] = count.get(v, 0) + 1
        touched = {}
        for v, k in count.items():
            touched.setdefault(of[v], {}).setdefault(k, set()).add(v)
        for x, parts in touched.items():
            rest = cls[x] - set().union(*parts.values())
            pieces = list(parts.values()) + ([rest] if rest else [])
            if len(pieces) == 1:
                continue
            cls[x] = pieces[0]
            ids = [x]
            for piece in pieces[1:]:
                cls[fresh_id] = piece
                for v in piece:
                    of[v] = fresh_id
                ids.append(fresh_id)
                fresh_id += 1
            for i in ids:  # (every piece: simpler than leaving the largest out, and as right)
                if i not in queued:
                    queue.append(i)
                    queued.add(i)
    return number([of[v] for v in range(n)])


def is_equitable(n, ro, ci, colour):
    """every two vertices of a class have equal multisets of colours in their rows"""
    ro, ci, colour = np.asarray(ro), np.asarray(ci), np.asarray(colour)
    seen = {}
    for v in range(n):
        row = tuple(sorted(colour[ci[ro[v]:ro[v + 1]]].tolist()))
        if seen.setdefault(int(colour[v]), row) != row:
            return False
    return True


def sizes_and_representatives(colour):
    colour = np.asarray(colour)
    k = int(colour.max()) + 1 if colour.shape[0] else 0
    rep = np.full(k, -1, np.int32)
    for v in range(colour.shape[0] - 1, -1, -1):
        rep[colour[v]] = v
    return np.bincount(colour, minlength=k).astype(np.int64), rep


def quotient(n, ro, ci, colour):
    """q[i][j]: the entries of the row of class i's smallest member that lead into class j"""
    ro, ci, colour = np.asarray(ro), np.asarray(ci), np.asarray(colour)
    _, rep = sizes_and_representatives(colour)
    q = np.zeros((rep.shape[0], rep.shape[0]), np.int64)
    for i, r in enumerate(rep.tolist()):
        np.add.at(q[i], colour[ci[ro[r]:ro[r + 1]]], 1)
    return q


# ---------------- the graphs the tests share ----------------

def path(n):
    return mirrored(n, [(i, i + 1) for i in range(n - 1)])


def cycle(n, offset=0):
    return [(offset + i, offset + (i + 1) % n) for i in range(n)]


def petersen():
    return mirrored(10, [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)])


def c6_and_triangles():
    """C6 u 2 K3: 12 vertices, 2-regular"""
    return mirrored(12, cycle(6) + cycle(3, 6) + cycle(3, 9))


def star(leaves):
    return mirrored(leaves + 1, [(0, i + 1) for i in range(leaves)])


def twin_hubs(seed=5, core=640, p=0.05, shared=(600, 40, 10)):
    """A G(core, p) part, rigid with overwhelming probability, and for every s of `shared` two further vertices adjacent to the same
    s vertices of it: each pair shares a class, and its rows hold about s distinct colours.  Returns (n, ro, ci, [(a, b), ...])."""
    rng = np.random.default_rng(seed)
    a, b = np.nonzero(np.triu(rng.random((core, core)) < p, 1))
    pairs = list(zip(a.tolist(), b.tolist()))
    n = core
    twins = []
    for s in shared:
        ends = rng.choice(core, s, replace=False).tolist()
        for t in (n, n + 1):
            pairs += [(t, e) for e in ends]
        twins.append((n, n + 1))
        n += 2
    ro, ci = mirrored(n, pairs)
    return n, ro, ci, twins


def random_graph(rng, max_n=64):
    """up to max_n vertices with loops, duplicates and one-way entries, rows shuffled; random labels or none"""
    n = int(rng.integers(1, max_n + 1))
    m = int(rng.integers(0, 4 * n + 1))
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
    if rng.integers(0, 2):  # mirror a part
        keep = rng.random(m) < 0.7
        rows, cols = np.concatenate([rows, cols[keep]]), np.concatenate([cols, rows[keep]])
    loops = rng.integers(0, n, int(rng.integers(0, n // 4 + 2)))
    dup = rng.integers(0, max(rows.shape[0], 1), int(rng.integers(0, rows.shape[0] // 4 + 2)) if rows.shape[0] else 0)
    rows, cols = np.concatenate([rows, rows[dup], loops]), np.concatenate([cols, cols[dup], loops])
    ro, ci = csr_of(n, rows, cols, shuffle=rng)
    labels = rng.integers(-3, 3, n).astype(np.int32) if rng.integers(0, 2) else None
    return n, ro, ci, labels
