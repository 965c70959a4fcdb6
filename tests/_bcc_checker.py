"""CPU checker for the biconnected components, articulation points, bridges and 2-edge-connected components (grx_bcc_*).

Three independent forms that must agree, all on the simple undirected graph of a CSR (entries symmetrised, duplicates and loops
dropped), with the M canonical edges (a, b), a < b, sorted by (a, b):
  tarjan_vishkin   the rules the GPU kernels follow, in plain Python over a spanning forest (breadth-first, or a non-BFS one)
  hopcroft_tarjan  the sequential depth-first search with an edge stack
  by_networkx      biconnected_component_edges / articulation_points / bridges, connected_components of G minus its bridges
Every form returns a dict of canonical arrays: "bcc" (int32 per edge: the smallest edge index of its block), "bridge" (uint8 per
edge), "articulation" (uint8 per vertex), "tecc" (int32 per vertex: the smallest id of its 2-edge-connected component)."""
import numpy as np


def simple_edges(nodes, row_offsets, col_indices):
    """(a, b): the canonical edges of the CSR read as an undirected simple graph, int32"""
    ro = np.asarray(row_offsets, np.int64)
    ci = np.asarray(col_indices, np.int64)
    rows = np.repeat(np.arange(nodes, dtype=np.int64), np.diff(ro)) if nodes else np.zeros(0, np.int64)
    keep = rows != ci
    lo, hi = np.minimum(rows, ci)[keep], np.maximum(rows, ci)[keep]
    keys = np.unique(lo * max(nodes, 1) + hi)
    return (keys // max(nodes, 1)).astype(np.int32), (keys % max(nodes, 1)).astype(np.int32)


def neighbour_csr(nodes, a, b):
    """rows ascending by neighbour id, with the edge index of every entry (the layout the device builds)"""
    M = a.shape[0]
    src = np.concatenate([a, b]).astype(np.int64)
    dst = np.concatenate([b, a]).astype(np.int64)
    eid = np.concatenate([np.arange(M), np.arange(M)])
    order = np.lexsort((dst, src))
    start = np.zeros(nodes + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=nodes), out=start[1:])
    return start, dst[order], eid[order]


def canonical(label):
    """label[i] -> the smallest index that carries the same label (int32)"""
    label = np.asarray(label, np.int64)
    if label.shape[0] == 0:
        return np.zeros(0, np.int32)
    _, inverse = np.unique(label, return_inverse=True)
    first = np.full(int(inverse.max()) + 1, label.shape[0], np.int64)
    np.minimum.at(first, inverse, np.arange(label.shape[0]))
    return first[inverse].astype(np.int32)


def _result(nodes, a, b, block, art):
    """the canonical arrays from a block label per edge and the articulation mask; bridges and tecc follow from the blocks"""
    bcc = canonical(block)
    size = block_sizes(bcc)
    bridge = (size == 1).astype(np.uint8)
    return {"bcc": bcc, "bridge": bridge, "articulation": np.asarray(art, np.uint8), "tecc": tecc_of(nodes, a, b, bridge)}


def tecc_of(nodes, a, b, bridge):
    """the components of G minus its bridges, smallest id each (a union-find with path halving)"""
    up = list(range(nodes))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x
    for u, v, cut in zip(a.tolist(), b.tolist(), bridge.tolist()):
        if not cut:
            ru, rv = find(u), find(v)
            if ru != rv:
                up[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(nodes)], np.int32).reshape(nodes)


def block_sizes(bcc):
    """block_size[e]: the edges in the block of e, int32"""
    bcc = np.asarray(bcc, np.int64)
    return np.bincount(bcc, minlength=bcc.shape[0])[bcc].astype(np.int32) if bcc.shape[0] else np.zeros(0, np.int32)


# ---------------- form 1: the Tarjan-Vishkin rules ----------------

def tarjan_vishkin(nodes, a, b, bfs=True):
    M = a.shape[0]
    start, nbr, eid = neighbour_csr(nodes, a, b)
    start, nbr, eid = start.tolist(), nbr.tolist(), eid.tolist()
    parent = [-2] * nodes
    order = []
    for r in range(nodes):  # the smallest id of a component is its root
        if parent[r] != -2:
            continue
        parent[r] = -1
        if start[r] == start[r + 1]:
            continue
        todo = [r]
        at = 0
        while at < len(todo) if bfs else todo:
            if bfs:
                v = todo[at]
                at += 1
            else:
                v = todo.pop()
            order.append(v)
            for i in range(start[v], start[v + 1]):
                w = nbr[i]
                if parent[w] == -2:
                    parent[w] = v
                    todo.append(w)
    size = [1] * nodes
    for v in reversed(order):
        if parent[v] >= 0:
            size[parent[v]] += size[v]
    pre = [0] * nodes
    cursor = 0
    for v in order:  # a parent comes before its children
        if parent[v] < 0:
            pre[v] = cursor
            cursor += size[v]
        nxt = pre[v] + 1
        for i in range(start[v], start[v + 1]):
            w = nbr[i]
            if parent[w] == v:
                pre[w] = nxt
                nxt += size[w]
    low, high = pre[:], pre[:]
    for v in reversed(order):
        for i in range(start[v], start[v + 1]):
            w = nbr[i]
            if w == parent[v]:
                continue
            lo, hi = (low[w], high[w]) if parent[w] == v else (pre[w], pre[w])
            low[v] = min(low[v], lo)
            high[v] = max(high[v], hi)
    up = list(range(nodes))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    def join(x, y):
        x, y = find(x), find(y)
        if x != y:
            up[max(x, y)] = min(x, y)

    def under(x, y):  # y in the subtree of x
        return pre[x] <= pre[y] < pre[x] + size[x]
    al, bl = a.tolist(), b.tolist()
    for u, w in zip(al, bl):
        if parent[w] == u or parent[u] == w:
            v, c = (u, w) if parent[w] == u else (w, u)
            if parent[v] >= 0 and (low[c] < pre[v] or high[c] >= pre[v] + size[v]):
                join(v, c)
        elif not under(u, w) and not under(w, u):
            join(u, w)
    block = np.zeros(M, np.int64)
    for e, (u, w) in enumerate(zip(al, bl)):
        if parent[w] == u:
            end = w
        elif parent[u] == w:
            end = u
        else:
            end = u if pre[u] > pre[w] else w
        block[e] = find(end)
    art = np.zeros(nodes, np.uint8)
    seen = {}
    for w in order:
        v = parent[w]
        if v < 0:
            continue
        if parent[v] >= 0:
            if find(w) != find(v):
                art[v] = 1
        elif seen.setdefault(v, find(w)) != find(w):
            art[v] = 1
    res = _result(nodes, a, b, block, art)
    # rule 6 and rule 10 on their own: the local bridge test, and the forest with its bridges cut
    bridge = np.zeros(M, np.uint8)
    edge_of = {(u, w): e for e, (u, w) in enumerate(zip(al, bl))}
    cut = list(range(nodes))
    for v in order:
        p = parent[v]
        if p < 0:
            continue
        if low[v] >= pre[v] and high[v] < pre[v] + size[v]:
            bridge[edge_of[(min(p, v), max(p, v))]] = 1
        else:
            cut[v] = cut[p]  # (order: the parent's root is final)
    assert np.array_equal(bridge, res["bridge"]), "the local bridge rule and the blocks of one edge differ"
    assert np.array_equal(canonical(np.array(cut, np.int64)), res["tecc"]), "the cut forest and G minus its bridges differ"
    return res


# ---------------- form 2: depth-first search with an edge stack ----------------

def hopcroft_tarjan(nodes, a, b):
    M = a.shape[0]
    start, nbr, eid = neighbour_csr(nodes, a, b)
    start, nbr, eid = start.tolist(), nbr.tolist(), eid.tolist()
    disc = [-1] * nodes
    low = [0] * nodes
    block = [-1] * M
    art = [0] * nodes
    clock = 0
    blocks = 0
    for root in range(nodes):
        if disc[root] >= 0 or start[root] == start[root + 1]:
            continue
        disc[root] = low[root] = clock
        clock += 1
        kids = 0
        st, pe, it, edges = [root], [-1], [start[root]], []
        while st:
            v = st[-1]
            i = it[-1]
            if i < start[v + 1]:
                it[-1] = i + 1
                w, e = nbr[i], eid[i]
                if e == pe[-1]:
                    continue
                if disc[w] < 0:
                    edges.append(e)
                    disc[w] = low[w] = clock
                    clock += 1
                    st.append(w)
                    pe.append(e)
                    it.append(start[w])
                elif disc[w] < disc[v]:
                    edges.append(e)
                    if disc[w] < low[v]:
                        low[v] = disc[w]
            else:
                st.pop()
                it.pop()
                e = pe.pop()
                if not st:
                    break
                u = st[-1]
                if low[v] < low[u]:
                    low[u] = low[v]
                if low[v] >= disc[u]:
                    if u == root:
                        kids += 1
                    else:
                        art[u] = 1
                    while True:
                        x = edges.pop()
                        block[x] = blocks
                        if x == e:
                            break
                    blocks += 1
        if kids > 1:
            art[root] = 1
    return _result(nodes, a, b, np.array(block, np.int64).reshape(M), art)


# ---------------- form 3: networkx ----------------

def by_networkx(nodes, a, b):
    import networkx as nx
    M = a.shape[0]
    g = nx.Graph()
    g.add_nodes_from(range(nodes))
    g.add_edges_from(zip(a.tolist(), b.tolist()))
    index = {(u, w): e for e, (u, w) in enumerate(zip(a.tolist(), b.tolist()))}
    block = np.full(M, -1, np.int64)
    for k, edges in enumerate(nx.biconnected_component_edges(g)):
        for u, w in edges:
            block[index[(min(u, w), max(u, w))]] = k
    assert (block >= 0).all()
    art = np.zeros(nodes, np.uint8)
    art[list(nx.articulation_points(g))] = 1
    bridge = np.zeros(M, np.uint8)
    for u, w in nx.bridges(g):
        bridge[index[(min(u, w), max(u, w))]] = 1
    g.remove_edges_from(list(nx.bridges(g)))
    tecc = np.zeros(nodes, np.int32)
    for part in nx.connected_components(g):
        tecc[list(part)] = min(part)
    bcc = canonical(block)
    assert np.array_equal(bridge, (block_sizes(bcc) == 1).astype(np.uint8)), "networkx: bridges are not the blocks of one edge"
    return {"bcc": bcc, "bridge": bridge, "articulation": art, "tecc": tecc}


def solve(nodes, row_offsets, col_indices):
    """(a, b, result) by the depth-first form: the reference of the GPU tests"""
    a, b = simple_edges(nodes, row_offsets, col_indices)
    return a, b, hopcroft_tarjan(nodes, a, b)


def same(x, y):
    return all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in ("bcc", "bridge", "articulation", "tecc"))


# ---------------- what follows from the arrays ----------------

def summary(res):
    bcc, tecc = res["bcc"].astype(np.int64), res["tecc"].astype(np.int64)
    out = {"blocks": int(np.unique(bcc).shape[0]), "bridges": int(res["bridge"].sum()), "articulation_points": int(res["articulation"].sum()),
           "largest_block": 0, "largest_block_id": -1, "tecc_components": int(np.unique(tecc).shape[0]), "largest_tecc": 0, "largest_tecc_root": -1}
    if bcc.shape[0]:
        count = np.bincount(bcc)
        out["largest_block"], out["largest_block_id"] = int(count.max()), int(np.argmax(count))  # (argmax: the first, the smaller id)
    if tecc.shape[0]:
        count = np.bincount(tecc)
        out["largest_tecc"], out["largest_tecc_root"] = int(count.max()), int(np.argmax(count))
    return out


def block_cut(a, b, res):
    """the distinct pairs (articulation point, bcc id), sorted: two int32 arrays"""
    v = np.concatenate([a, b]).astype(np.int64)
    ids = np.concatenate([res["bcc"], res["bcc"]]).astype(np.int64)
    keep = res["articulation"][v] != 0 if v.shape[0] else np.zeros(0, bool)
    span = max(int(res["bcc"].shape[0]), 1)
    keys = np.unique(v[keep] * span + ids[keep])
    return (keys // span).astype(np.int32), (keys % span).astype(np.int32)


def literal(nodes, a, res):
    """the tuple the tests pin: (n, M, blocks, bridges, articulation points, largest block, its id, 2-edge-connected components, the
    largest, sum of bcc, sum of tecc)"""
    s = summary(res)
    return (int(nodes), int(a.shape[0]), s["blocks"], s["bridges"], s["articulation_points"], s["largest_block"], s["largest_block_id"],
            s["tecc_components"], s["largest_tecc"], int(res["bcc"].astype(np.int64).sum()), int(res["tecc"].astype(np.int64).sum()))


# ---------------- generators: (nodes, row_offsets, col_indices), int32 ----------------

def from_edges(nodes, edges, symmetric=True, shuffle=None):
    """a CSR of the given (u, v) pairs; symmetric adds the reverse of each; shuffle: a Generator that permutes every row"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if symmetric:
        e = np.concatenate([e, e[:, ::-1]])
    order = np.lexsort((e[:, 1], e[:, 0])) if shuffle is None else np.lexsort((shuffle.random(e.shape[0]), e[:, 0]))
    e = e[order]
    ro = np.zeros(nodes + 1, np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=nodes), out=ro[1:])
    return nodes, ro.astype(np.int32), e[:, 1].astype(np.int32)


def relabel(graph, perm):
    """vertex v becomes perm[v]"""
    n, ro, ci = graph
    perm = np.asarray(perm, np.int64)
    rows = np.repeat(np.arange(n), np.diff(ro))
    return from_edges(n, np.stack([perm[rows], perm[ci]], axis=1), symmetric=False)


def path(n):
    return from_edges(n, [(i, i + 1) for i in range(n - 1)])


def cycle(n):
    return from_edges(n, [(i, (i + 1) % n) for i in range(n)])


def star(k):
    """hub 0 and k leaves"""
    return from_edges(k + 1, [(0, i) for i in range(1, k + 1)])


def windmill(k):
    """k triangles that share vertex 0"""
    return from_edges(2 * k + 1, [p for i in range(k) for p in ((0, 2 * i + 1), (0, 2 * i + 2), (2 * i + 1, 2 * i + 2))])


def complete(n):
    return from_edges(n, [(i, j) for i in range(n) for j in range(i + 1, n)])


def barbell(m1, m2):
    """two cliques of m1 vertices joined by a path of m2 inner vertices (networkx's barbell_graph)"""
    edges = [(i, j) for i in range(m1) for j in range(i + 1, m1)]
    edges += [(m1 + m2 + i, m1 + m2 + j) for i in range(m1) for j in range(i + 1, m1)]
    edges += [(i, i + 1) for i in range(m1 - 1, m1 + m2)]
    return from_edges(2 * m1 + m2, edges)


def lollipop(m, n):
    """a clique of m vertices with a tail of n"""
    return from_edges(m + n, [(i, j) for i in range(m) for j in range(i + 1, m)] + [(i, i + 1) for i in range(m - 1, m + n - 1)])


def ladder(n):
    return from_edges(2 * n, [(i, i + 1) for i in range(n - 1)] + [(n + i, n + i + 1) for i in range(n - 1)] + [(i, n + i) for i in range(n)])


def grid(rows, cols):
    at = lambda r, c: r * cols + c
    return from_edges(rows * cols, [(at(r, c), at(r, c + 1)) for r in range(rows) for c in range(cols - 1)] +
                      [(at(r, c), at(r + 1, c)) for r in range(rows - 1) for c in range(cols)])


def cross_trap():
    """one block, no articulation point, no bridge; the breadth-first tree from 0 has cross edges (3, 4) and (4, 5), and the local
    low / high test flags vertex 1"""
    return from_edges(6, [(0, 1), (0, 2), (1, 3), (1, 4), (3, 4), (2, 5), (4, 5)])


def planted(seed, vertices=3000, components=3, isolated=5):
    """A random tree of blocks per component -- a cycle, a clique or a single edge each, glued at shared vertices -- under a random
    relabelling, rows shuffled.  Returns (nodes, row_offsets, col_indices, a, b, result): the answer is known by construction."""
    rng = np.random.default_rng(seed)
    edges, block_of = [], []
    member = []   # blocks per vertex
    group = []    # 2-edge-connected group per vertex
    n = 0
    blocks = 0
    for _ in range(components):
        member.append(0)
        group.append(n)
        first = n
        n += 1
        while n - first < vertices // components:
            at = int(rng.integers(first, n))
            kind = int(rng.integers(0, 3))
            k = 2 if kind == 0 else int(rng.choice([3, 4, 5, 8, 63, 64, 65])) if kind == 1 else int(rng.integers(3, 8))
            vs = [at] + list(range(n, n + k - 1))
            if kind == 0:
                pairs = [(vs[0], vs[1])]
            elif kind == 1:
                pairs = [(vs[i], vs[(i + 1) % k]) for i in range(k)]
            else:
                pairs = [(vs[i], vs[j]) for i in range(k) for j in range(i + 1, k)]
            edges += pairs
            block_of += [blocks] * len(pairs)
            blocks += 1
            member[at] += 1
            for v in vs[1:]:
                member.append(1)
                group.append(v if kind == 0 else group[at])
            n += k - 1
    for _ in range(isolated):
        member.append(0)
        group.append(n)
        n += 1
    perm = rng.permutation(n)
    e = perm[np.asarray(edges, np.int64)]
    graph = from_edges(n, e, shuffle=rng)
    a, b = simple_edges(*graph)
    lo, hi = np.minimum(e[:, 0], e[:, 1]), np.maximum(e[:, 0], e[:, 1])
    order = np.lexsort((hi, lo))
    assert np.array_equal(lo[order], a) and np.array_equal(hi[order], b)
    bcc = canonical(np.asarray(block_of, np.int64)[order])
    art = np.zeros(n, np.uint8)
    art[perm[np.flatnonzero(np.asarray(member) > 1)]] = 1
    label = np.zeros(n, np.int64)
    label[perm] = np.asarray(group, np.int64)
    res = {"bcc": bcc, "bridge": (block_sizes(bcc) == 1).astype(np.uint8), "articulation": art, "tecc": canonical(label)}
    return graph + (a, b, res)


def mismatches(p, nodes, a, b, res):
    """what an enacted BccProblem `p` returns against `res`, bit for bit: a list of the names that differ (empty: all equal)"""
    bad = []
    src, dst = p.edges()
    if not (src.dtype == dst.dtype == np.int32 and np.array_equal(src, a) and np.array_equal(dst, b)):
        return ["edges"]
    out = p.extract()
    for key, dtype in (("bcc", np.int32), ("bridge", np.uint8), ("articulation", np.uint8), ("tecc", np.int32)):
        if out[key].dtype != dtype or not np.array_equal(out[key], res[key]):
            bad.append(key)
    if out["block_size"].dtype != np.int32 or not np.array_equal(out["block_size"], block_sizes(res["bcc"])):
        bad.append("block_size")
    if p.summary() != summary(res):
        bad.append("summary %s != %s" % (p.summary(), summary(res)))
    v, ids, count = p.block_cut()
    ref_v, ref_ids = block_cut(a, b, res)
    if not (v.dtype == ids.dtype == np.int32 and count == ref_v.shape[0] and np.array_equal(v, ref_v) and np.array_equal(ids, ref_ids)):
        bad.append("block_cut")
    none_v, none_ids, only_count = p.block_cut(max_edges=0)
    if not (none_v.shape[0] == none_ids.shape[0] == 0 and only_count == count):
        bad.append("block_cut(max_edges=0)")
    return bad
