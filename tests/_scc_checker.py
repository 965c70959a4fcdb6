"""CPU answers for the strongly connected components: three independent forms that must agree (an iterative Tarjan in plain
Python, scipy's connected_components(connection="strong"), networkx), each canonicalised to comp[v] = the smallest vertex id of
v's component; numpy restatements of sizes, summary and the sorted condensation; and the generators the tests share.  The CSR is
read as a directed multigraph: duplicates and self-loops change nothing, rows may be unsorted."""
import numpy as np


def _arrays(ro, ci):
    return np.asarray(ro, dtype=np.int64), np.asarray(ci, dtype=np.int64)


def canonical(labels):
    """any labelling of a partition -> int32 labels that are the smallest member of each part"""
    labels = np.asarray(labels, dtype=np.int64)
    n = labels.shape[0]
    _, dense = np.unique(labels, return_inverse=True)
    least = np.full(int(dense.max()) + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(least, dense, np.arange(n, dtype=np.int64))
    return least[dense].astype(np.int32)


def tarjan(nodes, ro, ci):
    """Tarjan's algorithm with an explicit stack (no recursion); canonical labels"""
    ro, ci = _arrays(ro, ci)
    ro_l, ci_l = ro.tolist(), ci.tolist()
    index = [-1] * nodes
    low = [0] * nodes
    on_stack = [False] * nodes
    label = [-1] * nodes
    stack, counter, parts = [], 0, 0
    for root in range(nodes):
        if index[root] >= 0:
            continue
        work = [(root, ro_l[root])]
        index[root] = low[root] = counter
        counter += 1
        stack.append(root)
        on_stack[root] = True
        while work:
            v, at = work[-1]
            if at < ro_l[v + 1]:
                work[-1] = (v, at + 1)
                u = ci_l[at]
                if index[u] < 0:
                    index[u] = low[u] = counter
                    counter += 1
                    stack.append(u)
                    on_stack[u] = True
                    work.append((u, ro_l[u]))
                elif on_stack[u] and index[u] < low[v]:
                    low[v] = index[u]
            else:
                work.pop()
                if work and low[v] < low[work[-1][0]]:
                    low[work[-1][0]] = low[v]
                if low[v] == index[v]:
                    while True:
                        u = stack.pop()
                        on_stack[u] = False
                        label[u] = parts
                        if u == v:
                            break
                    parts += 1
    return canonical(label)


def by_scipy(nodes, ro, ci):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    ro, ci = _arrays(ro, ci)
    m = csr_matrix((np.ones(ci.shape[0], dtype=np.int8), ci.astype(np.int32), ro.astype(np.int32)), shape=(nodes, nodes))
    _, labels = connected_components(m, directed=True, connection="strong")
    return canonical(labels)


def by_networkx(nodes, ro, ci):
    import networkx as nx
    ro, ci = _arrays(ro, ci)
    g = nx.DiGraph()
    g.add_nodes_from(range(nodes))
    g.add_edges_from(zip(np.repeat(np.arange(nodes), np.diff(ro)).tolist(), ci.tolist()))
    label = np.empty(nodes, dtype=np.int64)
    for i, part in enumerate(nx.strongly_connected_components(g)):
        label[list(part)] = i
    return canonical(label)


def scc(nodes, ro, ci):
    """the reference the GPU tests compare with (scipy's: the three forms agree, tests/test_scc_cpu.py)"""
    return by_scipy(nodes, ro, ci)


def sizes(comp):
    comp = np.asarray(comp, dtype=np.int64)
    return np.bincount(comp, minlength=comp.shape[0])[comp].astype(np.int32)


def summary(comp):
    """{"components", "trivial", "largest", "largest_root"}; ties of the largest go to the smaller root"""
    comp = np.asarray(comp, dtype=np.int64)
    count = np.bincount(comp, minlength=comp.shape[0])
    roots = np.flatnonzero(count > 0)
    largest = int(count.max())
    return {"components": int(roots.shape[0]), "trivial": int((count == 1).sum()), "largest": largest,
            "largest_root": int(np.flatnonzero(count == largest)[0])}


def condensation(nodes, ro, ci, comp):
    """the distinct (comp[u], comp[v]) over the edges between components, sorted by (from, to): two int32 arrays"""
    ro, ci = _arrays(ro, ci)
    comp = np.asarray(comp, dtype=np.int64)
    a, b = comp[np.repeat(np.arange(nodes), np.diff(ro))], comp[ci]
    keys = np.unique((a * nodes + b)[a != b])
    return (keys // nodes).astype(np.int32), (keys % nodes).astype(np.int32)


def literal(nodes, ro, ci, comp):
    """(n, directed entries, components, largest, trivial, sum of comp)"""
    s = summary(comp)
    return (int(nodes), int(np.asarray(ci).shape[0]), s["components"], s["largest"], s["trivial"], int(np.asarray(comp, dtype=np.int64).sum()))


# ---------------- generators: (nodes, row_offsets int32, col_indices int32) ----------------

def from_edges(nodes, src, dst):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    ro = np.zeros(nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=nodes), out=ro[1:])
    return nodes, ro.astype(np.int32), dst[order].astype(np.int32)


def dicycle(n):
    v = np.arange(n)
    return from_edges(n, v, (v + 1) % n)


def dipath(n):
    v = np.arange(n - 1)
    return from_edges(n, v, v + 1)


def in_star(n):
    """every leaf points at the hub, vertex 0"""
    return from_edges(n, np.arange(1, n), np.zeros(n - 1, dtype=np.int64))


def out_star(n):
    return from_edges(n, np.zeros(n - 1, dtype=np.int64), np.arange(1, n))


def complete_digraph(n):
    a, b = np.divmod(np.arange(n * n), n)
    keep = a != b
    return from_edges(n, a[keep], b[keep])


def bowtie(a, core, b):
    """`a` vertices that each point into a directed cycle of `core` vertices, which points at each of `b` vertices: ids are the
    in-part, then the core, then the out-part"""
    n = a + core + b
    c = a + np.arange(core)
    src = np.concatenate([np.arange(a), c, a + np.arange(b) % core])
    dst = np.concatenate([a + np.arange(a) % core, a + (np.arange(core) + 1) % core, a + core + np.arange(b)])
    return from_edges(n, src, dst)


def two_cycle_chain(k, ascending):
    """k two-cycles (2i, 2i + 1) linked one way, pair i -> pair i + 1; ascending: ids rise along the links; else they fall
    (colouring's worst case: the largest id reaches nothing but its own pair, one component per round)"""
    pair = np.arange(k) if ascending else np.arange(k)[::-1]
    a, b = 2 * pair, 2 * pair + 1
    src = np.concatenate([a, b, b[:-1]])
    dst = np.concatenate([b, a, a[1:]])
    return from_edges(2 * k, src, dst)


def planted(block_sizes, p_in, p_out, seed):
    """Blocks that are strongly connected by construction (a directed cycle plus random edges inside, density p_in), random
    edges between blocks only from a lower block to a higher one (p_out per ordered pair of blocks, a few each), ids shuffled.
    Returns (nodes, ro, ci, comp: the planted partition in canonical labels, block: the block of every vertex)."""
    rng = np.random.default_rng(seed)
    block_sizes = np.asarray(block_sizes, dtype=np.int64)
    n = int(block_sizes.sum())
    start = np.concatenate([[0], np.cumsum(block_sizes)])
    block = np.repeat(np.arange(block_sizes.shape[0]), block_sizes)
    src, dst = [], []
    for i, size in enumerate(block_sizes.tolist()):
        v = start[i] + np.arange(size)
        if size > 1:
            src.append(v)
            dst.append(start[i] + (np.arange(size) + 1) % size)
        extra = rng.binomial(size * size, p_in) if size > 1 else 0
        src.append(start[i] + rng.integers(0, size, extra))
        dst.append(start[i] + rng.integers(0, size, extra))
    blocks = block_sizes.shape[0]
    links = rng.binomial(blocks * (blocks - 1) // 2, p_out) if blocks > 1 else 0
    lo = rng.integers(0, blocks, links)
    hi = rng.integers(0, blocks, links)
    keep = lo != hi
    lo, hi = np.minimum(lo, hi)[keep], np.maximum(lo, hi)[keep]
    for _ in range(3):  # a few edges per linked pair of blocks
        src.append(start[lo] + rng.integers(0, block_sizes[lo]))
        dst.append(start[hi] + rng.integers(0, block_sizes[hi]))
    src, dst = np.concatenate(src), np.concatenate(dst)
    shuffle = rng.permutation(n)
    nodes, ro, ci = from_edges(n, shuffle[src], shuffle[dst])
    block_of = np.empty(n, dtype=np.int64)
    block_of[shuffle] = block
    return nodes, ro, ci, canonical(block_of), block_of
