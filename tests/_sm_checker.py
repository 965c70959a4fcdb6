"""CPU restatements of subgraph matching (gunrockinst_amd/sm.py), for the tests, the fuzz tool and the smoke run.

A graph is (nodes, row_offsets, col_indices), read as the simple undirected graph: u and v are neighbours when either row holds the
other, self-loops and duplicates dropped.  A pattern is (q, pairs) with optional labels, -1 a wildcard.  Two independent counts:

  count     plain backtracking in pattern-id order, no symmetry breaking: pattern vertex i takes every vertex that is unused, fits the
            label, is adjacent to the images of its earlier pattern neighbours and, when induced, to none of its earlier
            non-neighbours.  Every embedding credits the q vertices of its image; the sums are divided by a brute-force |Aut(H)|.
  nx_count  networkx's GraphMatcher: subgraph_monomorphisms_iter (not induced) or subgraph_isomorphisms_iter (induced), with a
            node_match for labels and wildcard.

Both return (count int64 per vertex, occurrences, aut)."""
import itertools

import numpy as np

WILDCARD = -1

PATTERNS = {
    "edge": (2, [(0, 1)]),
    "wedge": (3, [(0, 1), (1, 2)]),
    "triangle": (3, [(0, 1), (1, 2), (0, 2)]),
    "p4": (4, [(0, 1), (1, 2), (2, 3)]),
    "claw": (4, [(0, 1), (0, 2), (0, 3)]),
    "c4": (4, [(0, 1), (1, 2), (2, 3), (3, 0)]),
    "paw": (4, [(0, 1), (1, 2), (0, 2), (2, 3)]),
    "diamond": (4, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)]),
    "k4": (4, list(itertools.combinations(range(4), 2))),
    "c5": (5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]),
    "house": (5, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 4), (3, 4)]),
    "bull": (5, [(0, 1), (1, 2), (0, 2), (1, 3), (2, 4)]),
    "k5": (5, list(itertools.combinations(range(5), 2))),
    "c6": (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)]),
}
AUT = {"wedge": 2, "p4": 2, "claw": 6, "c4": 8, "paw": 2, "diamond": 4, "k4": 24, "c5": 10, "house": 2, "bull": 2, "c6": 12}
GRAPHLETS = {3: ("wedge", "triangle"), 4: ("p4", "claw", "c4", "paw", "diamond", "k4")}


# ---------------- graphs ----------------

def from_edges(nodes, edges):
    """the CSR that holds every pair once, in its first vertex's row, as given"""
    edges = sorted(edges)
    ro = np.zeros(nodes + 1, np.int32)
    for a, _ in edges:
        ro[a + 1] += 1
    return nodes, np.cumsum(ro, dtype=np.int32), np.array([b for _, b in edges], np.int32).reshape(-1)


def petersen():
    return from_edges(10, [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)])


def complete(n):
    return from_edges(n, list(itertools.combinations(range(n), 2)))


def complete_bipartite(a, b):
    return from_edges(a + b, [(i, a + j) for i in range(a) for j in range(b)])


def star(leaves):
    return from_edges(leaves + 1, [(0, 1 + i) for i in range(leaves)])


def double_star(leaves):
    """two adjacent hubs 0 and 1 that share `leaves` leaves"""
    return from_edges(leaves + 2, [(0, 1)] + [(h, 2 + i) for h in (0, 1) for i in range(leaves)])


def gnp(n, p, seed):
    rng = np.random.default_rng(seed)
    return from_edges(n, [(a, b) for a, b in itertools.combinations(range(n), 2) if rng.random() < p])


def rmat(scale, edges, seed):
    """a seeded R-MAT (0.57, 0.19, 0.19), entries as drawn: duplicates, self-loops and one-way entries included"""
    rng = np.random.default_rng(seed)
    r, c = np.zeros(edges, np.int64), np.zeros(edges, np.int64)
    for _ in range(scale):
        x = rng.random(edges)
        r = (r << 1) | (x >= 0.76)
        c = (c << 1) | (((x >= 0.57) & (x < 0.76)) | (x >= 0.95))
    return from_edges(1 << scale, list(zip(r.tolist(), c.tolist())))


def read_mtx(path):
    """a Matrix Market coordinate file as a graph, entries as they stand"""
    with open(path) as f:
        lines = [l for l in f if not l.startswith("%")]
    n = int(lines[0].split()[0])
    return from_edges(n, [(int(l.split()[0]) - 1, int(l.split()[1]) - 1) for l in lines[1:] if l.strip()])


def shuffled(graph, seed):
    """the same simple graph as another CSR: entries in random rows' order and direction, with duplicates and self-loops added"""
    n, ro, ci = graph
    rng = np.random.default_rng(seed)
    edges = [(v, int(u)) for v in range(n) for u in ci[ro[v]:ro[v + 1]]]
    edges = [(b, a) if rng.integers(0, 2) else (a, b) for a, b in edges]
    edges += [edges[int(i)] for i in rng.integers(0, max(len(edges), 1), len(edges) // 3)] if edges else []
    edges += [(int(v), int(v)) for v in rng.integers(0, n, 3)] if n else []
    order = rng.permutation(len(edges))
    ro2 = np.zeros(n + 1, np.int32)
    for a, _ in edges:
        ro2[a + 1] += 1
    ro2 = np.cumsum(ro2, dtype=np.int32)
    fill, ci2 = ro2[:-1].copy(), np.zeros(len(edges), np.int32)
    for i in order:
        a, b = edges[int(i)]
        ci2[fill[a]] = b
        fill[a] += 1
    return n, ro2, ci2


def adjacency(graph):
    """one Python int per vertex: bit u of adj[v] set iff v -- u in the simple graph"""
    n, ro, ci = graph
    adj = [0] * n
    for v in range(n):
        for u in ci[ro[v]:ro[v + 1]].tolist():
            if u != v:
                adj[v] |= 1 << u
                adj[u] |= 1 << v
    return adj


# ---------------- patterns ----------------

def pattern_adjacency(q, pairs):
    adj = [[False] * q for _ in range(q)]
    for a, b in pairs:
        adj[a][b] = adj[b][a] = True
    return adj


def aut(q, pairs, plabels=None):
    """|Aut(H)| by brute force: the permutations that keep labels (the wildcard one of them) and adjacency"""
    adj = pattern_adjacency(q, pairs)
    lab = [WILDCARD] * q if plabels is None else list(plabels)
    return sum(1 for p in itertools.permutations(range(q))
               if all(lab[p[i]] == lab[i] for i in range(q)) and all(adj[i][j] == adj[p[i]][p[j]] for i in range(q) for j in range(i)))


def relabelled(q, pairs, plabels, perm):
    """the same pattern with vertex i renamed perm[i]"""
    new_labels = None
    if plabels is not None:
        new_labels = [0] * q
        for i in range(q):
            new_labels[perm[i]] = plabels[i]
    return [(perm[a], perm[b]) for a, b in pairs], new_labels


# ---------------- the two counts ----------------

def _bits(x):
    while x:
        low = x & -x
        yield low.bit_length() - 1
        x ^= low


def embeddings(graph, q, pairs, labels=None, plabels=None, induced=False):
    """(per vertex: the embeddings whose image holds it, as Python ints; the embeddings): backtracking in pattern-id order"""
    n = graph[0]
    adj, padj = adjacency(graph), pattern_adjacency(q, pairs)
    everything = (1 << n) - 1
    lab = [0] * n if labels is None else [int(x) for x in labels]
    plab = [WILDCARD] * q if plabels is None else [int(x) for x in plabels]
    fits = [everything if plab[i] == WILDCARD else sum(1 << v for v in range(n) if lab[v] == plab[i]) for i in range(q)]
    through = [0] * n
    last = {}  # the last level's candidate sets and how often each came up: expanded once at the end
    image = [0] * q

    def descend(i, used):
        cand = fits[i] & ~used
        for j in range(i):
            cand &= adj[image[j]] if padj[i][j] else (~adj[image[j]] if induced else everything)
        if not cand:
            return 0
        if i == q - 1:
            last[cand] = last.get(cand, 0) + 1
            return bin(cand).count("1")
        found = 0
        for v in _bits(cand):
            image[i] = v
            below = descend(i + 1, used | 1 << v)
            through[v] += below
            found += below
        return found

    total = descend(0, 0)
    for cand, times in last.items():
        for v in _bits(cand):
            through[v] += times
    return through, total


def count(graph, q, pairs, labels=None, plabels=None, induced=False):
    through, total = embeddings(graph, q, pairs, labels, plabels, induced)
    a = aut(q, pairs, plabels)
    assert total % a == 0 and all(x % a == 0 for x in through), "the embeddings are no multiple of |Aut(H)|"
    return np.array([x // a for x in through], np.int64).reshape(-1), total // a, a


def nx_count(graph, q, pairs, labels=None, plabels=None, induced=False):
    import networkx as nx
    from networkx.algorithms.isomorphism import GraphMatcher
    n, ro, ci = graph
    G, H = nx.Graph(), nx.Graph()
    G.add_nodes_from((v, {"label": 0 if labels is None else int(labels[v])}) for v in range(n))
    G.add_edges_from((v, int(u)) for v in range(n) for u in ci[ro[v]:ro[v + 1]] if int(u) != v)
    H.add_nodes_from((i, {"label": WILDCARD if plabels is None else int(plabels[i])}) for i in range(q))
    H.add_edges_from(pairs)
    matcher = GraphMatcher(G, H, node_match=lambda g, h: h["label"] == WILDCARD or g["label"] == h["label"])
    through, total = [0] * n, 0
    for mapping in (matcher.subgraph_isomorphisms_iter() if induced else matcher.subgraph_monomorphisms_iter()):
        total += 1
        for v in mapping:
            through[v] += 1
    a = aut(q, pairs, plabels)
    assert total % a == 0 and all(x % a == 0 for x in through)
    return np.array([x // a for x in through], np.int64).reshape(-1), total // a, a


def spanning_copies(q, pairs, other_pairs):
    """how many subgraphs of H' = (q, other_pairs) on all q vertices are copies of H = (q, pairs): embeddings / aut, not induced"""
    return count(from_edges(q, [tuple(sorted(e)) for e in other_pairs]), q, pairs)[1]


def seeded_labels(n, q, seed):
    """labels in {0, 1, 2} for the graph and in {-1, 0, 1, 2} for the pattern"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 3, n).astype(np.int32), rng.integers(-1, 3, q).astype(np.int32)
