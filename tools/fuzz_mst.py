"""Randomised parity sweep of the minimum spanning forest against the Kruskal checker: python tools/fuzz_mst.py [seconds] [seed]

Graph families: R-MAT (directed and mirrored), random COO with duplicates and self-loops, chains, stars, sparse forests.
Weights: a narrow range (1..2: ties everywhere, the tie-break decides) or the full int32 range, independent per entry or equal on
both copies of an edge.  Every case must give the checker's `selected` bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _mst_checker import entry_rows, kruskal

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def coo_csr(n, rows, cols):
    """unsorted rows kept as drawn (stable by row only): duplicates, parallel edges and self-loops survive"""
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    return np.searchsorted(rows, np.arange(n + 1)).astype(np.int32), cols.astype(np.int32)


def graph():
    kind = int(rng.integers(0, 5))
    if kind == 0:  # R-MAT, directed or mirrored
        scale = int(rng.integers(4, 15))
        g = o.rmat_seeded(scale, int(rng.integers(1, 17)) << scale, undirected=bool(rng.integers(0, 2)), seed=int(rng.integers(1, 1 << 30)))
        return "rmat", g.nodes, g.row_offsets, g.col_indices
    n = int(rng.integers(1, 20000))
    if kind == 1:  # random COO with duplicates and self-loops, sometimes mirrored
        m = int(n * rng.uniform(0.2, 6.0))
        rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
        dup = rng.random(m) < 0.2
        cols = np.where(dup, np.roll(cols, 1), cols)
        rows = np.where(dup, np.roll(rows, 1), rows)
        if rng.integers(0, 2):
            rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
        name = "coo"
    elif kind == 2:  # chain in a random vertex order
        perm = rng.permutation(n)
        rows, cols = perm[:-1], perm[1:]
        if rng.integers(0, 2):
            rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
        name = "chain"
    elif kind == 3:  # star around a random hub
        hub = int(rng.choice([0, n - 1, int(rng.integers(0, n))]))
        leaves = np.delete(np.arange(n), hub)
        rows, cols = leaves, np.full(leaves.shape[0], hub)
        if rng.integers(0, 2):
            rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
        name = "star"
    else:  # sparse forest: random trees over random vertex subsets, plus isolated vertices
        parent = rng.integers(0, np.maximum(np.arange(n), 1))
        keep = (np.arange(n) > 0) & (rng.random(n) < 0.7)
        rows, cols = np.arange(n)[keep], parent[keep]
        if rng.integers(0, 2):
            rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
        name = "forest"
    ro, ci = coo_csr(n, rows, cols)
    return name, n, ro, ci


def weights(ro, ci):
    m = ci.shape[0]
    narrow = bool(rng.integers(0, 2))
    lo, hi = (1, 3) if narrow else (-(1 << 31), 1 << 31)
    if rng.integers(0, 2):  # equal on both copies of an edge: a hash of the vertex pair
        rows = entry_rows(ro)
        a, b = np.minimum(rows, ci).astype(np.uint64), np.maximum(rows, ci).astype(np.uint64)
        salt = np.uint64(int(rng.integers(1, 1 << 30)))
        h = (a * np.uint64(0x9E3779B97F4A7C15) + b * np.uint64(0xC2B2AE3D27D4EB4F) + salt) >> np.uint64(11)
        return (lo + (h % np.uint64(hi - lo)).astype(np.int64)).astype(np.int32)
    return rng.integers(lo, hi, m, dtype=np.int64).astype(np.int32)


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci = graph()
    w = weights(ro, ci)
    sel, total, count = ga.gunrock_mst(n, ro, ci, w)
    ref, ref_total, ref_count = kruskal(n, ro, ci, w)
    if not np.array_equal(sel, ref) or total != ref_total or count != ref_count:
        print("MST MISMATCH", name, "n", n, "m", ci.shape[0], "at", np.flatnonzero(sel != ref)[:8], total, ref_total, count, ref_count)
        sys.exit(1)
    cases += 1
print("fuzz ok:", cases, "runs")
