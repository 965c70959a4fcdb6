"""Randomised parity sweep of the maximal independent set / greedy colourings against the sequential greedy pass:
python tools/fuzz_mis.py [seconds] [seed]

Graph families: R-MAT (directed and mirrored), random COO with duplicates and self-loops, chains, stars, sparse forests.
Order: a hashed seed, or random int32 priorities -- a narrow range (-2..2: ties everywhere, the id decides) or the full range.
Every case, in all three modes, must give the checker's `ids` bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _mis_checker import MODES, SET, greedy

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
        scale = int(rng.integers(4, 14))
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


def order(n):
    kind = int(rng.integers(0, 3))
    if kind == 0:
        return int(rng.integers(0, 1 << 32))  # a seed: hashed priorities
    if kind == 1:
        return rng.integers(-2, 3, n).astype(np.int32)
    return rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci = graph()
    prio = order(n)
    hashed = isinstance(prio, int)
    p = ga.MisProblem().init(n, ro, ci, None if hashed else prio, prio if hashed else 0)
    for mode in MODES:
        p.reset()
        p.enact(mode)
        ids, summary = p.extract()
        ref = greedy(n, ro, ci, prio, mode)
        want = int(ref.sum()) if mode == SET else int(ref.max())
        if not np.array_equal(ids, ref) or summary != want:
            print("MIS MISMATCH", name, "mode", mode, "n", n, "m", ci.shape[0], "order", "seed %d" % prio if hashed else "priorities",
                  "at", np.flatnonzero(ids != ref)[:8], summary, want)
            sys.exit(1)
    p.close()
    cases += 1
print("fuzz ok:", cases, "runs")
