"""Randomised parity sweep of triangle counting against the numpy checker: python tools/fuzz_tc.py [seconds] [seed]

Graph families: R-MAT (directed and mirrored), random COO of random density with shuffled rows, injected duplicates and
self-loops (directed or mirrored), cliques joined by random edges, stars with a few chords.  Every case runs under a random
strategy, staging budget and lane threshold; triangles, total, degrees, clustering coefficients and transitivity must equal
the checker's bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _tc_checker import clustering, csr_of, oriented

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def graph():
    kind = int(rng.integers(0, 4))
    if kind == 0:  # R-MAT, directed or mirrored
        scale = int(rng.integers(4, 13))
        g = o.rmat_seeded(scale, int(rng.integers(1, 17)) << scale, undirected=bool(rng.integers(0, 2)), seed=int(rng.integers(1, 1 << 30)))
        return "rmat", g.nodes, g.row_offsets, g.col_indices
    if kind == 1:  # random COO: any density up to nearly complete on small graphs
        n = int(rng.integers(1, 3000))
        m = int(min(n * rng.uniform(0.2, 40.0), 0.6 * n * n)) + 1
        rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
        name = "coo"
    elif kind == 2:  # cliques joined by random edges
        size, count = int(rng.integers(3, 120)), int(rng.integers(1, 12))
        n = size * count + int(rng.integers(0, 50))
        r, c = np.nonzero(np.triu(np.ones((size, size), dtype=bool), 1))
        rows = np.concatenate([k * size + r for k in range(count)] + [rng.integers(0, n, 2 * n)])
        cols = np.concatenate([k * size + c for k in range(count)] + [rng.integers(0, n, 2 * n)])
        name = "cliques"
    else:  # a star with chords between leaves
        n = int(rng.integers(2, 20000))
        hub = int(rng.integers(0, n))
        leaves = np.delete(np.arange(n), hub)
        chords = int(rng.integers(0, 3 * n))
        rows = np.concatenate([leaves, rng.integers(0, n, chords)])
        cols = np.concatenate([np.full(n - 1, hub), rng.integers(0, n, chords)])
        name = "star"
    dup = rng.random(rows.shape[0]) < 0.2  # injected duplicates
    rows, cols = np.where(dup, np.roll(rows, 1), rows), np.where(dup, np.roll(cols, 1), cols)
    if rng.integers(0, 2):
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    shuffle = rng.permutation(rows.shape[0])  # rows in random order inside the CSR
    ro, ci = csr_of(n, rows[shuffle], cols[shuffle])
    return name, n, ro, ci


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci = graph()
    options = {"strategy": int(rng.integers(0, 4)), "lds_entries": int(rng.choice([1, 2, 7, 33, 64, 500, 4096, 8192])),
               "lane_max_row": int(rng.choice([0, 1, 8, 32, 64, 1000]))}
    p = ga.TcProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci)
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    p.reset()
    p.enact()
    tri, total = p.extract()
    coeff, trans = p.clustering()
    st = p.stats()
    p.close()
    ref, ref_total, d, longest, _ = oriented(n, ro, ci)
    ref_coeff, ref_trans = clustering(ref, d, ref_total)
    ok = (tri.dtype == np.int64 and np.array_equal(tri, ref) and total == ref_total and st["max_out_row"] == longest
          and coeff.tobytes() == ref_coeff.tobytes() and trans == ref_trans)
    if not ok:
        print("TC MISMATCH", name, "n", n, "m", ci.shape[0], options, "at", np.flatnonzero(tri != ref)[:8], total, ref_total, st)
        sys.exit(1)
    cases += 1
print("fuzz ok:", cases, "runs")
