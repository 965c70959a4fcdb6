"""Randomised parity sweep of the k-core decomposition against the numpy peel: python tools/fuzz_kcore.py [seconds] [seed]

Graph families: R-MAT (directed and mirrored), random COO of random density with shuffled rows, injected duplicates and
self-loops (directed or mirrored), cliques joined by random edges, stars with a few chords, paths with chords.  Every case runs
under a random schedule, compact_below, wave_min_row, device-loop thresholds and k_limit; core numbers (min(core, k_limit) for a
limited run), degeneracy, degrees, shells and the members of a random k must equal the checker's bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _kcore_checker import csr_of, members, peel, shells, simple_edges

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def graph():
    kind = int(rng.integers(0, 5))
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
    elif kind == 3:  # a star with chords between leaves
        n = int(rng.integers(2, 20000))
        hub = int(rng.integers(0, n))
        leaves = np.delete(np.arange(n), hub)
        chords = int(rng.integers(0, 3 * n))
        rows = np.concatenate([leaves, rng.integers(0, n, chords)])
        cols = np.concatenate([np.full(n - 1, hub), rng.integers(0, n, chords)])
        name = "star"
    else:  # a path in a random vertex order with a few chords: long chains of sub-rounds
        n = int(rng.integers(2, 4000))
        order = rng.permutation(n)
        chords = int(rng.integers(0, max(n // 50, 1)))
        rows = np.concatenate([order[:-1], rng.integers(0, n, chords)])
        cols = np.concatenate([order[1:], rng.integers(0, n, chords)])
        name = "path"
    dup = rng.random(rows.shape[0]) < 0.2  # injected duplicates
    rows, cols = np.where(dup, np.roll(rows, 1), rows), np.where(dup, np.roll(cols, 1), cols)
    loops = rng.integers(0, n, int(rng.integers(0, 4)))  # injected self-loops
    rows, cols = np.concatenate([rows, loops]), np.concatenate([cols, loops])
    if rng.integers(0, 2):
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    shuffle = rng.permutation(rows.shape[0])  # rows in random order inside the CSR
    ro, ci = csr_of(n, rows[shuffle], cols[shuffle])
    return name, n, ro, ci


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci = graph()
    options = {"schedule": int(rng.integers(0, 3)), "compact_below": float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0])),
               "wave_min_row": int(rng.choice([1, 2, 8, 32, 64, 65, 1000, 1 << 30])),
               "loop_max_list": int(rng.choice([0, 1, 64, 1000, 32768, 1 << 30])),
               "loop_max_entries": int(rng.choice([0, 1, 64, 1000, 8192, 1 << 30]))}
    ref, d, _, _ = peel(n, ro, ci)
    top = int(ref.max())
    k_limit = int(rng.choice([-1, -1, 0, 1, 2, max(top // 2, 0), top, top + 2]))
    want = ref if k_limit < 0 else np.minimum(ref, k_limit)
    p = ga.KcoreProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci)
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    p.reset()
    p.enact(k_limit)
    core, degeneracy = p.extract()
    sh = p.shells()
    k = int(rng.integers(0, top + 2))
    mask, nv, ne = p.members(k)
    st = p.stats()
    p.close()
    a, b = simple_edges(n, ro, ci)
    ok = (core.dtype == np.int32 and np.array_equal(core, want) and degeneracy == int(want.max()) and np.array_equal(sh, shells(want))
          and st["simple_edges"] == a.shape[0] and st["max_degree"] == int(d.max())
          and (k_limit >= 0 or st["vertices_peeled"] == n)
          and st["levels"] == np.unique(ref[(ref > 0) & ((ref < k_limit) | (k_limit < 0))]).shape[0])
    w_mask, w_nv, w_ne = members(want, a, b, k)
    ok = ok and np.array_equal(mask, w_mask) and (nv, ne) == (w_nv, w_ne)
    if not ok:
        print("KCORE MISMATCH", name, "n", n, "m", ci.shape[0], options, "k_limit", k_limit, "at", np.flatnonzero(core != want)[:8],
              degeneracy, int(want.max()), st, "members", k, (nv, ne), (w_nv, w_ne))
        sys.exit(1)
    cases += 1
print("fuzz ok:", cases, "cases")
