"""Randomised parity sweep of per-edge support and the k-truss decomposition against the numpy peel:
python tools/fuzz_truss.py [seconds] [seed]

Graph families: R-MAT (directed and mirrored) at scales 4 to 11, random COO of random density with shuffled rows, injected
duplicates and self-loops (directed or mirrored), cliques joined by random edges, stars with chords, paths with chords; sizes are
capped so that the checker stays near a second per case.  Every case runs under a random schedule, wave_min_row, device-loop
thresholds and k_limit; the edges, support, truss numbers (min(truss, k_limit) for a limited run), max_truss, classes,
vertex_truss and the members of a random k must equal the checker's bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _truss_checker import classes, csr_of, members, peel, vertex_truss

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def graph():
    kind = int(rng.integers(0, 5))
    if kind == 0:  # R-MAT, directed or mirrored
        scale = int(rng.integers(4, 12))
        g = o.rmat_seeded(scale, int(rng.integers(1, 17)) << scale, undirected=bool(rng.integers(0, 2)), seed=int(rng.integers(1, 1 << 30)))
        return "rmat", g.nodes, g.row_offsets, g.col_indices
    if kind == 1:  # random COO: any density up to nearly complete on small graphs
        n = int(rng.integers(1, 1500))
        m = int(min(n * rng.uniform(0.2, 30.0), 0.6 * n * n, 40000)) + 1
        rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
        name = "coo"
    elif kind == 2:  # cliques joined by random edges
        size, count = int(rng.integers(3, 60)), int(rng.integers(1, 8))
        n = size * count + int(rng.integers(0, 50))
        r, c = np.nonzero(np.triu(np.ones((size, size), dtype=bool), 1))
        rows = np.concatenate([k * size + r for k in range(count)] + [rng.integers(0, n, 2 * n)])
        cols = np.concatenate([k * size + c for k in range(count)] + [rng.integers(0, n, 2 * n)])
        name = "cliques"
    elif kind == 3:  # a star with chords between leaves: every chord closes a triangle through the hub
        n = int(rng.integers(2, 8000))
        hub = int(rng.integers(0, n))
        leaves = np.delete(np.arange(n), hub)
        chords = int(rng.integers(0, 3 * n))
        rows = np.concatenate([leaves, rng.integers(0, n, chords)])
        cols = np.concatenate([np.full(n - 1, hub), rng.integers(0, n, chords)])
        name = "star"
    else:  # a path in a random vertex order with short chords: chains of triangles, long chains of sub-rounds
        n = int(rng.integers(3, 4000))
        order = rng.permutation(n)
        chords = int(rng.integers(0, n))
        at = rng.integers(0, n - 2, chords)
        rows = np.concatenate([order[:-1], order[at]])
        cols = np.concatenate([order[1:], order[at + 2]])
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
    options = {"schedule": int(rng.integers(0, 2)), "wave_min_row": int(rng.choice([1, 2, 8, 32, 64, 65, 1000, 1 << 30])),
               "loop_max_list": int(rng.choice([0, 1, 64, 1000, 32768, 1 << 30])),
               "loop_max_entries": int(rng.choice([0, 1, 64, 1000, 8192, 1 << 30]))}
    a, b, tri, support, ref, levels, sub_rounds = peel(n, ro, ci)
    m = a.shape[0]
    top = int(ref.max()) if m else 0
    k_limit = int(rng.choice([-1, -1, 2, 3, max(top // 2, 2), max(top, 2), top + 2]))
    want = ref if k_limit < 0 else np.minimum(ref, k_limit)
    p = ga.TrussProblem(instrument=bool(rng.integers(0, 2)))
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    p.init(n, ro, ci)
    src, dst = p.edges()
    sup, total = p.support()
    if rng.integers(0, 2):
        p.reset()
    p.enact(k_limit)
    truss, got_top = p.extract()
    cl = p.classes()
    vt = p.vertex_truss()
    k = int(rng.integers(0, top + 2))
    mask, ne, nv = p.members(k)
    st = p.stats()
    p.close()
    peeled = ref < k_limit if k_limit >= 0 else np.ones(m, dtype=bool)
    ok = (truss.dtype == np.int32 and np.array_equal(src, a) and np.array_equal(dst, b) and np.array_equal(sup, support)
          and total == tri.shape[0] and np.array_equal(truss, want) and got_top == (int(want.max()) if m else 0)
          and np.array_equal(cl, classes(want)) and np.array_equal(vt, vertex_truss(n, want, a, b))
          and st["simple_edges"] == m and st["edges_peeled"] == int(peeled.sum())
          and st["levels"] == np.unique(ref[peeled]).shape[0] and (k_limit >= 0 or st["rounds"] == sub_rounds))
    w_mask, w_ne, w_nv = members(n, want, a, b, k)
    ok = ok and np.array_equal(mask, w_mask) and (ne, nv) == (w_ne, w_nv)
    if not ok:
        print("TRUSS MISMATCH", name, "n", n, "entries", ci.shape[0], options, "k_limit", k_limit, "support at",
              np.flatnonzero(sup != support)[:8], "truss at", np.flatnonzero(truss != want)[:8], got_top, top, st, (levels, sub_rounds),
              "members", k, (ne, nv), (w_ne, w_nv))
        sys.exit(1)
    cases += 1
print("fuzz ok:", cases, "cases")
