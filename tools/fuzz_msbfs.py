"""Randomised parity sweep of the multi-source BFS against the CPU checker: python tools/fuzz_msbfs.py [seconds] [seed]

Graph families: R-MAT (directed and undirected), random COO of random density (n in 1..3000), paths and cycles in a random vertex
order with chords; injected duplicates and self-loops, rows in random order; 1..200 sources with repeats.  Every case runs under a
random direction, inverse (a refused MSBFS_INVERSE_SELF falls back to auto), wave_min_row, alpha, beta and store_depths; the depths,
both summaries and the number of levels per batch must equal the checker's bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _msbfs_checker import depths, from_edges, source_summary, vertex_summary

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def graph():
    """(family, nodes, ro, ci)"""
    kind = int(rng.integers(0, 3))
    undirected = bool(rng.integers(0, 2))
    if kind == 0:
        scale = int(rng.integers(3, 12))
        g = o.rmat_seeded(scale, int(rng.integers(1, 17)) << scale, undirected=undirected, seed=int(rng.integers(1, 1 << 30)))
        if rng.integers(0, 2):  # as built: sorted, duplicate-free rows (the symmetry check can pass)
            return "rmat", g.nodes, g.row_offsets, g.col_indices
        n, rows, cols = g.nodes, np.repeat(np.arange(g.nodes), np.diff(g.row_offsets)), g.col_indices.astype(np.int64)
        name = "rmat+"
    elif kind == 1:  # random COO: any density up to nearly complete on small graphs
        n = int(rng.integers(1, 3001))
        m = int(min(n * rng.uniform(0.1, 12.0), 0.6 * n * n)) + int(rng.integers(0, 2))
        rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
        name = "coo"
    else:  # a path or a cycle in a random vertex order with a few chords: many levels, tiny frontiers
        n = int(rng.integers(2, 1500))
        order = rng.permutation(n)
        chords = int(rng.integers(0, max(n // 50, 1) + 1))
        closed = int(rng.integers(0, 2))
        rows = np.concatenate([order[:-1], order[-1:][:closed], rng.integers(0, n, chords)])
        cols = np.concatenate([order[1:], order[:1][:closed], rng.integers(0, n, chords)])
        name = "cycle" if closed else "path"
    if kind != 0 and undirected:
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    if rows.shape[0]:
        dup = rng.random(rows.shape[0]) < 0.2  # injected duplicates
        take = rng.integers(0, rows.shape[0], rows.shape[0])
        rows, cols = np.concatenate([rows, rows[take][dup]]), np.concatenate([cols, cols[take][dup]])
    loops = rng.integers(0, n, int(rng.integers(0, 4)))  # injected self-loops
    rows, cols = np.concatenate([rows, loops]), np.concatenate([cols, loops])
    shuffle = rng.permutation(rows.shape[0])  # rows in random order inside the CSR
    n, ro, ci = from_edges(n, rows[shuffle], cols[shuffle])
    return name, n, ro, ci


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci = graph()
    k = int(rng.integers(1, 201))
    sources = rng.integers(0, n, k).astype(np.int32)
    sources[rng.integers(0, k)] = sources[0]
    options = {"direction": int(rng.integers(0, 4)), "inverse": int(rng.integers(0, 4)),
               "wave_min_row": int(rng.choice([1, 2, 8, 16, 64, 65, 1000, 1 << 30])), "alpha": float(rng.choice([0.01, 1, 4, 1000])),
               "beta": float(rng.choice([0.01, 1, 24, 1000]))}
    store = bool(rng.integers(0, 4))
    ref = depths(n, ro, ci, sources)
    p = ga.MsbfsProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci)
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    try:
        p.reset(sources, store_depths=store)
    except RuntimeError as refused:  # the graph forced to be its own inverse and the symmetry check does not pass: the handle goes on
        assert options["inverse"] == ga.MSBFS_INVERSE_SELF and "code -5" in str(refused), refused
        assert p.set_option("inverse", ga.MSBFS_INVERSE_AUTO) == 0
        p.reset(sources, store_depths=store)
    p.enact()
    d = p.depths() if store else ref
    got_s, got_v = p.source_summary(), p.vertex_summary()
    batch = p.level_trace()[0]
    st = p.stats()
    p.close()
    want_s, want_v = source_summary(ref), vertex_summary(ref)
    levels = [int(want_s[2][first:first + 64].max()) + 1 for first in range(0, k, 64)]
    ok = (d.dtype == np.int32 and np.array_equal(d, ref) and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got_s + got_v, want_s + want_v))
          and np.bincount(batch, minlength=len(levels)).tolist() == levels and (options["inverse"] != ga.MSBFS_INVERSE_NONE or st["pull_levels"] == 0))
    if not ok:
        print("MSBFS MISMATCH", name, "n", n, "m", ci.shape[0], "k", k, options, "store", store, "depths at", np.argwhere(d != ref)[:8].tolist(),
              [np.flatnonzero(a != b)[:8].tolist() for a, b in zip(got_s + got_v, want_s + want_v)], st, levels)
        sys.exit(1)
    cases += 1
print("fuzz ok:", cases, "cases")
