"""Randomised parity sweep of the biconnected components against the CPU checker: python tools/fuzz_bcc.py [seconds] [seed]

Graph families: undirected R-MAT, random COO of random density, planted trees of blocks (known by construction), cycles and paths in
a random vertex order with chords; injected duplicates and self-loops, rows in random order, one-way entries, permuted ids.  Every
case runs under a random schedule, wave_min_row and device-loop thresholds; bcc, the two masks, tecc, block sizes, the summary and the
block-cut tree must equal the checker's bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _bcc_checker import from_edges, mismatches, planted, relabel, same, solve

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def graph():
    """(family, nodes, ro, ci, the answer when the construction gives it)"""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        scale = int(rng.integers(4, 12))
        g = o.rmat_seeded(scale, int(rng.integers(1, 9)) << scale, undirected=True, seed=int(rng.integers(1, 1 << 30)))
        return "rmat", g.nodes, g.row_offsets, g.col_indices, None
    if kind == 1:  # random COO: from a forest-like sparsity up to nearly complete on small graphs
        n = int(rng.integers(1, 2000))
        m = int(min(n * rng.uniform(0.2, 6.0), 0.6 * n * n)) + 1
        rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
        name, known = "coo", None
    elif kind == 2:
        n, ro, ci, _, _, known = planted(int(rng.integers(1, 1 << 30)), int(rng.integers(10, 3000)), int(rng.integers(1, 5)), int(rng.integers(0, 9)))
        rows, cols = np.repeat(np.arange(n), np.diff(ro)), ci.astype(np.int64)
        name = "planted"
    else:  # a cycle or a path in a random vertex order with a few chords: long chains of levels
        n = int(rng.integers(2, 3000))
        order = rng.permutation(n)
        chords = int(rng.integers(0, max(n // 50, 1) + 1))
        closed = int(rng.integers(0, 2))
        rows = np.concatenate([order[:-1], order[-1:][:closed], rng.integers(0, n, chords)])
        cols = np.concatenate([order[1:], order[:1][:closed], rng.integers(0, n, chords)])
        name, known = ("cycle" if closed else "path"), None
    dup = rng.random(rows.shape[0]) < 0.2  # injected duplicates (some of them reversed: one-way entries become two-way)
    take = rng.integers(0, rows.shape[0], rows.shape[0])
    flip = rng.random(rows.shape[0]) < 0.5
    extra_r, extra_c = np.where(flip, cols[take], rows[take])[dup], np.where(flip, rows[take], cols[take])[dup]
    loops = rng.integers(0, n, int(rng.integers(0, 4)))  # injected self-loops
    rows, cols = np.concatenate([rows, extra_r, loops]), np.concatenate([cols, extra_c, loops])
    graph = from_edges(n, np.stack([rows, cols], axis=1), symmetric=False, shuffle=rng)
    if known is None and rng.integers(0, 2):  # permuted ids (a planted answer is tied to its ids)
        graph = relabel(graph, rng.permutation(n))
    return (name,) + graph + (known,)


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci, known = graph()
    options = {"schedule": int(rng.integers(0, 3)), "wave_min_row": int(rng.choice([1, 2, 8, 16, 64, 65, 1000, 1 << 30])),
               "loop_max_list": int(rng.choice([0, 1, 64, 1000, 32768, 1 << 30])),
               "loop_max_entries": int(rng.choice([0, 1, 64, 1000, 8192, 1 << 30]))}
    a, b, ref = solve(n, ro, ci)
    if known is not None:
        assert same(ref, known), "the checker misses a planted answer"
    p = ga.BccProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci)
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    p.reset()
    p.enact()
    bad = mismatches(p, n, a, b, ref)
    st = p.stats()
    p.close()
    if bad or st["simple_edges"] != a.shape[0]:
        print("BCC MISMATCH", name, "n", n, "entries", ci.shape[0], options, bad, st)
        sys.exit(1)
    cases += 1
print("fuzz ok:", cases, "cases")
