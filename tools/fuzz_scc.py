"""Randomised parity sweep of the strongly connected components against the CPU checker: python tools/fuzz_scc.py [seconds] [seed]

Graph families: directed R-MAT, random COO of random density, planted partitions (known by construction), cycles and paths in a
random vertex order with chords, two-cycle chains; injected duplicates and self-loops, rows in random order.  Every case runs
under a random schedule, pivot_phase, trim, pair_trim, wave_min_row and device-loop thresholds; comp, the count, sizes, summary and the
condensation must equal the checker's bit for bit."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _scc_checker import condensation, from_edges, planted, scc, sizes, summary, two_cycle_chain

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def graph():
    """(family, nodes, ro, ci, the answer when the construction gives it)"""
    kind = int(rng.integers(0, 5))
    known = None
    if kind == 0:  # directed R-MAT
        scale = int(rng.integers(4, 13))
        g = o.rmat_seeded(scale, int(rng.integers(1, 17)) << scale, undirected=False, seed=int(rng.integers(1, 1 << 30)))
        return "rmat", g.nodes, g.row_offsets, g.col_indices, None
    if kind == 1:  # random COO: any density up to nearly complete on small graphs
        n = int(rng.integers(1, 3000))
        m = int(min(n * rng.uniform(0.2, 12.0), 0.6 * n * n)) + 1
        rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
        name = "coo"
    elif kind == 2:  # planted blocks
        blocks = rng.choice([1, 2, 3, 17, 64, 65, 300], int(rng.integers(1, 60)))
        n, ro, ci, known, _ = planted(blocks, float(rng.uniform(0, 0.01)), float(rng.uniform(0, 0.2)), int(rng.integers(1, 1 << 30)))
        rows, cols = np.repeat(np.arange(n), np.diff(ro)), ci.astype(np.int64)
        name = "planted"
    elif kind == 3:  # a cycle or a path in a random vertex order with a few chords: long chains of levels and sub-rounds
        n = int(rng.integers(2, 4000))
        order = rng.permutation(n)
        chords = int(rng.integers(0, max(n // 50, 1) + 1))
        closed = int(rng.integers(0, 2))
        rows = np.concatenate([order[:-1], order[-1:][:closed], rng.integers(0, n, chords)])
        cols = np.concatenate([order[1:], order[:1][:closed], rng.integers(0, n, chords)])
        name = "cycle" if closed else "path"
    else:
        n, ro, ci = two_cycle_chain(int(rng.integers(1, 300)), bool(rng.integers(0, 2)))
        rows, cols = np.repeat(np.arange(n), np.diff(ro)), ci.astype(np.int64)
        name = "chain"
    dup = rng.random(rows.shape[0]) < 0.2  # injected duplicates
    take = rng.integers(0, rows.shape[0], rows.shape[0])
    rows, cols = np.concatenate([rows, rows[take][dup]]), np.concatenate([cols, cols[take][dup]])
    loops = rng.integers(0, n, int(rng.integers(0, 4)))  # injected self-loops
    rows, cols = np.concatenate([rows, loops]), np.concatenate([cols, loops])
    shuffle = rng.permutation(rows.shape[0])  # rows in random order inside the CSR
    n, ro, ci = from_edges(n, rows[shuffle], cols[shuffle])
    return name, n, ro, ci, known


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci, known = graph()
    options = {"schedule": int(rng.integers(0, 3)), "pivot_phase": int(rng.integers(0, 2)), "trim": int(rng.integers(0, 2)), "pair_trim": int(rng.integers(0, 2)),
               "wave_min_row": int(rng.choice([1, 2, 8, 32, 64, 65, 1000, 1 << 30])),
               "loop_max_list": int(rng.choice([0, 1, 64, 1000, 32768, 1 << 30])),
               "loop_max_entries": int(rng.choice([0, 1, 64, 1000, 8192, 1 << 30]))}
    ref = scc(n, ro, ci)
    if known is not None:
        assert np.array_equal(ref, known), "the checker misses a planted partition"
    p = ga.SccProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci)
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    p.reset()
    p.enact()
    comp, components = p.extract()
    size, s = p.sizes(), p.summary()
    f, t, count = p.condensation()
    st = p.stats()
    p.close()
    ref_f, ref_t = condensation(n, ro, ci, ref)
    ok = (comp.dtype == np.int32 and np.array_equal(comp, ref) and s == summary(ref) and components == s["components"]
          and np.array_equal(size, sizes(ref)) and count == ref_f.shape[0] and np.array_equal(f, ref_f) and np.array_equal(t, ref_t)
          and (options["trim"] == 1 or st["trimmed"] == 0) and (options["pivot_phase"] == 1 or st["pivot_component"] == 0))
    if not ok:
        print("SCC MISMATCH", name, "n", n, "m", ci.shape[0], options, "at", np.flatnonzero(comp != ref)[:8], components, s, summary(ref), st,
              "condensation", count, ref_f.shape[0])
        sys.exit(1)
    cases += 1
print("fuzz ok:", cases, "cases")
