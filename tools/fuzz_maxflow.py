"""Randomised parity sweep of the maximum flow and the minimum cuts against the CPU checker: python tools/fuzz_maxflow.py [seconds] [seed]

Each case draws a size up to 2^12 and a density, from a graph family (directed R-MAT, random COO, a layered network, a path or cycle
with chords in a random vertex order), capacities (unit / NULL, small with zeros, wide, a few huge ones), injected parallel and
antiparallel arcs and self-loops, rows in random order, a random (src, sink), and a random schedule, wave_min_row, discharge_steps,
relabel_interval and device-loop thresholds.  A handle runs two or three pairs in a row.  The value, side[], cut[], the summary and
the pairs must equal the checker's bit for bit; flow[] and arc_flow[] must pass its validation."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
import _maxflow_checker as k

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def graph():
    """(family, nodes, rows, cols)"""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        scale = int(rng.integers(3, 13))
        g = o.rmat_seeded(scale, int(rng.integers(1, 9)) << scale, undirected=bool(rng.integers(0, 2)), seed=int(rng.integers(1, 1 << 30)))
        return "rmat", g.nodes, np.repeat(np.arange(g.nodes), np.diff(g.row_offsets)), np.asarray(g.col_indices, np.int64)
    n = int(rng.integers(2, 1 << 12))
    if kind == 1:  # random COO: from forest-like up to nearly complete on small graphs
        m = int(min(n * rng.uniform(0.2, 8.0), 0.6 * n * n)) + 1
        return "coo", n, rng.integers(0, n, m), rng.integers(0, n, m)
    if kind == 2:  # layers: arcs go one or two layers on, a few go back
        layers = int(rng.integers(2, 40))
        layer = np.sort(rng.integers(0, layers, n))
        m = int(n * rng.uniform(1.0, 6.0))
        rows = rng.integers(0, n, m)
        want = layer[rows] + rng.choice([-1, 1, 1, 1, 2], m)
        first = np.searchsorted(layer, want, "left")
        last = np.searchsorted(layer, want, "right")
        ok = last > first
        cols = first + (rng.random(m) * (last - first)).astype(np.int64)
        return "layers", n, rows[ok], cols[ok]
    order = rng.permutation(n)  # a path or a cycle in a random vertex order with a few chords: deep searches
    chords = int(rng.integers(0, max(n // 50, 1) + 1))
    closed = int(rng.integers(0, 2))
    rows = np.concatenate([order[:-1], order[-1:][:closed], rng.integers(0, n, chords)])
    cols = np.concatenate([order[1:], order[:1][:closed], rng.integers(0, n, chords)])
    if rng.integers(0, 2):  # both directions
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    return ("cycle" if closed else "path"), n, rows, cols


def capacities(m):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return None
    if kind == 1:
        return rng.integers(0, 9, m)
    if kind == 2:
        return rng.integers(0, 1 << 16, m)
    caps = rng.integers(1, 50, m)
    caps[rng.random(m) < 0.02] = 1 << 28  # (the caller leaves a pair at most one of them: it must stay under 2^31 - 1)
    return caps


t_end = time.time() + budget
cases = most_rounds = 0
while time.time() < t_end:
    name, n, rows, cols = graph()
    m = rows.shape[0]
    dup = rng.random(m) < 0.1  # injected parallel arcs, half of them reversed
    take = rng.integers(0, max(m, 1), m)
    flip = rng.random(m) < 0.5
    if m:
        extra_r, extra_c = np.where(flip, cols[take], rows[take])[dup], np.where(flip, rows[take], cols[take])[dup]
    else:
        extra_r = extra_c = np.zeros(0, np.int64)
    loops = rng.integers(0, n, int(rng.integers(0, 4)))
    rows, cols = np.concatenate([rows, extra_r, loops]), np.concatenate([cols, extra_c, loops])
    caps = capacities(rows.shape[0])
    if caps is not None and int(caps.max(initial=0)) >= 1 << 28:
        # at most one huge capacity per pair, whatever the injected copies did
        key = np.minimum(rows, cols) * n + np.maximum(rows, cols)
        _, first = np.unique(key, return_index=True)
        keep = np.zeros(rows.shape[0], bool)
        keep[first] = True
        caps = np.where(keep, caps, np.minimum(caps, 49))
    ro, ci, cap = k.csr_from_arcs(n, rows, cols, caps, shuffle=rng)
    options = {"schedule": int(rng.integers(0, 3)), "wave_min_row": int(rng.choice([1, 2, 8, 16, 64, 65, 1000, 1 << 30])),
               "discharge_steps": int(rng.choice([1, 2, 4, 16])), "relabel_interval": float(rng.choice([0, 0.1, 1.0, 4.0])),
               "loop_max_list": int(rng.choice([0, 1, 64, 1000, 32768, 1 << 30])),
               "loop_max_entries": int(rng.choice([0, 1, 64, 1000, 8192, 1 << 30]))}
    p = ga.MaxflowProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci, cap)
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    degree = np.diff(ro)
    for trial in range(int(rng.integers(2, 4))):
        if trial == 0 and degree.max(initial=0) > 0 and n > 1:  # the first pair starts at a vertex that has arcs
            s = int(rng.choice(np.flatnonzero(degree > 0)))
            t = int(rng.choice(np.delete(np.arange(n), s)))
        else:
            s, t = (int(x) for x in rng.choice(n, 2, replace=False))
        a, b, cab, cba, ref = k.solve(n, ro, ci, cap, s, t)
        p.reset(s, t)
        p.enact()
        bad = k.mismatches(p, n, ro, ci, cap, s, t, a, b, cab, cba, ref)
        st = p.stats()
        most_rounds = max(most_rounds, st["rounds"])
        if bad or st["pairs"] != a.shape[0]:
            print("MAXFLOW MISMATCH", name, "n", n, "entries", ci.shape[0], "pair", (s, t), options, bad, st)
            sys.exit(1)
        p.set_option("schedule", int(rng.integers(0, 3)))
    p.close()
    cases += 1
print("fuzz ok:", cases, "cases, at most", most_rounds, "rounds")
