"""Randomised parity sweep of the heavy-edge matching and its contraction against the CPU checker: python tools/fuzz_matching.py [seconds] [seed]

Each case draws a size up to 2^12 and a density, from a graph family (R-MAT, random COO, a path or cycle with chords in a random vertex
order, a few hubs over shared leaves), read undirected or with one-way entries only, injected duplicates and self-loops, rows in
random order, weights (NULL, one value only, a small range with ties, wide, the int32 extremes), a seed, and a random schedule,
wave_min_row and device-loop thresholds.  A handle runs two or three schedules in a row.  in_matching, mate, medge, the summary, the
pairs and the round count must equal the checker's bit for bit, and so must one contraction, with or without vertex weights."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
import _matching_checker as k

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def graph():
    """(family, nodes, rows, cols)"""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        scale = int(rng.integers(3, 13))
        g = o.rmat_seeded(scale, int(rng.integers(1, 9)) << scale, undirected=False, seed=int(rng.integers(1, 1 << 30)))
        return "rmat", g.nodes, np.repeat(np.arange(g.nodes), np.diff(g.row_offsets)), np.asarray(g.col_indices, np.int64)
    n = int(rng.integers(1, 1 << 12))
    if kind == 1:  # random COO: from forest-like up to nearly complete on small graphs
        m = int(min(n * rng.uniform(0.0, 8.0), 0.6 * n * n))
        return "coo", n, rng.integers(0, n, m), rng.integers(0, n, m)
    if kind == 2:  # a path or a cycle in a random vertex order with a few chords: many rounds
        order = rng.permutation(n)
        chords = int(rng.integers(0, max(n // 50, 1) + 1))
        closed = int(rng.integers(0, 2))
        rows = np.concatenate([order[:-1], order[-1:][:closed], rng.integers(0, n, chords)])
        cols = np.concatenate([order[1:], order[:1][:closed], rng.integers(0, n, chords)])
        return ("cycle" if closed else "path"), n, rows, cols
    hubs = int(rng.integers(1, 5))  # hubs over shared leaves: long rows, most pointers answered elsewhere
    n = max(n, hubs + 1)
    m = int(n * rng.uniform(0.5, 3.0))
    return "hubs", n, rng.integers(0, hubs, m), rng.integers(hubs, n, m)


def weights(m):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return None
    if kind == 1:
        return np.full(m, int(rng.integers(-(1 << 31), 1 << 31)))
    if kind == 2:
        return rng.integers(-2, 3, m)
    if kind == 3:
        return rng.integers(-(1 << 31), 1 << 31, m)
    return rng.choice(np.array([-(1 << 31), -(1 << 31) + 1, 0, (1 << 31) - 2, (1 << 31) - 1]), m)


t_end = time.time() + budget
cases = most_rounds = overflows = 0
while time.time() < t_end:
    name, n, rows, cols = graph()
    m = rows.shape[0]
    if m:
        dup = rng.random(m) < rng.choice([0.0, 0.1, 0.5])  # injected duplicates, half of them reversed
        take = rng.integers(0, m, m)
        flip = rng.random(m) < 0.5
        rows, cols = (np.concatenate([rows, np.where(flip, cols[take], rows[take])[dup]]),
                      np.concatenate([cols, np.where(flip, rows[take], cols[take])[dup]]))
    loops = rng.integers(0, n, int(rng.integers(0, 4)))
    rows, cols = np.concatenate([rows, loops]), np.concatenate([cols, loops])
    mirror = bool(rng.integers(0, 2))
    w = weights(rows.shape[0])
    if mirror and w is not None and rng.integers(0, 2):  # the two directions of an entry disagree: the larger one counts
        ro, ci, we = k.csr_from_pairs(n, np.concatenate([rows, cols]), np.concatenate([cols, rows]),
                                      np.concatenate([w, rng.permutation(w)]), mirror=False, shuffle=rng)
    else:
        ro, ci, we = k.csr_from_pairs(n, rows, cols, w, mirror=mirror, shuffle=rng)
    seed = int(rng.choice([0, 1, int(rng.integers(0, 1 << 32))]))
    options = {"wave_min_row": int(rng.choice([1, 2, 8, 16, 64, 65, 1000, 1 << 30])),
               "loop_max_list": int(rng.choice([0, 1, 64, 1000, 32768, 1 << 30])),
               "loop_max_entries": int(rng.choice([0, 1, 64, 1000, 65536, 1 << 30]))}
    a, b, pw, ref, count = k.solve(n, ro, ci, we, seed)
    p = ga.MatchingProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci, we, seed)
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    for trial in range(int(rng.integers(2, 4))):
        schedule = int(rng.integers(0, 3))
        p.set_option("schedule", schedule)
        p.reset()
        p.enact()
        bad = k.mismatches(p, n, a, b, pw, ref)
        st = p.stats()
        most_rounds = max(most_rounds, st["rounds"])
        if bad or st["pairs"] != a.shape[0] or st["rounds"] != count:
            print("MATCHING MISMATCH", name, "n", n, "entries", ci.shape[0], "seed", seed, "schedule", schedule, options, bad, st, "rounds form", count)
            sys.exit(1)
    vw = None if rng.integers(0, 2) else rng.integers(-3, 1 << int(rng.integers(1, 31)), n).astype(np.int32)
    try:
        want = k.contract(n, a, b, pw, ref["mate"], vw)
        assert k.same_coarse(want, k.contract_sparse(n, a, b, pw, ref["mate"], vw))
    except k.Overflow:
        want = None
    try:
        p.contract(vw)
        got = p.coarse_extract()
    except ga.MatchingOverflow:
        got = None
        overflows += 1
    if (want is None) != (got is None) or (want is not None and not k.same_coarse(got, want)):
        print("CONTRACT MISMATCH", name, "n", n, "entries", ci.shape[0], "seed", seed, options, "overflow" if want is None else "coarse nodes %d" % want[1])
        sys.exit(1)
    p.close()
    cases += 1
print("fuzz ok:", cases, "cases, at most", most_rounds, "rounds,", overflows, "overflows")
