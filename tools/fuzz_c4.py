"""Randomised parity sweep of 4-cycle counting against the checker: python tools/fuzz_c4.py [seconds] [seed] [--dry]

Graph families, all with n <= 2^9: R-MAT; G(n, p); random bipartite graphs (the butterflies the primitive is named for); a few hubs
over a sparse background.  The entries come mirrored, one-way, shuffled or with injected self-loops and duplicates; the strategy,
lane_max_wedges, table_slots, block_slots, scratch_mib, edges and max_grid_size are random.  Every case must equal the dense form of
the checker bit for bit -- cycles, edge_cycles, total, and the canonical edges -- and so must a second run of the same case under
other options on the same handle; the wedges and the bound must equal the rank-ordered form's.  --dry runs the generator and the two
forms of the checker against each other alone, without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
import _c4_checker as k

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dry = "--dry" in sys.argv
budget = float(args[0]) if len(args) > 0 else 60.0
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)


def graph():
    kind = int(rng.integers(0, 4))
    if kind == 0:  # R-MAT
        scale = int(rng.integers(2, 10))
        g = o.rmat_seeded(scale, int(rng.integers(1, 9)) << scale, undirected=False, seed=int(rng.integers(1, 1 << 30)))
        n = g.nodes
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.row_offsets))
        cols = g.col_indices.astype(np.int64)
        name = "rmat"
    elif kind == 1:  # G(n, p)
        n = int(rng.integers(1, 513))
        rows, cols = np.nonzero(np.triu(rng.random((n, n)) < rng.uniform(0.0, min(1.0, 16.0 / n)), 1))
        name = "gnp"
    elif kind == 2:  # bipartite: a left side of l vertices, in random positions
        n = int(rng.integers(2, 513))
        l = int(rng.integers(1, n))
        place = rng.permutation(n)
        r, c = np.nonzero(rng.random((l, n - l)) < rng.uniform(0.0, min(1.0, 24.0 / n)))
        rows, cols = place[r], place[l + c]
        name = "bipartite"
    else:  # hubs over a sparse background
        n = int(rng.integers(40, 513))
        back = int(n * rng.uniform(0.2, 2.0))
        rows, cols = [rng.integers(0, n, back)], [rng.integers(0, n, back)]
        for _ in range(int(rng.integers(1, 4))):
            leaves = rng.choice(n, int(rng.integers(20, n)), replace=False)
            rows.append(np.full(leaves.shape[0], int(rng.integers(0, n))))
            cols.append(leaves)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        name = "hubs"
    forms = k.entry_forms((n, rows, cols), rng)
    form = list(forms)[int(rng.integers(0, len(forms)))]
    return name + "/" + form, n, forms[form][0], forms[form][1]


def options():
    return {"strategy": int(rng.integers(0, 5)), "lane_max_wedges": int(rng.choice([0, 1, 4, 16, 32])),
            "table_slots": int(rng.choice([64, 128, 1024])), "block_slots": int(rng.choice([256, 1024, 8192])),
            "scratch_mib": int(rng.choice([1, 1024])), "edges": int(rng.integers(0, 2))}


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci = graph()
    cycles, edge, total = k.dense(n, ro, ci)
    ref = k.ranked(n, ro, ci)
    assert np.array_equal(cycles, ref["cycles"]) and np.array_equal(edge, ref["edge_cycles"]) and total == ref["total"], "the checker's forms disagree"
    cases += 1
    if dry:
        continue
    p = ga.C4Problem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci)
    src, dst = p.edges()
    for _ in range(2):  # the case, and the same under other options
        chosen = options()
        for key, value in chosen.items():
            assert p.set_option(key, value) == 0
        grid = int(rng.choice([0, 0, 1, 7]))
        p.reset()
        p.enact(grid)
        got, got_total = p.extract()
        st = p.stats()
        bad = []
        if not np.array_equal(got, cycles):
            bad.append("cycles")
        if got_total != total:
            bad.append("total")
        if chosen["edges"] and not np.array_equal(p.extract_edges(), edge):
            bad.append("edge_cycles")
        if not (np.array_equal(src, ref["src"]) and np.array_equal(dst, ref["dst"])):
            bad.append("edges")
        if st["wedges"] != ref["wedges"] or st["bound"] != ref["bound"]:
            bad.append("wedges or bound")
        if sum(st[r + "_wedges"] for r in ("lane", "wave", "block", "global")) != int(ref["W"][ref["W"] >= 2].sum()):
            bad.append("regime wedges")
        if bad:
            print("C4 MISMATCH", name, "n", n, "entries", ci.shape[0], chosen, "grid", grid, bad, st, "want total", total)
            sys.exit(1)
    p.close()
print("fuzz ok:", cases, "cases")
