"""Randomised parity sweep of label propagation against the checker: python tools/fuzz_lp.py [seconds] [seed] [--dry]

Graph families, all with n <= 2^9: R-MAT; G(n, p); a few hubs over a sparse background; disjoint cliques with a few bridges.  Entries
are mirrored or one-way, in shuffled order, with injected self-loops and duplicates; the weights are absent or random in 1 .. 9 (a
duplicate may carry another weight: the largest counts); the start labels are the ids or random.  The mode, the classes (the
checker's id-order greedy colouring or a random relabelling of it), the strategy, lane_max_row, wave_max_row, table_slots and
max_rounds are random.  Every case must equal both forms of the checker bit for bit -- labels, community, state, rounds, visits,
entries_read and the summary arrays -- and so must a second run of the same case under other options on the same handle.  --dry runs the
generator and the two forms of the checker against each other alone, without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
import _lp_checker as k

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
        rows, cols = np.nonzero(np.triu(rng.random((n, n)) < rng.uniform(0.0, min(1.0, 12.0 / n)), 1))
        name = "gnp"
    elif kind == 2:  # hubs over a sparse background
        n = int(rng.integers(40, 513))
        back = int(n * rng.uniform(0.2, 2.0))
        rows, cols = [rng.integers(0, n, back)], [rng.integers(0, n, back)]
        for _ in range(int(rng.integers(1, 4))):
            leaves = rng.choice(n, int(rng.integers(20, n)), replace=False)
            rows.append(np.full(leaves.shape[0], int(rng.integers(0, n))))
            cols.append(leaves)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        name = "hubs"
    else:  # disjoint cliques and a few bridges
        sizes = rng.integers(2, 12, int(rng.integers(1, 30)))
        n = int(sizes.sum())
        label = np.repeat(np.arange(sizes.shape[0]), sizes)
        rows, cols = np.nonzero(np.triu(label[:, None] == label[None, :], 1))
        bridges = int(rng.integers(0, sizes.shape[0] + 1))
        rows, cols = np.concatenate([rows, rng.integers(0, n, bridges)]), np.concatenate([cols, rng.integers(0, n, bridges)])
        name = "cliques"
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    flip = rng.random(rows.shape[0]) < 0.5  # one-way entries in either direction
    rows, cols = np.where(flip, cols, rows), np.where(flip, rows, cols)
    if rng.integers(0, 2):  # mirrored
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    extra = int(rng.integers(0, rows.shape[0] // 5 + 2))  # duplicates and self-loops
    dup = rng.integers(0, max(rows.shape[0], 1), extra if rows.shape[0] else 0)
    loops = rng.integers(0, n, int(rng.integers(0, n // 8 + 2)))
    rows, cols = np.concatenate([rows, rows[dup], loops]), np.concatenate([cols, cols[dup], loops])
    w = rng.integers(1, 10, rows.shape[0]) if rng.integers(0, 2) else None
    ro, ci, w = k.csr_from_pairs(n, rows, cols, w, mirror=False, shuffle=rng)
    return name, n, ro, ci, w


def options():
    return {"strategy": int(rng.integers(0, 4)), "lane_max_row": int(rng.choice([0, 1, 2, 5, 16, 1 << 20])),
            "wave_max_row": int(rng.choice([0, 3, 17, 64, 512, 1 << 20])), "table_slots": int(rng.choice([64, 128, 1024]))}


def differs(p, n, a, b, pw, ref):
    labels, community, communities = p.extract()
    st = p.stats()
    bad = [name for name in k.FIELDS if st[name] != ref[name]]
    want_community, want_count = k.community_of(ref["labels"])
    if not np.array_equal(labels, ref["labels"]):
        bad.append("labels")
    if not np.array_equal(community, want_community) or communities != want_count:
        bad.append("community")
    got, want = p.summary(), k.summary_of(n, a, b, pw, ref["labels"])
    bad += [name for name in ("size", "internal", "volume") if not np.array_equal(got[name], want[name])]
    if got["W"] != want["W"]:
        bad.append("W")
    if st["readbacks"] > st["rounds"] + 2:
        bad.append("readbacks")
    return bad, st


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci, w = graph()
    a, b, pw = k.pairs_of(n, ro, ci, w)
    mode = int(rng.integers(0, 2))
    classes = None
    if mode == k.CLASSES:
        classes = k.greedy_classes(n, a, b)
        if rng.integers(0, 2):  # other names for the classes, some of them unused (never more names than vertices)
            used = int(classes.max()) + 1
            classes = rng.permutation(min(used + int(rng.integers(0, 3)), max(n, used)))[classes].astype(np.int32)
    start = rng.integers(0, n, n).astype(np.int32) if rng.integers(0, 2) else None
    max_rounds = int(rng.choice([1, 2, 3, 1000]))
    ref = k.solve(n, a, b, pw, mode, classes, start, max_rounds)
    cases += 1
    if dry:
        continue
    p = ga.LpProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci, w)
    p.set_option("mode", mode)
    p.set_option("max_rounds", max_rounds)
    if classes is not None:
        assert p.set_classes(classes) == 0
    for _ in range(2):  # the case, and the same under other options
        chosen = options()
        for key, value in chosen.items():
            assert p.set_option(key, value) == 0
        p.reset(start)
        p.enact()
        bad, st = differs(p, n, a, b, pw, ref)
        if bad:
            print("LP MISMATCH", name, "n", n, "entries", ci.shape[0], "mode", mode, "weighted", w is not None, "start", start is not None,
                  "max_rounds", max_rounds, chosen, bad, st, {x: ref[x] for x in k.FIELDS})
            sys.exit(1)
    p.close()
print("fuzz ok:", cases, "cases")
