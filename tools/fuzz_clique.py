"""Randomised parity sweep of k-clique counting against the checker: python tools/fuzz_clique.py [seconds] [seed] [--dry]

Graph families, all with n <= 2^10: R-MAT; G(n, p) with p up to 0.3 (and an average degree the checker can follow); cliques of 6 .. 20
vertices planted in a sparse background; complete multipartite graphs.  Entries are mirrored or one-way, in shuffled order, with
injected self-loops and duplicates.  k, bitmap_rows, the strategy and the kind of rank (none, core numbers, a permutation, all equal
and negative, reversed degrees) are random.  Every case must equal the checker's recursion bit for bit, and so must a second run of
the same graph under another configuration on a handle of its own.

A case is skipped only when the checker's own work estimate (tests/_clique_checker.py work_estimate: at least the calls of its
recursion) exceeds WORK_BUDGET; more than one skip in ten cases fails the sweep.  --dry runs the generator and the checker alone,
without a GPU, to show that rate."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
from _clique_checker import count, work_estimate
from _tc_checker import csr_of, simple_edges

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dry = "--dry" in sys.argv
budget = float(args[0]) if len(args) > 0 else 60.0
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)
WORK_BUDGET = 1_500_000  # recursion calls of the checker per case: about a second


def graph():
    kind = int(rng.integers(0, 4))
    if kind == 0:  # R-MAT
        scale = int(rng.integers(3, 11))
        g = o.rmat_seeded(scale, int(rng.integers(1, 9)) << scale, undirected=False, seed=int(rng.integers(1, 1 << 30)))
        n = g.nodes
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.row_offsets))
        cols = g.col_indices.astype(np.int64)
        name = "rmat"
    elif kind == 1:  # G(n, p): p up to 0.3, the average degree up to 24
        n = int(rng.integers(2, 1025))
        p = rng.uniform(0.0, min(0.3, 24.0 / n))
        rows, cols = np.nonzero(np.triu(rng.random((n, n)) < p, 1))
        name = "gnp"
    elif kind == 2:  # planted cliques in a sparse background
        n = int(rng.integers(24, 1025))
        back = int(n * rng.uniform(0.5, 3.0))
        rows, cols = [rng.integers(0, n, back)], [rng.integers(0, n, back)]
        for _ in range(int(rng.integers(1, 5))):
            members = rng.choice(n, int(rng.integers(6, 21)), replace=False)
            r, c = np.nonzero(np.triu(np.ones((members.shape[0],) * 2, dtype=bool), 1))
            rows.append(members[r])
            cols.append(members[c])
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        name = "planted"
    else:  # complete multipartite
        parts = rng.integers(1, 9, int(rng.integers(2, 8)))
        label = rng.permutation(np.repeat(np.arange(parts.shape[0]), parts))
        n = int(label.shape[0])
        rows, cols = np.nonzero(np.triu(label[:, None] != label[None, :], 1))
        name = "multipartite"
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    flip = rng.random(rows.shape[0]) < 0.5  # one-way entries in either direction
    rows, cols = np.where(flip, cols, rows), np.where(flip, rows, cols)
    if rng.integers(0, 2):  # mirrored
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    extra = int(rng.integers(0, rows.shape[0] // 5 + 2))  # duplicates and self-loops
    dup = rng.integers(0, max(rows.shape[0], 1), extra if rows.shape[0] else 0)
    loops = rng.integers(0, n, int(rng.integers(0, n // 8 + 2)))
    rows, cols = np.concatenate([rows, rows[dup], loops]), np.concatenate([cols, cols[dup], loops])
    shuffle = rng.permutation(rows.shape[0])
    ro, ci = csr_of(n, rows[shuffle], cols[shuffle])
    return name, n, ro, ci


def config(n, ro, ci):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        rank = None
    elif kind == 1:
        rank = None if dry else ga.gunrock_kcore(n, ro, ci)[0]
    elif kind == 2:
        rank = rng.permutation(n).astype(np.int32)
    elif kind == 3:
        rank = np.full(n, -int(rng.integers(1, 1 << 31)), np.int32)
    else:
        a, b = simple_edges(n, ro, ci)
        rank = -(np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.int32)
    return {"strategy": int(rng.integers(0, 3)), "bitmap_rows": int(rng.choice([32, 33, 64, 100, 512, 1024]))}, kind, rank


def run(n, ro, ci, k, options, rank, instrument):
    p = ga.CliqueProblem(instrument=instrument).init(n, ro, ci, rank)
    for key, value in options.items():
        assert p.set_option(key, value) == 0
    p.reset()
    p.enact(k)
    cl, total = p.extract()
    st = p.stats()
    p.close()
    return cl, total, st


t_end = time.time() + budget
cases = skipped = 0
while time.time() < t_end:
    name, n, ro, ci = graph()
    k = int(rng.integers(3, 7))
    cases += 1
    work = work_estimate(n, ro, ci, k)
    if work > WORK_BUDGET:
        skipped += 1
        continue
    ref, ref_total = count(n, ro, ci, k)
    if dry:
        continue
    for _ in range(2):  # the case, and one other configuration of itself
        options, rank_kind, rank = config(n, ro, ci)
        cl, total, st = run(n, ro, ci, k, options, rank, bool(rng.integers(0, 2)))
        ok = cl.dtype == np.int64 and np.array_equal(cl, ref) and total == ref_total and int(cl.sum()) == k * total
        if not ok:
            print("CLIQUE MISMATCH", name, "n", n, "entries", ci.shape[0], "k", k, options, "rank kind", rank_kind, "at",
                  np.flatnonzero(cl != ref)[:8], total, ref_total, st)
            sys.exit(1)
if skipped * 10 > cases:
    print("CLIQUE FUZZ SKIPPED TOO MUCH:", skipped, "of", cases)
    sys.exit(1)
print("fuzz ok:", cases - skipped, "runs,", skipped, "skipped")
