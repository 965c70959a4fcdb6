"""Randomised parity sweep of the sparse product against the checker: python tools/fuzz_spgemm.py [seconds] [seed] [--dry]

Shapes with rows, inner and cols <= 300: uniform entries, a few dense rows of A or of B over a sparse background, empty matrices;
values in a small signed range (so that products cancel), non-negative, or absent; the entries in row order or shuffled, with
duplicates.  The right operand is A itself, its transpose or a matrix of its own; strategy, lane_max, table_slots, block_slots,
scratch_mib, max_grid_size and pattern_only are random.  Every case must equal the expand form of the checker bit for bit -- offsets,
cols, vals -- and so must a second run of the same case under other options on the same handle; the regimes of the rows, the products
and the bound must equal the restated rules'.  --dry runs the generator and the two forms of the checker against each other alone,
without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
import _spgemm_checker as k

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dry = "--dry" in sys.argv
budget = float(args[0]) if len(args) > 0 else 60.0
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)


def matrix(rows, cols):
    kind = int(rng.integers(0, 4))
    if rows == 0 or cols == 0 or kind == 0 and rng.random() < 0.3:
        r = c = np.zeros(0, dtype=np.int64)
    elif kind <= 1:  # uniform
        entries = int(rows * rng.uniform(0.0, 8.0))
        r, c = rng.integers(0, rows, entries), rng.integers(0, cols, entries)
    else:  # a few dense rows over a sparse background
        entries = int(rows * rng.uniform(0.0, 2.0))
        r, c = [rng.integers(0, rows, entries)], [rng.integers(0, cols, entries)]
        for _ in range(int(rng.integers(1, 4))):
            width = int(rng.integers(1, cols + 1))
            r.append(np.full(width, int(rng.integers(0, rows))))
            c.append(rng.choice(cols, width, replace=False))
        r, c = np.concatenate(r), np.concatenate(c)
    values = int(rng.integers(0, 3))
    v = None if values == 0 else rng.integers(-3 if values == 1 else 0, 4, len(r))
    m = k.from_coo((rows, cols), r, c, v)
    return k.shuffled(m, rng) if rng.random() < 0.5 else m


def case():
    right = int(rng.integers(0, 3))
    rows, inner, cols = (int(x) for x in rng.integers(0, 301, 3))
    if right == k.SELF:
        inner = rows
    a = matrix(rows, inner)
    b = a if right == k.SELF else k.transpose(a) if right == k.TRANSPOSE else matrix(inner, cols)
    return right, a, b


def options():
    return {"strategy": int(rng.integers(0, 5)), "lane_max": int(rng.choice([0, 1, 8, 64])), "table_slots": int(rng.choice([64, 128, 1024])),
            "block_slots": int(rng.choice([256, 1024, 8192])), "scratch_mib": int(rng.choice([1, 1024])), "pattern_only": int(rng.random() < 0.25)}


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    right, a, b = case()
    ref = k.expand(a, b)
    if cases % 4 == 0:
        what = k.same(ref, k.dense(a, b))
        assert what is None, "the checker's forms disagree: " + what
    cases += 1
    if dry:
        continue
    p = ga.SpgemmProblem(instrument=bool(rng.integers(0, 2))).init(a[0], a[1], a[2], a[3])
    if right == k.GIVEN:
        assert p.set_right(b[0], b[1], b[2], b[3]) == 0
    else:
        assert p.set_option("right", right) == 0
    for _ in range(2):  # the case, and the same under other options
        chosen = options()
        for key, value in chosen.items():
            assert p.set_option(key, value) == 0
        grid = int(rng.choice([0, 0, 1, 7]))
        p.enact(grid)
        got, st = p.extract(values=not chosen["pattern_only"]), p.stats()
        bad = []
        what = k.same(got, ref, values=not chosen["pattern_only"])
        if what:
            bad.append(what)
        want = k.regime_stats(a, b, chosen["strategy"], chosen["lane_max"], chosen["table_slots"], chosen["block_slots"])
        if {key: st[key] for key in want} != want:
            bad.append("regimes")
        if st["products"] != int(k.work(a, b).sum()) or st["nnz"] != ref["cols"].shape[0] or st["bound"] != float(k.bound(a, b)):
            bad.append("products, nnz or bound")
        if bad:
            print("SPGEMM MISMATCH right", right, "shapes", a[0], b[0], "entries", len(a[2]), len(b[2]), chosen, "grid", grid, bad, st)
            sys.exit(1)
    p.close()
print("fuzz ok:", cases, "cases")
