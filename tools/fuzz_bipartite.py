"""Randomised parity sweep of the bipartite matching against the checker: python tools/fuzz_bipartite.py [seconds] [seed] [--dry]

Rectangular patterns of up to 2^9 rows and columns, tall and wide: R-MAT-like (each index drawn bit by bit with skewed quadrant
probabilities) and G(n, p), with injected empty rows and columns and duplicate entries, in shuffled order.  The strategy, the
thresholds, the schedule, the loop limits, the greedy start and a random valid start matching vary per case.  Every case must equal
the checker -- size, parts, part sizes, cover, blocks; the matching validated, the certificate (0, 0, size) -- and so must a second
run of the same case under other options on the same handle.  --dry runs the generator and the checker alone (the parts from two
different maximum matchings must agree), without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
import _bipartite_checker as k

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dry = "--dry" in sys.argv
budget = float(args[0]) if len(args) > 0 else 60.0
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)


def pattern():
    rows, cols = (int(1 << rng.integers(0, 10)) if rng.integers(0, 2) else int(rng.integers(1, 513)) for _ in range(2))
    if rng.integers(0, 2):  # R-MAT-like: the bits of a row and a column index together, quadrant by quadrant
        count = int(rng.integers(0, 6 * max(rows, cols) + 1))
        a, b, c = 0.55, 0.2, 0.2
        r, cc = np.zeros(count, np.int64), np.zeros(count, np.int64)
        for bit in range(9):
            q = rng.random(count)
            r = (r << 1) | ((q >= a + b) & (q < 1.0)).astype(np.int64)
            cc = (cc << 1) | (((q >= a) & (q < a + b)) | (q >= a + b + c)).astype(np.int64)
        r, cc = r % rows, cc % cols
        name = "rmat"
    else:
        r, cc = np.nonzero(rng.random((rows, cols)) < rng.uniform(0.0, min(1.0, 6.0 / max(rows, cols))))
        name = "gnp"
    if rng.integers(0, 2) and r.shape[0]:  # empty rows and columns: a random subset loses everything
        keep = ~np.isin(r, rng.choice(rows, rows // 4, replace=False)) & ~np.isin(cc, rng.choice(cols, cols // 4, replace=False))
        r, cc = r[keep], cc[keep]
    if rng.integers(0, 2) and r.shape[0]:  # duplicates
        dup = rng.integers(0, r.shape[0], int(rng.integers(0, r.shape[0] // 4 + 2)))
        r, cc = np.concatenate([r, r[dup]]), np.concatenate([cc, cc[dup]])
    order = rng.permutation(r.shape[0])
    return name, k.from_pairs((rows, cols), r[order], cc[order])


def start(matrix):
    """None, or a random valid matching: rows in random order take a random free entry of theirs, some of them"""
    if rng.integers(0, 2):
        return None
    (rows, cols), ro, ci = matrix
    mate_row, used = np.full(rows, -1, np.int32), np.zeros(cols, bool)
    for r in rng.permutation(rows)[:int(rng.integers(0, rows + 1))]:
        free = [c for c in ci[ro[r]:ro[r + 1]].tolist() if not used[c]]
        if free:
            mate_row[r] = free[int(rng.integers(0, len(free)))]
            used[mate_row[r]] = True
    return mate_row


def options():
    return {"strategy": int(rng.integers(0, 4)), "wave_min_row": int(rng.choice([1, 2, 5, 16, 1 << 20])),
            "block_min_row": int(rng.choice([1, 3, 17, 64, 2048])), "schedule": int(rng.integers(0, 3)),
            "loop_max_list": int(rng.choice([0, 8, 32768])), "loop_max_entries": int(rng.choice([0, 64, 8192])), "greedy": int(rng.integers(0, 2))}


def differs(p, matrix, ref):
    bad = []
    st = p.stats()
    m = p.extract_matching()
    try:
        if not (k.validate(matrix, m["mate_row"], m["mate_col"]) == ref["size"] == m["size"] == st["size"]):
            bad.append("size")
    except AssertionError as e:
        bad.append("matching: %s" % e)
    if st["state"] != ga.BIPARTITE_MAXIMUM or st["certificate"] != [0, 0, ref["size"]]:
        bad.append("certificate")
    row_part, col_part, sizes = p.extract_parts()
    if not np.array_equal(row_part, ref["row_part"]) or not np.array_equal(col_part, ref["col_part"]) or sizes != ref["part_sizes"]:
        bad.append("parts")
    row_cover, col_cover = p.extract_cover()
    if not np.array_equal(row_cover, ref["row_cover"]) or not np.array_equal(col_cover, ref["col_cover"]):
        bad.append("cover")
    row_block, col_block, blocks = p.blocks()
    if not np.array_equal(row_block, ref["row_block"]) or not np.array_equal(col_block, ref["col_block"]) or blocks != ref["blocks"]:
        bad.append("blocks")
    return bad, st


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, matrix = pattern()
    ref = k.decompose(matrix)
    cases += 1
    if dry:
        (rows, cols), ro, ci = matrix
        t = k.transpose(matrix)  # another maximum matching: the transpose's, turned round
        mc, mr = k.hopcroft_karp(t)
        other = k.decompose(matrix, (mr, mc))
        assert all(np.array_equal(ref[x], other[x]) for x in ("row_part", "col_part", "row_cover", "col_cover", "row_block", "col_block")), name
        continue
    p = ga.BipartiteProblem(instrument=bool(rng.integers(0, 2))).init(*matrix)
    for _ in range(2):  # the case, and the same under other options
        chosen = options()
        for key, value in chosen.items():
            assert p.set_option(key, value) == 0, key
        first = start(matrix)
        p.reset(first)
        p.enact()
        bad, st = differs(p, matrix, ref)
        if bad:
            print("BIPARTITE MISMATCH", name, "shape", matrix[0], "entries", matrix[2].shape[0], "start", first is not None, chosen, bad, st)
            sys.exit(1)
    p.close()
print("fuzz ok:", cases, "cases")
