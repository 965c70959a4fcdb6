"""Randomised parity sweep of the neighbourhood sampling against the checker: python tools/fuzz_sample.py [seconds] [seed] [--dry]

Graph families, all with n <= 2^9: R-MAT (directed) and G(n, p).  The entries come as built, shuffled within their rows, or dirty
(injected self-loops, duplicates, sinks); the mode (without replacement, with it, weighted with zero weights among them), the fanout
list (-1 among the fanouts), the seed, the seeds, the strategy, max_grid_size, `long_row` and `eids` are random.  Every case must equal
the vectorised form of the checker bit for bit -- vertices, vertex_ptr, offsets, cols, eids, edge_ptr -- and so must a second run of
the same graph under other options on the same handle.  --dry runs the generator and the two forms of the checker against each other
alone, without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
import _sample_checker as k

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dry = "--dry" in sys.argv
budget = float(args[0]) if len(args) > 0 else 60.0
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)


def graph():
    if int(rng.integers(0, 2)) == 0:
        scale = int(rng.integers(2, 10))
        g = o.rmat_seeded(scale, int(rng.integers(1, 9)) << scale, undirected=bool(rng.integers(0, 2)), seed=int(rng.integers(1, 1 << 30)))
        n = g.nodes
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.row_offsets))
        cols = np.asarray(g.col_indices).astype(np.int64)
        name = "rmat"
    else:
        n = int(rng.integers(1, 513))
        rows, cols = np.nonzero(rng.random((n, n)) < rng.uniform(0.0, min(1.0, 16.0 / n)))
        name = "gnp"
    form = ("built", "shuffled", "dirty")[int(rng.integers(0, 3))]
    if form == "dirty" and rows.shape[0]:
        extra = int(rng.integers(1, 2 + rows.shape[0] // 4))
        loops = rng.integers(0, n, extra)
        again = rng.integers(0, rows.shape[0], extra)
        rows, cols = np.concatenate([rows, loops, rows[again]]), np.concatenate([cols, loops, cols[again]])
        keep = rows % int(rng.integers(2, 9)) != 0  # sinks
        rows, cols = rows[keep], cols[keep]
    weights = rng.integers(0, int(rng.choice([2, 10, 2 ** 31])), rows.shape[0])
    n, ro, ci, w = k.csr(n, rows, cols, weights)
    if form != "built":
        ci, w = k.shuffled_rows(ro, ci, w, rng)
    return name + "/" + form, n, ro, ci, w


def options(n):
    mode = int(rng.integers(0, 3))  # without replacement, with it, weighted
    hops = int(rng.choice([1, 2, 3, 5]))
    return {"replace": mode > 0, "weighted": mode == 2, "fanouts": [int(rng.choice([-1, 1, 2, 3, 5, 8, 17, 33, 64])) for _ in range(hops)],
            "seed": int(rng.integers(0, 1 << 53)), "seeds": rng.permutation(n)[:int(rng.choice([1, 7, 64, 100, 300]))].astype(np.int32),
            "strategy": int(rng.integers(0, 3)), "grid": int(rng.choice([0, 0, 1, 3])), "long_row": int(rng.choice([8, 9, 64, 4096])),
            "eids": bool(rng.integers(0, 4))}


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci, w = graph()
    p = None if dry else ga.SampleProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci, w)
    for _ in range(2):  # the case, and the same graph under other options
        c = options(n)
        kw = {"weights": w, "replace": c["replace"], "weighted": c["weighted"], "seed": c["seed"]}
        want = k.vectorised(n, ro, ci, c["seeds"], c["fanouts"], **kw)
        if dry or cases % 8 == 0:
            other = k.scalar(n, ro, ci, c["seeds"][:40], c["fanouts"][:2], **kw)
            part = k.vectorised(n, ro, ci, c["seeds"][:40], c["fanouts"][:2], **kw)
            assert k.same(other, part), "the checker's forms disagree"
        cases += 1
        if dry:
            continue
        first = (("replace", 1), ("weighted", int(c["weighted"]))) if c["replace"] else (("weighted", 0), ("replace", 0))
        for key, value in first + (("strategy", c["strategy"]), ("seed", c["seed"]), ("long_row", c["long_row"]), ("eids", int(c["eids"]))):
            assert p.set_option(key, value) == 0, key
        p.set_fanouts(c["fanouts"])
        p.reset(c["seeds"])
        p.enact(c["grid"])
        got = p.extract(eids=c["eids"])
        bad = [key for key in k.KEYS if (key != "eids" or c["eids"]) and not np.array_equal(got[key], want[key])]
        if bad:
            c["seeds"] = c["seeds"][:8]
            print("SAMPLE MISMATCH", name, "n", n, "entries", ci.shape[0], c, bad, p.stats())
            sys.exit(1)
    if p is not None:
        p.close()
print("fuzz ok:", cases, "cases")
