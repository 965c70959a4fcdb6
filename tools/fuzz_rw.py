"""Randomised parity sweep of the random walks against the checker: python tools/fuzz_rw.py [seconds] [seed] [--dry]

Graph families, all with n <= 2^9: R-MAT (directed) and G(n, p).  The entries come as built, shuffled within their rows, or dirty
(injected self-loops, duplicates, sinks); the mode (uniform, weighted with zero weights among them, biased, both), the biases, tries,
length, seed, the start vertices, the strategy, max_grid_size and `visits` are random.  Every case must equal the vectorised form
of the checker bit for bit -- walks, lengths, visits, steps and the counters of the biased steps -- and so must a second run of the
same graph under other options on the same handle.  --dry runs the generator and the two forms of the checker against each other
alone, without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
import _rw_checker as k

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dry = "--dry" in sys.argv
budget = float(args[0]) if len(args) > 0 else 60.0
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)
KEYS = ("walks", "lengths", "visits", "steps", "ended_early", "biased_tries", "forced_fallbacks")


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
    biased = bool(rng.integers(0, 2))
    return {"weighted": bool(rng.integers(0, 2)), "bias": tuple(int(b) for b in rng.integers(0, int(rng.choice([3, 9, 65536])), 3)) if biased else (1, 1, 1),
            "tries": int(rng.choice([1, 2, 5, 32, 128])), "length": int(rng.choice([0, 1, 7, 15, 16, 17, 31, 40, 70])), "seed": int(rng.integers(0, 1 << 53)),
            "starts": rng.integers(0, n, int(rng.choice([1, 64, 100, 300]))).astype(np.int32), "strategy": int(rng.integers(0, 3)),
            "grid": int(rng.choice([0, 0, 1, 3])), "visits": bool(rng.integers(0, 2))}


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci, w = graph()
    p = None if dry else ga.RwProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci, w)
    for _ in range(2):  # the case, and the same graph under other options
        c = options(n)
        kw = {"weights": w if c["weighted"] else None, "seed": c["seed"], "bias": c["bias"], "tries": c["tries"]}
        want = k.vectorised(n, ro, ci, c["starts"], c["length"], **kw)
        if dry or cases % 8 == 0:
            other = k.scalar(n, ro, ci, c["starts"][:40], min(c["length"], 16), **kw)
            part = k.vectorised(n, ro, ci, c["starts"][:40], min(c["length"], 16), **kw)
            assert all(np.array_equal(other[key], part[key]) for key in KEYS), "the checker's forms disagree"
        cases += 1
        if dry:
            continue
        for key, value in (("strategy", c["strategy"]), ("length", c["length"]), ("seed", c["seed"]), ("weighted", int(c["weighted"])),
                           ("bias_return", c["bias"][0]), ("bias_in", c["bias"][1]), ("bias_out", c["bias"][2]), ("tries", c["tries"]),
                           ("visits", int(c["visits"]))):
            assert p.set_option(key, value) == 0, key
        p.reset(c["starts"])
        p.enact(c["grid"])
        walks, lengths, visits, steps = p.extract(visits=c["visits"])
        st = p.stats()
        bad = []
        if not np.array_equal(walks, want["walks"]):
            bad.append("walks")
        if not np.array_equal(lengths, want["lengths"]):
            bad.append("lengths")
        if c["visits"] and not np.array_equal(visits, want["visits"]):
            bad.append("visits")
        if steps != want["steps"]:
            bad.append("steps")
        if any(st[key] != want[key] for key in ("steps", "ended_early", "biased_tries", "forced_fallbacks")):
            bad.append("stats")
        if bad:
            c["starts"] = c["starts"][:8]
            print("RW MISMATCH", name, "n", n, "entries", ci.shape[0], c, bad, st, {key: want[key] for key in KEYS[3:]})
            sys.exit(1)
    if p is not None:
        p.close()
print("fuzz ok:", cases, "cases")
