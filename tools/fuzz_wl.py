"""Randomised parity sweep of colour refinement against the checker: python tools/fuzz_wl.py [seconds] [seed] [--dry]

Graph families, all with n <= 2^9: R-MAT; G(n, p); a few hubs over a sparse background; twins (pairs of vertices with one row);
paths; disjoint copies of a small random graph.  Entries are mirrored or one-way, in shuffled order, with injected self-loops and
duplicates; the labels are absent or random from a few values, negative ones among them.  The strategy, lane_max_row, wave_max_row,
the table sizes, sig_bits (128, 8 or 2), the seed, max_rounds and the history are random.  Every case must equal the checker's rounds
bit for bit -- the colouring, the class sizes, the representatives, the state, and with certified rounds the round count, the trace
and the history -- and so must a second run of the same case under other options on the same handle.  The stable partition must also
be the splitter queue's.  --dry runs the generator and the two forms of the checker against each other alone, without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
import _wl_checker as k

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dry = "--dry" in sys.argv
budget = float(args[0]) if len(args) > 0 else 60.0
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)


def graph():
    kind = int(rng.integers(0, 6))
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
    elif kind == 3:  # twins: pairs of vertices with the same row over a random part
        core = int(rng.integers(8, 400))
        rows, cols = np.nonzero(np.triu(rng.random((core, core)) < min(1.0, 6.0 / core), 1))
        rows, cols = [rows], [cols]
        n = core
        for _ in range(int(rng.integers(1, 6))):
            ends = rng.choice(core, int(rng.integers(1, core + 1)), replace=False)
            for t in (n, n + 1):
                rows.append(np.full(ends.shape[0], t))
                cols.append(ends)
            n += 2
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        name = "twins"
    elif kind == 4:  # paths
        n = int(rng.integers(2, 513))
        cut = rng.random(n - 1) < 0.02
        rows = np.arange(n - 1)[~cut]
        cols = rows + 1
        name = "paths"
    else:  # disjoint copies
        base = int(rng.integers(2, 40))
        copies = int(rng.integers(2, 512 // base + 1))
        a, b = np.nonzero(rng.random((base, base)) < min(1.0, 3.0 / base))
        rows = np.concatenate([a + i * base for i in range(copies)])
        cols = np.concatenate([b + i * base for i in range(copies)])
        n = base * copies
        name = "copies"
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    mode = int(rng.integers(0, 3))
    if mode == 0:  # mirrored
        rows, cols = np.concatenate([rows, cols]), np.concatenate([cols, rows])
    elif mode == 1:  # one-way entries in either direction
        flip = rng.random(rows.shape[0]) < 0.5
        rows, cols = np.where(flip, cols, rows), np.where(flip, rows, cols)
    if rng.integers(0, 2):  # duplicates and self-loops
        dup = rng.integers(0, max(rows.shape[0], 1), int(rng.integers(0, rows.shape[0] // 5 + 2)) if rows.shape[0] else 0)
        loops = rng.integers(0, n, int(rng.integers(0, n // 8 + 2)))
        rows, cols = np.concatenate([rows, rows[dup], loops]), np.concatenate([cols, cols[dup], loops])
    ro, ci = k.csr_of(n, rows, cols, shuffle=rng)
    labels = rng.choice(np.array([-2147483648, -1, 0, 1, 7, 2147483647]), n).astype(np.int32) if rng.integers(0, 3) == 0 else None
    return name, n, ro, ci, labels


def options():
    return {"strategy": int(rng.integers(0, 4)), "lane_max_row": int(rng.choice([0, 1, 2, 5, 16, 1 << 20])),
            "wave_max_row": int(rng.choice([0, 3, 17, 64, 512, 1 << 20])), "table_slots": int(rng.choice([64, 128, 1024])),
            "block_slots": int(rng.choice([256, 1024, 8192])), "scratch_mib": int(rng.choice([1, 1024])),
            "sig_bits": int(rng.choice([128, 8, 2])), "seed": int(rng.integers(0, 1 << 40)), "max_repairs": 1 << 20}


def differs(p, ref, max_rounds, history, sig_bits):
    h = ref["rounds"] if max_rounds < 0 else min(max_rounds, ref["rounds"])
    want = ref["history"][h]
    colour, size, rep = p.extract()
    st = p.stats()
    want_size, want_rep = k.sizes_and_representatives(want)
    bad = []
    if not np.array_equal(colour, want):
        bad.append("colour")
    if not np.array_equal(size, want_size) or not np.array_equal(rep, want_rep) or st["classes"] != want_size.shape[0]:
        bad.append("classes")
    if st["state"] != (k.CAPPED if 0 <= max_rounds <= ref["rounds"] else k.STABLE):
        bad.append("state")
    if max_rounds >= 0 or sig_bits == 128:  # the rounds are certified one by one, or cannot be told from it
        if st["rounds"] != h or p.round_trace().tolist() != ref["trace"][:h + 1]:
            bad.append("rounds")
    if sig_bits == 128 and st["repairs"]:
        bad.append("repairs")
    if st["readbacks"] != 1 + st["rounds"] + st["repairs"] + (st["state"] == k.STABLE and max_rounds != 0):
        bad.append("readbacks")
    if history:
        got = p.history()
        if got.shape[0] != h + 1 or any(not np.array_equal(a, b) for a, b in zip(got, ref["history"])):
            bad.append("history")
    return bad, st


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci, labels = graph()
    ref = k.rounds(n, ro, ci, labels)
    assert np.array_equal(ref["colour"], k.splitters(n, ro, ci, labels)) and k.is_equitable(n, ro, ci, ref["colour"]), "the checker's two forms differ"
    cases += 1
    if dry:
        continue
    p = ga.WlProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci)
    for _ in range(2):  # the case, and the same under other options
        chosen = options()
        history = bool(rng.integers(0, 3) == 0)
        max_rounds = int(rng.choice([1, 2, 3, 64])) if history else int(rng.choice([-1, -1, 0, 1, 2, 5, 1000]))
        chosen.update({"history": int(history), "max_rounds": max_rounds})
        for key, value in chosen.items():
            assert p.set_option(key, value) == 0, key
        p.reset(labels)
        p.enact()
        bad, st = differs(p, ref, max_rounds, history, chosen["sig_bits"])
        if bad:
            print("WL MISMATCH", name, "n", n, "entries", ci.shape[0], "labels", labels is not None, chosen, bad, st,
                  {x: ref[x] for x in ("rounds", "state", "trace")})
            sys.exit(1)
    p.close()
print("fuzz ok:", cases, "cases")
