"""Randomised parity sweep of subgraph matching against the checker: python tools/fuzz_sm.py [seconds] [seed] [--dry]

G(n, p) and R-MAT graphs of up to 2^7 vertices, as CSRs with duplicates, self-loops and one-way entries; random connected patterns
of 2 .. 5 vertices (6 only on graphs of up to 24 vertices) from a random spanning tree and random further edges, given with
duplicate and reversed pairs; random labels in {0, 1, 2} with wildcards in the pattern, or none; induced or not.  The symmetry
breaking, the strategy, the group threshold, the order rule and per_vertex vary per run.  Every case must equal the checker --
count[], occurrences, embeddings, aut -- and so must a second run of the same case under other options on the same handle.  --dry
runs the generator and the checker alone (its two restatements must agree on the small cases), without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
import _sm_checker as k

args = [a for a in sys.argv[1:] if not a.startswith("--")]
dry = "--dry" in sys.argv
budget = float(args[0]) if len(args) > 0 else 60.0
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)


def a_graph():
    if rng.integers(0, 2):
        scale = int(rng.integers(2, 8))
        g = k.rmat(scale, int(rng.integers(1, 4 * (1 << scale) + 1)), int(rng.integers(0, 1 << 30)))
        name = "rmat"
    else:
        n = int(rng.integers(1, 129))
        g = k.gnp(n, float(rng.uniform(0.0, min(1.0, 8.0 / n))), int(rng.integers(0, 1 << 30)))
        name = "gnp"
    if rng.integers(0, 2):
        g = k.shuffled(g, int(rng.integers(0, 1 << 30)))
    return name, g


def a_pattern(max_q):
    q = int(rng.integers(2, max_q + 1))
    order = rng.permutation(q).tolist()
    pairs = [(order[i], order[int(rng.integers(0, i))]) for i in range(1, q)]  # a random spanning tree
    for a in range(q):
        for b in range(a + 1, q):
            if rng.random() < 0.3:
                pairs.append((a, b))
    pairs += [(b, a) for a, b in pairs if rng.random() < 0.2]  # both orientations, duplicates
    return q, [pairs[int(i)] for i in rng.permutation(len(pairs))]


def options():
    return {"symmetry": int(rng.integers(0, 2)), "strategy": int(rng.integers(0, 3)), "group_max_row": int(rng.choice([1, 3, 8, 16, 1024])),
            "order": int(rng.integers(0, 3)), "per_vertex": int(rng.integers(0, 4) > 0)}


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, g = a_graph()
    q, pairs = a_pattern(6 if g[0] <= 24 else 5)
    labelled, induced = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    labels, plabels = k.seeded_labels(g[0], q, int(rng.integers(0, 1 << 30))) if labelled else (None, None)
    ref = k.count(g, q, pairs, labels, plabels, induced)
    cases += 1
    if dry:
        if g[0] <= 16:
            other = k.nx_count(g, q, pairs, labels, plabels, induced)
            assert np.array_equal(ref[0], other[0]) and ref[1:] == other[1:], (name, q, pairs)
        continue
    p = ga.SmProblem(instrument=bool(rng.integers(0, 2))).init(*g, labels)
    for _ in range(2):  # the case, and the same under other options
        chosen = options()
        for key, value in chosen.items():
            assert p.set_option(key, value) == 0, key
        p.set_pattern(q, pairs, plabels, induced)
        p.enact()
        count, occurrences, embeddings = p.extract()
        aut = p.pattern_info()["aut"]
        want = ref[0] if chosen["per_vertex"] else np.zeros_like(ref[0])
        if not np.array_equal(count, want) or (occurrences, aut, embeddings) != (ref[1], ref[2], ref[1] * ref[2]):
            print("SM MISMATCH", name, "nodes", g[0], "entries", g[2].shape[0], "q", q, "pairs", pairs, "labels", None if labels is None else labels.tolist(),
                  "plabels", None if plabels is None else plabels.tolist(), "induced", induced, chosen, "got", occurrences, aut, "want", ref[1:], p.stats())
            sys.exit(1)
    p.close()
print("fuzz ok:", cases, "cases")
