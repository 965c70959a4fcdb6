"""Randomised parity sweep of vertex similarity against the checker: python tools/fuzz_sim.py [seconds] [seed] [--dry]

Graph families, all with n <= 2^9: R-MAT; G(n, p); random bipartite graphs (the user-item graphs top-k similarity is asked on); a few
hubs over a sparse background.  The entries come mirrored, one-way, shuffled or with injected self-loops and duplicates; the metric,
strategy, lane_max, table_slots, block_slots, scratch_mib, max_grid_size, k and skip_neighbors are random.  Every case must equal the
dense form of the checker bit for bit in both modes -- common, num, den, score; ids, count, candidates -- and so must a second run of
the same case under other options on the same handle; the regimes of the sources and the wedges walked must equal the restated
rule's.  --dry runs the generator and the two forms of the checker against each other alone, without a GPU."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gunrockinst_amd as ga
from oracle import gr_oracle as o
import _c4_checker as c4
import _sim_checker as k

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
    forms = c4.entry_forms((n, rows, cols), rng)
    form = list(forms)[int(rng.integers(0, len(forms)))]
    return name + "/" + form, n, forms[form][0], forms[form][1]


def options():
    return {"metric": int(rng.integers(0, 4)), "skip_neighbors": int(rng.integers(0, 2)), "strategy": int(rng.integers(0, 5)),
            "lane_max": int(rng.choice([0, 1, 8, 64, 1 << 20])), "table_slots": int(rng.choice([64, 128, 1024])),
            "block_slots": int(rng.choice([256, 1024, 8192])), "scratch_mib": int(rng.choice([1, 1024]))}


t_end = time.time() + budget
cases = 0
while time.time() < t_end:
    name, n, ro, ci = graph()
    ref = k.Dense(n, ro, ci)
    count, rows = int(rng.choice([0, 1, 63, 200, 1000])), int(rng.choice([0, 1, 5, 64, n]))
    u, v = rng.integers(0, n, count).astype(np.int32), rng.integers(0, n, count).astype(np.int32)
    sources = rng.integers(0, n, rows).astype(np.int32) if rows != n else rng.permutation(n).astype(np.int32)
    if cases % 8 == 0:  # the second form, on a sample: it is the slow one
        other = k.Sets(n, ro, ci)
        some = sources[:20]
        assert np.array_equal(ref.wd, other.wd) and k.same(ref.pairs(u[:50], v[:50], k.JACCARD), other.pairs(u[:50], v[:50], k.JACCARD)) is None and \
            k.same(ref.topk(some, 7, k.OVERLAP, True), other.topk(some, 7, k.OVERLAP, True)) is None, "the checker's forms disagree"
    cases += 1
    if dry:
        continue
    p = ga.SimProblem(instrument=bool(rng.integers(0, 2))).init(n, ro, ci)
    for _ in range(2):  # the case, and the same under other options
        chosen = options()
        for key, value in chosen.items():
            assert p.set_option(key, value) == 0
        grid, kk = int(rng.choice([0, 0, 1, 7])), int(rng.choice([1, 2, 16, 63, 64]))
        p.reset()
        p.pairs(u, v, grid)
        pair_stats = p.stats()
        p.topk(sources, kk, grid)
        st = p.stats()
        got_pairs, got_topk = p.extract_pairs(), p.extract_topk()
        bad = []
        what = k.same(got_pairs, ref.pairs(u, v, chosen["metric"]))
        if what:
            bad.append("pairs: " + what)
        what = k.same(got_topk, ref.topk(sources, kk, chosen["metric"], bool(chosen["skip_neighbors"])))
        if what:
            bad.append("topk: " + what)
        regimes = [k.pair_regime(int(ref.d[x]) + int(ref.d[y]), chosen["strategy"], chosen["lane_max"]) for x, y in zip(u, v)]
        if count and (pair_stats["lane_pairs"], pair_stats["wave_pairs"]) != (regimes.count(k.LANE), regimes.count(k.WAVE)):
            bad.append("pair regimes")
        wd = [int(ref.wd[s]) for s in sources]
        regimes = [k.topk_regime(w, chosen["strategy"], chosen["table_slots"], chosen["block_slots"]) for w in wd]
        if rows and [st[r + "_sources"] for r in ("wave", "block", "global")] != [regimes.count(r) for r in (k.WAVE, k.BLOCK, k.GLOBAL)]:
            bad.append("source regimes")
        if rows and (st["wedges_walked"] != sum(wd) or st["candidates"] != int(got_topk["candidates"].sum())):
            bad.append("wedges walked or candidates")
        if st["simple_edges"] != ref.a.shape[0] or st["wedges"] != int(ref.wd.sum()):
            bad.append("edges or wedges")
        if bad:
            print("SIM MISMATCH", name, "n", n, "entries", ci.shape[0], chosen, "grid", grid, "k", kk, "pairs", count, "sources", rows, bad, st)
            sys.exit(1)
    p.close()
print("fuzz ok:", cases, "cases")
