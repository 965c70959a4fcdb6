"""Bipartite-matching timing, Reset + Enact, median and minimum of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_bipartite.py <file.mtx | rmatSCALE | gridSIDE> [reps] [--configs "greedy:schedule:strategy,..."] [--scipy] [--blocks] [--trace]

file.mtx: the matrix as it stands (tests/_bipartite_checker.read_pattern); rmatSCALE (e.g. rmat20): a bipartite R-MAT pattern of
2^SCALE x 2^SCALE with 8 x 2^SCALE generated entries (the library's seeded generator: row and column of a tuple are a row and a
column), duplicates kept; gridSIDE (e.g. grid2048): the 5-point-stencil matrix of a SIDE x SIDE mesh.  --configs: greedy 0 / 1,
schedule 0 auto / 1 rounds / 2 device loop, strategy 0 auto / 1 lane / 2 wave / 3 block; the default is the library's defaults alone.
One plain handle is timed, the configurations alternated rep by rep in one process; an instrumented one gives the per-kernel split.
All configurations must give the same size, parts and cover.  --scipy also runs scipy.sparse.csgraph.maximum_bipartite_matching on
the host, compares the size and prints its time; --blocks adds the fine decomposition (the square graph and SCC) and its time;
--trace prints the phase trace."""
import sys, os, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def flag(name, default=None):
    if name not in sys.argv:
        return default
    value = sys.argv[sys.argv.index(name) + 1]
    args.remove(value)
    return value


def csr(rows, cols, r, c):
    order = np.argsort(r, kind="stable")
    ro = np.zeros(rows + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=rows), out=ro[1:])
    return (rows, cols), ro, np.ascontiguousarray(c[order], np.int32)


args = [a for a in sys.argv[1:] if not a.startswith("--")]
spec = flag("--configs", "1:0:0")
what = args[0]
reps = int(args[1]) if len(args) > 1 else 5

import gunrockinst_amd as ga

if what.startswith("rmat"):
    from gunrockinst_amd import devgraph
    scale = int(what[4:])
    r, c = devgraph.rmat_tuples_device(scale, 8 << scale)
    shape, ro, ci = csr(1 << scale, 1 << scale, r.cpu().numpy().astype(np.int64), c.cpu().numpy())
elif what.startswith("grid"):
    side = int(what[4:])
    v = np.arange(side * side, dtype=np.int64)
    x, y = v % side, v // side
    r = np.concatenate([v, v[x > 0], v[x < side - 1], v[y > 0], v[y < side - 1]])
    c = np.concatenate([v, v[x > 0] - 1, v[x < side - 1] + 1, v[y > 0] - side, v[y < side - 1] + side])
    shape, ro, ci = csr(side * side, side * side, r, c)
else:
    import _bipartite_checker as k
    shape, ro, ci = k.read_pattern(what)
print("%s shape %s entries %d" % (what, shape, ci.shape[0]))

configs = [tuple(int(x) for x in c.split(":")) for c in spec.split(",")]
SCHEDULES = {0: "auto", 1: "rounds", 2: "loop"}
STRATEGIES = {0: "auto", 1: "lane", 2: "wave", 3: "block"}


def setup(p, c):
    p.set_option("greedy", c[0]); p.set_option("schedule", c[1]); p.set_option("strategy", c[2])


def checksum(p):
    parts = p.extract_parts()
    cover = p.extract_cover()
    return "parts %s crc %08x" % (parts[2], zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in parts[:2] + cover)))


p = ga.BipartiteProblem(False).init(shape, ro, ci)
q = ga.BipartiteProblem(True).init(shape, ro, ci)
times = {c: [] for c in configs}
stats, split, sums = {}, {}, {}
for rep in range(reps + 1):
    for c in configs:
        setup(p, c)
        p.reset(); ms = p.enact()
        if rep:
            times[c].append(ms)
        else:
            stats[c] = p.stats()
            sums[c] = checksum(p)
            setup(q, c)
            q.reset(); q.enact()
            split[c] = q.stats()
            if "--trace" in sys.argv:
                levels, flipped, tms = p.phase_trace()
                for i in range(len(levels)):
                    print("  %s %d: levels %d augmentations %d ms %.3f" % ("phase" if i + 1 < len(levels) else "rows ", i, levels[i], flipped[i], tms[i]))
for c in configs:
    st, sp = stats[c], split[c]
    assert sums[c] == sums[configs[0]] and st["size"] == stats[configs[0]]["size"], "configurations disagree: %s" % (c,)
    t = sorted(times[c])
    print("%s | greedy %d schedule %s strategy %s: enact ms median %.3f min %.3f | size %d greedy pairs %d augmentations %d | phases %d levels %d "
          "(+ %d from the rows), %d in the device loop | launches %d read-backs %d | certificate %s | columns lane %d wave %d block %d | "
          "instrumented kernel ms %.3f: roots %.3f levels %.3f loop %.3f augment %.3f rest %.3f | transpose ms %.3f | %s" % (
              what, c[0], SCHEDULES[c[1]], STRATEGIES[c[2]], t[len(t) // 2], t[0], st["size"], st["greedy_pairs"], st["augmentations"], st["phases"],
              st["levels"], st["vertical_levels"], st["loop_levels"], st["kernel_launches"], st["readbacks"], st["certificate"],
              st["regime_columns"][0], st["regime_columns"][1], st["regime_columns"][2], sp["kernel_ms"], sp["roots_ms"], sp["level_ms"],
              sp["loop_ms"], sp["augment_ms"], sp["rest_ms"], st["build_ms"], sums[c]))
if "--blocks" in sys.argv:
    t0 = time.time()
    blocks = p.blocks()[2]
    print("%s | fine decomposition: %d blocks, %.3f s with the read-backs" % (what, blocks, time.time() - t0))
if "--scipy" in sys.argv:
    import scipy.sparse as sp_
    from scipy.sparse.csgraph import maximum_bipartite_matching
    a = sp_.csr_matrix((np.ones(ci.shape[0], np.int8), ci.copy(), ro.copy()), shape=shape)
    a.sum_duplicates()
    t0 = time.time()
    size = int((maximum_bipartite_matching(a, perm_type="column") >= 0).sum())
    seconds = time.time() - t0
    print("%s | scipy maximum_bipartite_matching %.3f s, size %d: %s" % (what, seconds, size, "identical" if size == stats[configs[0]]["size"] else "DIFFERENT"))
    assert size == stats[configs[0]]["size"]
p.close()
q.close()
