"""Subgraph-matching timing, Reset + Enact by HIP events, median and minimum of `reps` after a warm-up; also usable under rocprofv3
--kernel-trace:
python tools/one_sm.py <file.mtx | rmatSCALE | gridSIDE> [reps] [--patterns "triangle,k4,..."] [--configs "symmetry:strategy,..."] [--induced] [--families] [--work-limit X]

file.mtx: the graph as it stands (tests/_sm_checker.read_mtx); rmatSCALE (e.g. rmat20): the library's seeded R-MAT with 8 x 2^SCALE
generated entries; gridSIDE (e.g. grid4096): the 4-neighbour SIDE x SIDE mesh.  --patterns: names of gunrockinst_amd.SM_PATTERNS
(default: triangle,k4,c4,wedge,p4,paw,diamond,c5).  --configs: symmetry 0 / 1, strategy 0 auto / 1 group8 / 2 wave; the default is
the library's defaults alone.  One plain handle is timed, the configurations alternated rep by rep in one process (an Enact on
written counts resets them itself, inside the timed span); an instrumented one gives the per-kernel split and the candidate rate.
All configurations must give the same counts.  A pattern whose work bound exceeds the work limit is reported as refused.
--families also times tc, clique (k = 4) and c4 on the same graph in the same process and compares their counts with the
triangle, k4 and c4 patterns'."""
import sys, os, zlib
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


args = [a for a in sys.argv[1:] if not a.startswith("--")]
names = flag("--patterns", "triangle,k4,c4,wedge,p4,paw,diamond,c5").split(",")
spec = flag("--configs", "1:0")
work_limit = flag("--work-limit")
what = args[0]
reps = int(args[1]) if len(args) > 1 else 5
induced = "--induced" in sys.argv

import gunrockinst_amd as ga

if what.startswith("rmat"):
    from gunrockinst_amd import devgraph
    scale = int(what[4:])
    d_ro, d_ci = devgraph.rmat_csr_device(scale, 8)
    nodes, ro, ci = 1 << scale, d_ro.cpu().numpy(), d_ci.cpu().numpy()
elif what.startswith("grid"):
    side = int(what[4:])
    v = np.arange(side * side, dtype=np.int64)
    x, y = v % side, v // side
    r = np.concatenate([v[x > 0], v[x < side - 1], v[y > 0], v[y < side - 1]])
    c = np.concatenate([v[x > 0] - 1, v[x < side - 1] + 1, v[y > 0] - side, v[y < side - 1] + side])
    order = np.argsort(r, kind="stable")
    nodes, ro = side * side, np.zeros(side * side + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=nodes), out=ro[1:])
    ci = np.ascontiguousarray(c[order], np.int32)
else:
    import _sm_checker as k
    nodes, ro, ci = k.read_mtx(what)
print("%s nodes %d entries %d" % (what, nodes, ci.shape[0]))

configs = [tuple(int(x) for x in c.split(":")) for c in spec.split(",")]
STRATEGIES = {0: "auto", 1: "group8", 2: "wave"}


def median(t):
    t = sorted(t)
    return t[len(t) // 2], t[0]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


p = ga.SmProblem(False).init(nodes, ro, ci)
q = ga.SmProblem(True).init(nodes, ro, ci)
if work_limit is not None:
    p.set_option("work_limit", float(work_limit)); q.set_option("work_limit", float(work_limit))
results = {}
for name in names:
    size, pairs = ga.SM_PATTERNS[name]
    times = {c: [] for c in configs}
    stats, split, sums = {}, {}, {}
    refused = False
    for rep in range(reps + 1):
        for c in configs:
            for h in (p, q) if rep == 0 else (p,):
                h.set_option("symmetry", c[0]); h.set_option("strategy", c[1])
                h.set_pattern(size, pairs, induced=induced)
            try:
                ms = p.enact()
            except ga.SmTooLarge as e:
                refused = True
                print("%s | %s: refused, hom(T, G) = %.4g" % (what, name, p.stats()["bound"]))
                break
            if rep:
                times[c].append(ms)
            else:
                count, occurrences, _ = p.extract()
                stats[c], sums[c] = p.stats(), (occurrences, crc(count))
                q.enact()
                split[c] = q.stats()
        if refused:
            break
    if refused:
        continue
    results[name] = sums[configs[0]]
    for c in configs:
        st, sp = stats[c], split[c]
        assert sums[c] == sums[configs[0]], "configurations disagree: %s %s" % (name, c)
        t, least = median(times[c])
        enum_ms = sp["group8_ms"] + sp["wave_ms"]
        print("%s | %s%s symmetry %d strategy %s: enact ms median %.3f min %.3f | occurrences %d aut %d crc %08x | items %d (group8 %d wave %d) "
              "candidates %d bisections %d | hom(T, G) %.4g | instrumented kernel ms %.3f: bin %.3f group8 %.3f wave %.3f finish %.3f | "
              "%.3g candidates/s | build ms %.3f" % (
                  what, name, " induced" if induced else "", c[0], STRATEGIES[c[1]], t, least, sums[c][0], p.pattern_info()["aut"], sums[c][1],
                  st["items"], st["group8_items"], st["wave_items"], st["candidates"], st["bisections"], st["bound"], sp["kernel_ms"], sp["bin_ms"],
                  sp["group8_ms"], sp["wave_ms"], sp["finish_ms"], st["candidates"] / (enum_ms * 1e-3) if enum_ms > 0 else 0.0, st["build_ms"]))
p.close()
q.close()

if "--families" in sys.argv:
    def timed(problem, enact, extract):
        run = lambda: (problem.reset(), enact(problem))[1]  # (the families' reset is outside their timed span)
        run()
        out = extract(problem)
        t, least = median([run() for _ in range(reps)])
        problem.close()
        return out, t, least
    (tri, total), t, least = timed(ga.TcProblem().init(nodes, ro, ci), lambda h: h.enact(), lambda h: h.extract())
    print("%s | tc: enact ms median %.3f min %.3f | triangles %d%s" % (what, t, least, total, "" if "triangle" not in results else
          " | sm: %s" % ("identical" if results["triangle"] == (total, crc(tri.astype(np.int64))) else "DIFFERENT")))
    (cl, total), t, least = timed(ga.CliqueProblem().init(nodes, ro, ci), lambda h: h.enact(4), lambda h: h.extract())
    print("%s | clique k = 4: enact ms median %.3f min %.3f | cliques %d%s" % (what, t, least, total, "" if "k4" not in results else
          " | sm: %s" % ("identical" if results["k4"] == (total, crc(cl)) else "DIFFERENT")))
    c4 = ga.C4Problem().init(nodes, ro, ci)
    c4.set_option("edges", 0)
    (cy, total), t, least = timed(c4, lambda h: h.enact(), lambda h: h.extract())
    print("%s | c4: enact ms median %.3f min %.3f | cycles %d%s" % (what, t, least, total, "" if "c4" not in results else
          " | sm: %s" % ("identical" if results["c4"] == (total, crc(cy)) else "DIFFERENT")))
