"""k-clique counting timing on a device-built graph, Reset + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_clique.py <scale | gridSIDE> k [reps] [--configs "s:rows:rank,..."] [--tc]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid4096): the road-like
SIDE x SIDE grid (devgraph.grid_csr_device).  --configs: strategy:bitmap_rows:rank triples, strategy 0 auto / 1 bitmap / 2 list, rank
"none" (the (d, id) orientation) or "core" (grx_kcore's core numbers, taken on the device); the default alternates AUTO with each
forced regime under each orientation.  One handle per orientation, the configurations alternated rep by rep in one process, so they
see the same device state; all of them must give the same arrays.  --tc also times triangle counting on the same graph: the line to
hold a k = 3 run against."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--configs" in sys.argv:
    spec = sys.argv[sys.argv.index("--configs") + 1]
    args.remove(spec)
else:
    spec = "0:512:none,1:512:none,2:512:none,0:512:core,1:512:core,2:512:core"
what, k = args[0], int(args[1])
reps = int(args[2]) if len(args) > 2 else 5
configs = [(int(c.split(":")[0]), int(c.split(":")[1]), c.split(":")[2]) for c in spec.split(",")]
ro, ci = devgraph.grid_csr_device(int(what[4:])) if what.startswith("grid") else devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "bitmap", 2: "list"}
handles = {}
for rank in sorted({c[2] for c in configs}):
    if rank == "core":
        kc = ga.KcoreProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
        kc.reset(); kc.enact()
        degeneracy = kc.extract(core=False)[1]
        handles[rank] = ga.CliqueProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr(), kc.device_results()[0])
        kc.close()
        print("%s degeneracy %d" % (what, degeneracy))
    else:
        handles[rank] = ga.CliqueProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
times = {c: [] for c in configs}
stats, results = {}, {}
for rep in range(reps + 1):
    for c in configs:
        p = handles[c[2]]
        p.set_option("strategy", c[0]); p.set_option("bitmap_rows", c[1])
        p.reset(); ms = p.enact(k)
        if rep:
            times[c].append(ms)
        else:
            stats[c] = p.stats()
            results[c] = p.extract()
first = results[configs[0]]
for c in configs:
    assert results[c][1] == first[1] and results[c][0].tobytes() == first[0].tobytes(), "configurations disagree: %s" % (c,)
    t = sorted(times[c])
    st = stats[c]
    med = t[len(t) // 2]
    print("%s nodes %d entries %d k %d | %s bitmap_rows %d rank %s: enact ms median %.3f min %.3f | build ms %.3f | cliques %d bound %.4g | "
          "oriented edges %d longest out-row %d | rows bitmap %d list %d | edges bitmap %d list %d | bit-row ANDs %d (%.3f G/s) "
          "list look-ups %d launches %d" % (
              what, n, m, k, NAMES[c[0]], c[1], c[2], med, t[0], st["build_ms"], first[1], st["bound"], st["oriented_edges"],
              st["max_out_row"], st["bitmap_rows"], st["list_rows"], st["bitmap_edges"], st["list_edges"], st["bit_ands"],
              st["bit_ands"] / med / 1e6, st["list_lookups"], st["kernel_launches"]))
for p in handles.values():
    p.close()
if "--tc" in sys.argv:
    q = ga.TcProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
    t = []
    for rep in range(reps + 1):
        q.reset(); ms = q.enact()
        if rep: t.append(ms)
    t.sort()
    total = q.extract(triangles=False)[1]
    print("%s TC enact ms median %.3f min %.3f | triangles %d" % (what, t[len(t) // 2], t[0], total))
    q.close()
