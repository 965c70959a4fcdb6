"""Max-flow timing on a device-built directed R-MAT, Reset + Enact, median of `reps` per schedule; also usable under rocprofv3
--kernel-trace:  python tools/one_maxflow.py <scale> [reps] [--configs "schedule[:wave_min_row:discharge_steps:relabel_interval],..."] [--no-cpu] [--trace]

The graph: 2^scale vertices, 8 * 2^scale generated arcs (devgraph.rmat_tuples_device, read directed), capacities torch.randint(0, 17)
under the seed `scale`; src is the first vertex of largest out-degree, sink the first other vertex of largest in-degree.  --configs:
default "0,1,2" (AUTO, ROUNDS, DEVICE_LOOP); the configurations are alternated rep by rep in one process, so they see the same device
state.  Every repetition is timed twice: the HIP-event time of Enact, and the host's clock around Reset + Enact.  Unless --no-cpu is
given, scipy's Dinic (scipy.sparse.csgraph.maximum_flow) is timed on the same graph in the same run for scale, and its value must be
the GPU's.  --trace prints the phases of the first configuration."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

scale = int(sys.argv[1])
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 3
spec = sys.argv[sys.argv.index("--configs") + 1] if "--configs" in sys.argv else "0,1,2"
DEFAULTS = (0, 16, 4, 0.1)  # the library's; a configuration that names fewer values takes the rest from here
configs = [tuple(float(x) for x in c.split(":")) for c in spec.split(",")]
configs = [c + DEFAULTS[len(c):] for c in configs]
n = 1 << scale
rows, cols = devgraph.rmat_tuples_device(scale, 8 << scale)
ro, ci = devgraph.csr_from_tuples_device(n, rows, cols, undirected=False)
m = int(ci.shape[0])
torch.manual_seed(scale)
cap = torch.randint(0, 17, (m,), dtype=torch.int32, device="cuda")
src = devgraph.largest_degree_source(ro)[0]
indegree = torch.bincount(ci.long(), minlength=n)
indegree[src] = -1
sink = int(torch.nonzero(indegree == indegree.max())[0])
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "rounds", 2: "device_loop"}
OPTIONS = ("schedule", "wave_min_row", "discharge_steps", "relabel_interval")
p = ga.MaxflowProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr(), cap.data_ptr())
times = {c: [] for c in configs}
walls = {c: [] for c in configs}
stats, results, traces = {}, {}, {}
for rep in range(reps + 1):
    for c in configs:
        for name, value in zip(OPTIONS, c):
            assert p.set_option(name, value) == 0
        t0 = time.perf_counter()
        p.reset(src, sink); ms = p.enact()
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            times[c].append(ms)
            walls[c].append(wall)
        else:
            stats[c] = p.stats()
            results[c] = p.extract()
            traces[c] = p.phase_trace()
first = results[configs[0]]
summary = p.summary()
for c in configs:
    assert results[c]["value"] == first["value"] and all(results[c][key].tobytes() == first[key].tobytes() for key in ("side", "cut")), \
        "configurations disagree: %s" % (c,)
    t, w = sorted(times[c]), sorted(walls[c])
    st = stats[c]
    med = t[len(t) // 2]
    print("rmat%d nodes %d arcs %d src %d sink %d | %s %s: enact ms median %.3f min %.3f | reset + enact (host clock) ms median %.3f | build ms %.3f | "
          "pairs %d | value %d sides %d / %d / %d cut pairs %d / %d | rounds %d global relabels %d pushes %d relabels %d launches %d read-backs %d | "
          "entries read %d = %.2f per pair (%.2f G/s)" % (
              scale, n, m, src, sink, NAMES[int(c[0])], ":".join("%g" % x for x in c[1:]), med, t[0], w[len(w) // 2], st["build_ms"], st["pairs"],
              summary["value"], summary["side0"], summary["side1"], summary["side2"], summary["cut0"], summary["cut1"], st["rounds"],
              st["global_relabels"], st["pushes"], st["relabels"], st["kernel_launches"], st["readbacks"], st["entries_read"],
              st["entries_read"] / max(st["pairs"], 1), st["entries_read"] / max(med, 1e-9) / 1e6))
if "--trace" in sys.argv:
    kind, rounds, ms = traces[configs[0]]
    for i in range(kind.shape[0]):
        print("phase %s: %d rounds, %.3f ms" % (("preflow", "return", "cut")[kind[i]], rounds[i], ms[i]))
    print("trace total %.3f ms" % ms.sum())
a, b, cab, cba = p.pairs()
p.close()
if "--no-cpu" not in sys.argv:
    import scipy.sparse as sp
    from scipy.sparse.csgraph import maximum_flow
    capacity = sp.csr_matrix((np.concatenate([cab, cba]), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n))
    t0 = time.perf_counter()
    got = maximum_flow(capacity, src, sink, method="dinic")
    cpu = (time.perf_counter() - t0) * 1e3
    assert got.flow_value == summary["value"], "scipy's value %d differs" % got.flow_value
    print("rmat%d scipy dinic on the merged matrix (one CPU thread): %.1f ms, value %d" % (scale, cpu, got.flow_value))
