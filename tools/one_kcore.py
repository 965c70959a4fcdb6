"""k-core timing on a device-built graph, Reset + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_kcore.py <scale | gridSIDE | pathN> [reps] [--configs "schedule:compact_below:wave_min_row[:loop_max_list:loop_max_entries],..."] [--cc] [--tc] [--trace]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid4096): the road-like
SIDE x SIDE grid (devgraph.grid_csr_device); pathN (e.g. path1048576): a path of N vertices.  --configs: default
"0:0.75:16,1:0:16,2:0.75:16" (the library's defaults, the plain form, the device loop everywhere); the configurations are
alternated rep by rep in one process, so they see the same device state.  --cc / --tc also time CC / TC on the same graph, for
scale; --trace prints the ten longest levels of the first configuration."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
spec = sys.argv[sys.argv.index("--configs") + 1] if "--configs" in sys.argv else "0:0.75:16,1:0:16,2:0.75:16"
DEFAULTS = (0, 0.75, 16, 32768, 8192)  # the library's; a configuration that names fewer values takes the rest from here
configs = [tuple(float(x) for x in c.split(":")) for c in spec.split(",")]
configs = [c + DEFAULTS[len(c):] for c in configs]
if what.startswith("grid"):
    ro, ci = devgraph.grid_csr_device(int(what[4:]))
elif what.startswith("path"):
    n = int(what[4:])
    rows = np.concatenate([np.arange(n - 1), np.arange(1, n)])  # both directions of every edge, rows ascending
    cols = np.concatenate([np.arange(1, n), np.arange(n - 1)])
    order = np.argsort(rows, kind="stable")
    h_ro = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=h_ro[1:])
    h_ci = cols[order].astype(np.int32)
    ro, ci = torch.from_numpy(h_ro).cuda(), torch.from_numpy(h_ci).cuda()
else:
    ro, ci = devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "rounds", 2: "device_loop"}
OPTIONS = ("schedule", "compact_below", "wave_min_row", "loop_max_list", "loop_max_entries")
p = ga.KcoreProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
times = {c: [] for c in configs}
stats, results, traces = {}, {}, {}
for rep in range(reps + 1):
    for c in configs:
        for name, value in zip(OPTIONS, c):
            assert p.set_option(name, value) == 0
        p.reset(); ms = p.enact()
        if rep:
            times[c].append(ms)
        else:
            stats[c] = p.stats()
            results[c] = p.extract()
            traces[c] = p.level_trace()
first = results[configs[0]]
for c in configs:
    assert results[c][1] == first[1] and results[c][0].tobytes() == first[0].tobytes(), "configurations disagree: %s" % (c,)
    t = sorted(times[c])
    st = stats[c]
    med = t[len(t) // 2]
    print("%s nodes %d entries %d | %s %s: enact ms median %.3f min %.3f | build ms %.3f | degeneracy %d | simple edges %d max degree %d | "
          "levels %d rounds %d launches %d compactions %d | entries read %d (%.2f G/s)" % (
              what, n, m, NAMES[int(c[0])], ":".join("%g" % x for x in c[1:]), med, t[0], st["build_ms"], first[1], st["simple_edges"],
              st["max_degree"], st["levels"], st["rounds"], st["kernel_launches"], st["compactions"], st["entries_read"],
              st["entries_read"] / med / 1e6))
if "--trace" in sys.argv:
    k, vertices, ms = traces[configs[0]]
    for i in np.argsort(-ms)[:10]:
        print("level %d: %d vertices, %.3f ms" % (k[i], vertices[i], ms[i]))
    print("levels %d, trace total %.3f ms" % (k.shape[0], ms.sum()))
p.close()
if "--cc" in sys.argv:
    q = ga.CcProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
    t = []
    for rep in range(reps + 1):
        q.reset(); ms = q.enact()
        if rep: t.append(ms)
    t.sort()
    print("%s CC enact ms median %.3f min %.3f" % (what, t[len(t) // 2], t[0]))
    q.close()
if "--tc" in sys.argv:
    q = ga.TcProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
    t = []
    for rep in range(reps + 1):
        q.reset(); ms = q.enact()
        if rep: t.append(ms)
    t.sort()
    print("%s TC enact ms median %.3f min %.3f" % (what, t[len(t) // 2], t[0]))
    q.close()
