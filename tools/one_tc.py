"""Triangle counting timing on a device-built graph, Reset + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_tc.py <scale | gridSIDE> [reps] [--configs "s:lds:lane,..."] [--cc]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid4096): the road-like
SIDE x SIDE grid (devgraph.grid_csr_device).  --configs: strategy:lds_entries:lane_max_row triples (default "0:4096:32", the
library's defaults); the configurations are alternated rep by rep in one process, so they see the same device state.
--cc also times CC on the same graph, for scale."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
spec = sys.argv[sys.argv.index("--configs") + 1] if "--configs" in sys.argv else "0:4096:32"
configs = [tuple(int(x) for x in c.split(":")) for c in spec.split(",")]
ro, ci = devgraph.grid_csr_device(int(what[4:])) if what.startswith("grid") else devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "lane", 2: "lds", 3: "global"}
p = ga.TcProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
times = {c: [] for c in configs}
stats = {}
results = {}
for rep in range(reps + 1):
    for c in configs:
        p.set_option("strategy", c[0]); p.set_option("lds_entries", c[1]); p.set_option("lane_max_row", c[2])
        p.reset(); ms = p.enact()
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
    print("%s nodes %d entries %d | %s lds_entries %d lane_max_row %d: enact ms median %.3f min %.3f | build ms %.3f | triangles %d | "
          "oriented edges %d largest out-row %d | rows lane %d lds %d global %d | entries probed %d (%.2f G/s) launches %d" % (
              what, n, m, NAMES[c[0]], c[1], c[2], med, t[0], st["build_ms"], first[1], st["oriented_edges"], st["max_out_row"],
              st["lane_rows"], st["lds_rows"], st["global_rows"], st["entries_probed"], st["entries_probed"] / med / 1e6,
              st["kernel_launches"]))
_, transitivity = p.clustering(coefficients=False)
print("transitivity %.6f" % transitivity)
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
