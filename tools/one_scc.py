"""SCC timing on a device-built directed graph, Reset + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_scc.py <scale | gridSIDE | cycleN> [reps] [--configs "schedule:pivot_phase:trim[:pair_trim:wave_min_row:loop_max_list:loop_max_entries],..."] [--cc] [--trace]

<scale>: directed R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device, undirected=False); gridSIDE (e.g.
grid4096): the SIDE x SIDE 4-neighbour grid with each edge given one random direction; cycleN (e.g. cycle1048576): a directed
cycle of N vertices.  --configs: default "0:1:1,1:1:1,2:1:1,1:0:1" (the library's defaults, the plain form, the device loop
everywhere, the plain form without the pivot phase); the configurations are alternated rep by rep in one process, so they see the
same device state.  --cc also times CC on the same CSR, for scale; --trace prints the phases of the first configuration."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
spec = sys.argv[sys.argv.index("--configs") + 1] if "--configs" in sys.argv else "0:1:1,1:1:1,2:1:1,1:0:1"
DEFAULTS = (0, 1, 1, 1, 16, 32768, 8192)  # the library's; a configuration that names fewer values takes the rest from here
configs = [tuple(float(x) for x in c.split(":")) for c in spec.split(",")]
configs = [c + DEFAULTS[len(c):] for c in configs]
if what.startswith("grid"):
    side = int(what[4:])
    n = side * side
    v = torch.arange(n, device="cuda", dtype=torch.int64)
    right, down = v[v % side < side - 1], v[v // side < side - 1]
    rows, cols = torch.cat([right, down]), torch.cat([right + 1, down + side])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x6772)
    flip = torch.rand(rows.shape[0], generator=gen, device="cuda") < 0.5
    ro, ci = devgraph.csr_from_tuples_device(n, torch.where(flip, cols, rows).int(), torch.where(flip, rows, cols).int(), undirected=False)
elif what.startswith("cycle"):
    n = int(what[5:])
    ro = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    ci = ((torch.arange(n, dtype=torch.int64, device="cuda") + 1) % n).int()
else:
    ro, ci = devgraph.rmat_csr_device(int(what), 8, undirected=False)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "rounds", 2: "device_loop"}
OPTIONS = ("schedule", "pivot_phase", "trim", "pair_trim", "wave_min_row", "loop_max_list", "loop_max_entries")
p = ga.SccProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
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
            traces[c] = p.phase_trace()
first = results[configs[0]]
summary = p.summary()
for c in configs:
    assert results[c][1] == first[1] and results[c][0].tobytes() == first[0].tobytes(), "configurations disagree: %s" % (c,)
    t = sorted(times[c])
    st = stats[c]
    med = t[len(t) // 2]
    print("%s nodes %d entries %d | %s pivot %d trim %d pairs %d %s: enact ms median %.3f min %.3f | build ms %.3f | components %d largest %d trivial %d | "
          "trimmed %d in %d sub-rounds, pivot component %d, colour rounds %d sweeps %d, search levels %d, launches %d | entries read %d (%.2f G/s)" % (
              what, n, m, NAMES[int(c[0])], c[1], c[2], c[3], ":".join("%g" % x for x in c[4:]), med, t[0], st["build_ms"], summary["components"],
              summary["largest"], summary["trivial"], st["trimmed"], st["trim_rounds"], st["pivot_component"], st["colour_rounds"], st["sweeps"],
              st["bfs_levels"], st["kernel_launches"], st["entries_read"], st["entries_read"] / max(med, 1e-9) / 1e6))
if "--trace" in sys.argv:
    kind, vertices, ms = traces[configs[0]]
    for i in np.argsort(-ms)[:10]:
        print("phase %d (%s): %d vertices, %.3f ms" % (i, ("trim", "pivot", "colour")[kind[i]], vertices[i], ms[i]))
    print("phases %d, trace total %.3f ms" % (kind.shape[0], ms.sum()))
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
