"""BCC timing on a device-built undirected graph, Reset + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_bcc.py <scale | gridSIDE | pathN> [reps] [--configs "schedule[:wave_min_row:loop_max_list:loop_max_entries],..."] [--cc] [--kcore] [--trace]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid4096): the plain SIDE x
SIDE 4-neighbour grid; pathN (e.g. path1048576): a path of N vertices.  --configs: default "0,1" (the library's defaults and the
plain form; "2", the device loop everywhere, is one workgroup for the whole graph); the configurations are alternated rep by rep in
one process, so they see the same device state.  Every repetition is timed twice: the HIP-event time of Enact, and the host's clock
around Reset + Enact.  --cc / --kcore also time the CC Enact and report the k-core build on the same CSR, the yardsticks of DESIGN.md
3.15; --trace prints the phases of the first configuration."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 3
spec = sys.argv[sys.argv.index("--configs") + 1] if "--configs" in sys.argv else "0,1"
DEFAULTS = (0, 16, 32768, 8192)  # the library's; a configuration that names fewer values takes the rest from here
configs = [tuple(float(x) for x in c.split(":")) for c in spec.split(",")]
configs = [c + DEFAULTS[len(c):] for c in configs]
if what.startswith("grid"):
    side = int(what[4:])
    n = side * side
    v = torch.arange(n, device="cuda", dtype=torch.int64)
    right, down = v[v % side < side - 1], v[v // side < side - 1]
    ro, ci = devgraph.csr_from_tuples_device(n, torch.cat([right, down]).int(), torch.cat([right + 1, down + side]).int(), undirected=True)
elif what.startswith("path"):
    n = int(what[4:])
    v = torch.arange(n - 1, device="cuda", dtype=torch.int32)
    ro, ci = devgraph.csr_from_tuples_device(n, v, v + 1, undirected=True)
else:
    ro, ci = devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "rounds", 2: "device_loop"}
OPTIONS = ("schedule", "wave_min_row", "loop_max_list", "loop_max_entries")
p = ga.BccProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
times = {c: [] for c in configs}
walls = {c: [] for c in configs}
stats, results, traces = {}, {}, {}
for rep in range(reps + 1):
    for c in configs:
        for name, value in zip(OPTIONS, c):
            assert p.set_option(name, value) == 0
        t0 = time.perf_counter()
        p.reset(); ms = p.enact()
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
    assert all(results[c][key].tobytes() == first[key].tobytes() for key in first), "configurations disagree: %s" % (c,)
    t, w = sorted(times[c]), sorted(walls[c])
    st = stats[c]
    med = t[len(t) // 2]
    print("%s nodes %d entries %d | %s %s: enact ms median %.3f min %.3f | reset + enact (host clock) ms median %.3f | build ms %.3f | simple edges %d | "
          "blocks %d bridges %d articulation points %d largest block %d | 2-edge-connected components %d largest %d | trees %d levels %d launches %d "
          "read-backs %d | entries read %d = %.2f M (%.2f G/s)" % (
              what, n, m, NAMES[int(c[0])], ":".join("%g" % x for x in c[1:]), med, t[0], w[len(w) // 2], st["build_ms"], st["simple_edges"],
              summary["blocks"], summary["bridges"], summary["articulation_points"], summary["largest_block"], summary["tecc_components"],
              summary["largest_tecc"], st["trees"], st["levels"], st["kernel_launches"], st["readbacks"], st["entries_read"],
              st["entries_read"] / max(st["simple_edges"], 1), st["entries_read"] / max(med, 1e-9) / 1e6))
if "--trace" in sys.argv:
    kind, items, ms = traces[configs[0]]
    for i in range(kind.shape[0]):
        print("phase %s: %d items, %.3f ms" % (("forest", "sizes", "numbering", "low/high", "link", "label")[kind[i]], items[i], ms[i]))
    print("trace total %.3f ms" % ms.sum())
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
if "--kcore" in sys.argv:
    q = ga.KcoreProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
    print("%s k-core build ms %.3f" % (what, q.stats()["build_ms"]))
    q.close()
