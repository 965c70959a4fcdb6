"""k-truss timing on a device-built graph, Reset + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_truss.py <scale | gridSIDE> [reps] [--configs "schedule:wave_min_row[:loop_max_list:loop_max_entries],..."] [--tc] [--kcore] [--trace]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid4096): the road-like
SIDE x SIDE grid (devgraph.grid_csr_device).  --configs: default "0:32,1:32" (the library's defaults, the plain form); the
configurations are alternated rep by rep in one process, so they see the same device state.  --tc / --kcore also time TC and
k-core (Reset + Enact) on the same graph, the yardsticks of the support pass and of the peel; --trace prints the ten longest
levels of the first configuration."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
spec = sys.argv[sys.argv.index("--configs") + 1] if "--configs" in sys.argv else "0:32,1:32"
DEFAULTS = (0, 32, 32768, 8192)  # the library's; a configuration that names fewer values takes the rest from here
configs = [tuple(float(x) for x in c.split(":")) for c in spec.split(",")]
configs = [c + DEFAULTS[len(c):] for c in configs]
if what.startswith("grid"):
    ro, ci = devgraph.grid_csr_device(int(what[4:]))
else:
    ro, ci = devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "rounds"}
OPTIONS = ("schedule", "wave_min_row", "loop_max_list", "loop_max_entries")
p = ga.TrussProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
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
    print("%s nodes %d entries %d | %s %s: enact ms median %.3f min %.3f max %.3f | build ms %.3f support ms %.3f | max truss %d | "
          "simple edges %d triangles %d max support %d | levels %d rounds %d launches %d read-backs %d | entries: support %d peel %d "
          "(%.2f G/s)" % (
              what, n, m, NAMES[int(c[0])], ":".join("%g" % x for x in c[1:]), med, t[0], t[-1], st["build_ms"], st["support_ms"], first[1],
              st["simple_edges"], st["triangles"], st["max_support"], st["levels"], st["rounds"], st["kernel_launches"], st["readbacks"],
              st["support_entries"], st["peel_entries"], st["peel_entries"] / med / 1e6))
if "--trace" in sys.argv:
    k, edges, ms = traces[configs[0]]
    for i in np.argsort(-ms)[:10]:
        print("level %d: %d edges, %.3f ms" % (k[i], edges[i], ms[i]))
    print("levels %d, trace total %.3f ms" % (k.shape[0], ms.sum()))
p.close()
for flag, cls, label in (("--tc", ga.TcProblem, "TC"), ("--kcore", ga.KcoreProblem, "k-core")):
    if flag in sys.argv:
        q = cls(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
        t = []
        for rep in range(reps + 1):
            q.reset(); ms = q.enact()
            if rep: t.append(ms)
        t.sort()
        print("%s %s enact ms median %.3f min %.3f max %.3f" % (what, label, t[len(t) // 2], t[0], t[-1]))
        q.close()
