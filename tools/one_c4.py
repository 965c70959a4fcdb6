"""4-cycle (butterfly) counting timing on a device-built graph, Reset + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_c4.py <scale | gridSIDE> [reps] [--configs "strategy:edges[:scratch_mib],..."] [--tc] [--max-wedges N]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid4096): the road-like
SIDE x SIDE grid (devgraph.grid_csr_device).  --configs: strategy 0 auto / 1 lane / 2 wave / 3 block / 4 global, edges 0 or 1, and
optionally the scratch budget of the GLOBAL regime in MiB (default 1024); the default is AUTO without and with the per-edge counts.
One handle, the configurations alternated rep by rep in one process, so they see the same device state; all of them must give the same arrays.  The wedges are known after Init and printed at once; --max-wedges N ends
the run there when the graph has more.  --tc also times triangle counting on the same graph, for scale."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph


def option(name, default):
    if name not in sys.argv:
        return default
    value = sys.argv[sys.argv.index(name) + 1]
    args.remove(value)
    return value


args = [a for a in sys.argv[1:] if not a.startswith("--")]
spec = option("--configs", "0:0,0:1")
max_wedges = int(option("--max-wedges", "0"))
what = args[0]
reps = int(args[1]) if len(args) > 1 else 5
configs = [tuple(int(x) for x in (c.split(":") + ["1024"])[:3]) for c in spec.split(",")]
ro, ci = devgraph.grid_csr_device(int(what[4:])) if what.startswith("grid") else devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "lane", 2: "wave", 3: "block", 4: "global"}
REGIMES = ("lane", "wave", "block", "global")
p = ga.C4Problem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
st = p.stats()
print("%s nodes %d entries %d | init ms %.3f | edges %d wedges %d | bound %.6g = 2^62 * %.3g" % (
    what, n, m, st["build_ms"], st["simple_edges"], st["wedges"], st["bound"], st["bound"] / 2.0 ** 62), flush=True)
if max_wedges and st["wedges"] > max_wedges:
    print("%s: more than %d wedges, not enacted" % (what, max_wedges))
    p.close()
    sys.exit(0)
times = {c: [] for c in configs}
stats, results = {}, {}
for rep in range(reps + 1):
    for c in configs:
        p.set_option("strategy", c[0]); p.set_option("edges", c[1]); p.set_option("scratch_mib", c[2])
        p.reset(); ms = p.enact()
        if rep:
            times[c].append(ms)
        else:
            stats[c] = p.stats()
            results[c] = p.extract() + ((p.extract_edges(),) if c[1] else ())
first = results[configs[0]]
with_edges = [results[c][2] for c in configs if c[1]]
for c in configs:
    assert results[c][1] == first[1] and results[c][0].tobytes() == first[0].tobytes(), "configurations disagree: %s" % (c,)
    assert not c[1] or results[c][2].tobytes() == with_edges[0].tobytes(), "configurations disagree on the edges: %s" % (c,)
    t = sorted(times[c])
    st = stats[c]
    med = t[len(t) // 2]
    starts = sum(st[r + "_vertices"] for r in REGIMES)
    shares = " ".join("%s %d (%.1f%%) / %d (%.1f%%)" % (r, st[r + "_vertices"], 100.0 * st[r + "_vertices"] / max(starts, 1), st[r + "_wedges"],
                                                        100.0 * st[r + "_wedges"] / max(st["wedges"], 1)) for r in REGIMES)
    print("%s | %s edges %d scratch_mib %d: enact ms median %.3f min %.3f | 4-cycles %d | wedges %d (%.3f G/s) | start vertices / wedges: %s | "
          "table probes %d launches %d" % (what, NAMES[c[0]], c[1], c[2], med, t[0], first[1], st["wedges"], st["wedges"] / med / 1e6, shares,
                                           st["table_probes"], st["kernel_launches"]))
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
