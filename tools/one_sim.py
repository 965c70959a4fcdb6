"""Vertex-similarity timing on a device-built graph, Reset + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_sim.py <scale> [reps] [--k K] [--pair-configs "strategy[:lane_max],..."] [--topk-configs "strategy:skip[:scratch_mib],..."]
                        [--max-wedges N] [--no-truss]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device).  Pair mode scores the M canonical pairs of the
graph, taken on the device from a truss handle of the same graph; next to it the time of grx_truss's support pass on that graph (a
fresh handle per rep: the pass runs in Init) -- the same intersections, the yardstick.  Top-k mode takes every vertex as a source.
One handle, the configurations alternated rep by rep in one process, so they see the same device state; every run must give the arrays
of the first one (compared on the device) and pair mode's `common` must be the truss handle's support."""
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
kk = int(option("--k", "16"))
pair_configs = [tuple(int(x) for x in (c.split(":") + ["64"])[:2]) for c in option("--pair-configs", "0,2").split(",")]
topk_configs = [tuple(int(x) for x in (c.split(":") + ["1024"])[:3]) for c in option("--topk-configs", "0:0,0:1").split(",")]
max_wedges = int(option("--max-wedges", "0"))
scale = int(args[0])
reps = int(args[1]) if len(args) > 1 else 5
ro, ci = devgraph.rmat_csr_device(scale, 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "lane", 2: "wave", 3: "block", 4: "global"}


def median(t):
    t = sorted(t)
    return t[len(t) // 2], t[0]


p = ga.SimProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
st = p.stats()
print("rmat%d nodes %d entries %d | init ms %.3f | edges %d wedges %d" % (scale, n, m, st["build_ms"], st["simple_edges"], st["wedges"]), flush=True)
M = st["simple_edges"]

# ---- pair mode on the canonical pairs, next to truss's support pass ----
if "--no-truss" not in sys.argv:
    t = ga.TrussProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
    _, d_support, d_src, d_dst = t.device_results()
    support = devgraph.as_tensor(d_support, M, "<i4")
    times, support_ms, first = {c: [] for c in pair_configs}, [], {}
    for rep in range(reps + 1):
        other = ga.TrussProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
        if rep:
            support_ms.append(other.stats()["support_ms"])
        other.close()
        for c in pair_configs:
            p.set_option("metric", ga.SIM_JACCARD); p.set_option("strategy", c[0]); p.set_option("lane_max", c[1])
            p.reset(); ms = p.pairs_device(M, d_src, d_dst)
            d = p.device_results()
            got = [devgraph.as_tensor(d[name], M, ts) for name, ts in (("pair_common", "<i4"), ("pair_num", "<i8"), ("pair_den", "<i8"))]
            assert torch.equal(got[0], support), "common differs from the truss handle's support: %s" % (c,)
            if "arrays" not in first:
                first["arrays"] = [x.clone() for x in got]
            assert all(torch.equal(x, y) for x, y in zip(got, first["arrays"])), "configurations disagree: %s" % (c,)
            if rep:
                times[c].append(ms)
            else:
                first[c] = p.stats()
    truss_med, truss_min = median(support_ms)
    print("rmat%d | truss support pass: ms median %.3f min %.3f | %d pairs" % (scale, truss_med, truss_min, M))
    for c in pair_configs:
        med, low = median(times[c])
        print("rmat%d | pairs %s lane_max %d: enact ms median %.3f min %.3f | %.3f G pairs/s | lane %d wave %d | x %.2f of the support pass" % (
            scale, NAMES[c[0]], c[1], med, low, M / med / 1e6, first[c]["lane_pairs"], first[c]["wave_pairs"], med / truss_med))
    t.close()

# ---- top-k of every vertex ----
if max_wedges and st["wedges"] > max_wedges:
    print("rmat%d: more than %d wedges, top-k not enacted" % (scale, max_wedges))
    p.close()
    sys.exit(0)
sources = torch.arange(n, dtype=torch.int32, device="cuda")
NAMES_TOPK = (("ids", "<i4"), ("common", "<i4"), ("num", "<i8"), ("den", "<i8"))
times, first, stats = {c: [] for c in topk_configs}, {}, {}
for rep in range(reps + 1):
    for c in topk_configs:
        p.set_option("metric", ga.SIM_JACCARD); p.set_option("strategy", c[0]); p.set_option("skip_neighbors", c[1]); p.set_option("scratch_mib", c[2])
        p.reset(); ms = p.topk_device(n, sources.data_ptr(), kk)
        d = p.device_results()
        got = [devgraph.as_tensor(d[name], n * kk, ts) for name, ts in NAMES_TOPK] + [devgraph.as_tensor(d[name], n, "<i4") for name in ("count", "candidates")]
        if c[1] not in first:
            first[c[1]] = [x.clone() for x in got]
        assert all(torch.equal(x, y) for x, y in zip(got, first[c[1]])), "configurations disagree: %s" % (c,)
        if rep:
            times[c].append(ms)
        else:
            stats[c] = p.stats()
for c in topk_configs:
    med, low = median(times[c])
    s = stats[c]
    shares = " ".join("%s %d (%.1f%%) / %d (%.1f%%)" % (r, s[r + "_sources"], 100.0 * s[r + "_sources"] / n, s[r + "_wedges"],
                                                        100.0 * s[r + "_wedges"] / max(s["wedges_walked"], 1)) for r in ("wave", "block", "global"))
    print("rmat%d | top-%d %s skip_neighbors %d scratch_mib %d: enact ms median %.3f min %.3f | wedges %d (%.3f G/s) | candidates %d | "
          "sources / wedges: %s | table probes %d launches %d" % (scale, kk, NAMES[c[0]], c[1], c[2], med, low, s["wedges_walked"],
                                                                  s["wedges_walked"] / med / 1e6, s["candidates"], shares, s["table_probes"],
                                                                  s["kernel_launches"]))
p.close()
