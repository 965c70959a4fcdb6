"""MS-BFS against k separate direction-optimizing searches on the same handle-resident graph:
python tools/one_msbfs.py <scale | file.mtx> [k] [reps] [--directed] [--alpha A] [--beta B]

<scale>: device-built R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device), undirected unless --directed; a .mtx file
is read undirected unless --directed.  k sources (default 64) with a non-empty row from devgraph.seeded_sources.  Three things are
timed with a host clock around Reset + Enact (each ends in a device synchronise), alternated rep by rep in one process after one
warm-up round, and reported as median / min / max of `reps` (default 7):
  msbfs          one MsbfsProblem run over all k sources, depths not stored
  msbfs+depths   the same with the k * nodes depths stored (Reset fills them with -1)
  k x bfs        k BfsProblem searches one after another (reset + enact, traversal_mode 2; top-down when --directed)
Rows of the stored depths are compared with the single-source labels first.  The level trace printed is the one of an instrumented
handle (HIP events around every level, which adds a wait per level: its times are not the timed runs')."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

argv = sys.argv[1:]
tuning = {}
for name in ("alpha", "beta"):
    if "--" + name in argv:
        at = argv.index("--" + name)
        tuning[name] = float(argv[at + 1])
        del argv[at:at + 2]
directed = "--directed" in argv
args = [a for a in argv if not a.startswith("--")]
what = args[0]
k = int(args[1]) if len(args) > 1 else 64
reps = int(args[2]) if len(args) > 2 else 7
if what.endswith(".mtx"):
    from oracle import gr_oracle as o
    g = o.build_market(what, undirected=not directed)
    ro, ci = torch.from_numpy(g.row_offsets).cuda(), torch.from_numpy(g.col_indices).cuda()
else:
    ro, ci = devgraph.rmat_csr_device(int(what), 8, undirected=not directed)
n, m = ro.shape[0] - 1, ci.shape[0]
sources = np.array(devgraph.seeded_sources(ro.cpu(), k), dtype=np.int32)
torch.cuda.synchronize()

p = ga.MsbfsProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr())
for name, value in tuning.items():
    assert p.set_option(name, value) == 0
single = ga.BfsProblem().init_device(n, m, ro.data_ptr(), ci.data_ptr())
mode = 0 if directed else 2
if not directed:
    single.set_inverse_graph()


def msbfs(store):
    t = time.perf_counter()
    p.reset(sources, store_depths=store)
    ms = p.enact()
    return (time.perf_counter() - t) * 1e3, ms


def searches():
    t = time.perf_counter()
    ms = 0.0
    for s in sources.tolist():
        single.reset(s)
        ms += single.enact(s, traversal_mode=mode)
    return (time.perf_counter() - t) * 1e3, ms


# parity first: rows of the stored depths against the single-source labels
msbfs(True)
d_depth = p.device_results()[0]
for row in range(0, k, max(k // 8, 1)):
    s = int(sources[row])
    single.reset(s)
    single.enact(s, traversal_mode=mode)
    labels = devgraph.as_tensor(single.device_results()[0], n, "<i4")
    assert torch.equal(devgraph.as_tensor(d_depth + 4 * row * n, n, "<i4"), labels), "row %d differs from the search from %d" % (row, s)
reached, dist_sum, ecc = p.source_summary()
st = p.stats()
runs = {"msbfs": lambda: msbfs(False), "msbfs+depths": lambda: msbfs(True), "%d x bfs" % k: searches}
times = {name: [] for name in runs}
for rep in range(reps + 1):
    for name, run in runs.items():
        wall, device = run()
        if rep:
            times[name].append((wall, device))
print("%s nodes %d entries %d sources %d | batches %d levels %d push %d pull %d launches %d entries read %d (%.2f per entry of the graph) build ms %.3f | "
      "reached min %d max %d, largest eccentricity %d" % (what, n, m, k, st["batches"], st["levels"], st["push_levels"], st["pull_levels"], st["kernel_launches"],
                                                         st["entries_read"], st["entries_read"] / max(m, 1), st["build_ms"], reached.min(), reached.max(), ecc.max()))
for name in runs:
    wall = sorted(t[0] for t in times[name])
    device = sorted(t[1] for t in times[name])
    print("%-14s reset + enact wall ms median %.3f min %.3f max %.3f | enact device ms median %.3f min %.3f max %.3f" % (
        name, wall[len(wall) // 2], wall[0], wall[-1], device[len(device) // 2], device[0], device[-1]))
p.close()
single.close()

q = ga.MsbfsProblem(True).init_device(n, m, ro.data_ptr(), ci.data_ptr())
for name, value in tuning.items():
    assert q.set_option(name, value) == 0
for _ in range(2):
    q.reset(sources, store_depths=False)
    q.enact()
batch, level, kind, frontier, edges, ms = q.level_trace()
for i in range(batch.shape[0]):
    print("batch %d level %d %s: frontier %d vertices %d entries, %.3f ms" % (batch[i], level[i], ("push", "pull")[kind[i]], frontier[i], edges[i], ms[i]))
print("instrumented: levels %.3f ms, of which push %.3f pull %.3f" % (ms.sum(), ms[kind == 0].sum(), ms[kind == 1].sum()))
q.close()
