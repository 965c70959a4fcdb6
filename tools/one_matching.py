"""Heavy-edge matching timing on a device-built graph, Reset + Enact, median of `reps` per schedule; also usable under rocprofv3
--kernel-trace:  python tools/one_matching.py <scale | grid:SIDE> [reps] [--configs "schedule[:wave_min_row],..."] [--weights] [--levels L] [--no-cpu] [--mis] [--trace]

The graph: an undirected R-MAT of 2^scale vertices and 8 * 2^scale generated pairs (devgraph.rmat_csr_device), or the SIDE x SIDE
grid; --weights gives every entry torch.randint(1, 8) under the seed `scale` (the two directions of a pair may differ: the larger
counts).  --configs: default "0,1,2" (AUTO, ROUNDS, DEVICE_LOOP); the configurations are alternated rep by rep in one process, so they
see the same device state.  Every repetition is timed twice: the HIP-event time of Enact, and the host's clock around Reset + Enact.
The contraction of the last result is timed by the host's clock.  --levels L chains L levels on the device the way gunrock_coarsen
does (each handle takes the coarse arrays of the one before through init_device) under the first configuration and prints each
level's sizes and times.  Unless --no-cpu is given, the checker's numpy rounds form is timed on the same
graph in the same run and its matching must be the GPU's.  --mis times the MIS set's Enact on the same graph as a frame of
reference.  --trace prints the host's steps of the first configuration."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
spec = sys.argv[sys.argv.index("--configs") + 1] if "--configs" in sys.argv else "0,1,2"
levels = int(sys.argv[sys.argv.index("--levels") + 1]) if "--levels" in sys.argv else 0
DEFAULTS = (0, 16)  # the library's; a configuration that names fewer values takes the rest from here
configs = [tuple(int(x) for x in c.split(":")) for c in spec.split(",")]
configs = [c + DEFAULTS[len(c):] for c in configs]
if what.startswith("grid:"):
    side = int(what[5:])
    n, seed = side * side, side
    v = torch.arange(n, dtype=torch.int64, device="cuda")
    right, down = v[(v % side) < side - 1], v[v < n - side]
    rows = torch.cat([right, right + 1, down, down + side])
    cols = torch.cat([right + 1, right, down + side, down])
    order = torch.argsort(rows * n + cols)
    ci = cols[order].to(torch.int32)
    ro = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ro[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    ro = ro.to(torch.int32)
    name = "grid%d" % side
else:
    seed = int(what)
    n = 1 << seed
    ro, ci = devgraph.rmat_csr_device(seed, 8)
    name = "rmat%d" % seed
m = int(ci.shape[0])
w = None
if "--weights" in sys.argv:
    torch.manual_seed(seed)
    w = torch.randint(1, 8, (m,), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "rounds", 2: "device_loop"}
OPTIONS = ("schedule", "wave_min_row")
p = ga.MatchingProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr(), w.data_ptr() if w is not None else None, seed=seed)
times = {c: [] for c in configs}
walls = {c: [] for c in configs}
stats, results, traces = {}, {}, {}
for rep in range(reps + 1):
    for c in configs:
        for key, value in zip(OPTIONS, c):
            assert p.set_option(key, value) == 0
        t0 = time.perf_counter()
        p.reset(); ms = p.enact()
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            times[c].append(ms)
            walls[c].append(wall)
        else:
            stats[c] = p.stats()
            results[c] = p.extract()
            traces[c] = p.round_trace()
first = results[configs[0]]
summary = p.summary()
for c in configs:
    assert all(results[c][key].tobytes() == first[key].tobytes() for key in ("in_matching", "mate", "medge")), "configurations disagree: %s" % (c,)
    t, wl = sorted(times[c]), sorted(walls[c])
    st = stats[c]
    med = t[len(t) // 2]
    print("%s nodes %d entries %d | %s wave_min_row %d: enact ms median %.3f min %.3f | reset + enact (host clock) ms median %.3f | build ms %.3f | "
          "pairs %d matched %d weight %d unmatched %d (%d with neighbours) | rounds %d (%d in the loop) launches %d | "
          "entries read %d = %.2f x 2M, polls %d (%.2f G entries/s)" % (
              name, n, m, NAMES[c[0]], c[1], med, t[0], wl[len(wl) // 2], st["build_ms"], st["pairs"], summary["matched"], summary["weight"],
              summary["unmatched"], summary["unmatched_with_neighbours"], st["rounds"], st["loop_rounds"], st["kernel_launches"], st["entries_read"],
              st["entries_read"] / max(2 * st["pairs"], 1), st["polls"], st["entries_read"] / max(med, 1e-9) / 1e6))
if "--trace" in sys.argv:
    kind, ran, live, matched = traces[configs[0]]
    for i in range(kind.shape[0]):
        print("step %d %s: %d rounds, list %d, matched %d" % (i, ("wide", "loop")[kind[i]], ran[i], live[i], matched[i]))
contract = []
for rep in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nc, ne = p.contract()
    contract.append((time.perf_counter() - t0) * 1e3)
contract.sort()
print("%s contract (host clock) ms median %.3f min %.3f | coarse nodes %d entries %d" % (name, contract[len(contract) // 2], contract[0], nc, ne))
a, b, pw = p.pairs()
if levels:
    for key, value in zip(OPTIONS, configs[0]):
        p.set_option(key, value)
    handles, q, d_vw = [p], p, None
    for level in range(levels):
        t0 = time.perf_counter()
        q.reset(); ms = q.enact()
        s = q.summary()
        nc, ne = q.contract(d_vw)
        wall = (time.perf_counter() - t0) * 1e3
        print("level %d: nodes %d pairs %d matched %d rounds %d | enact ms %.3f | reset + enact + contract (host clock) ms %.3f | coarse nodes %d entries %d" % (
            level, q.nodes, s["pairs"], s["matched"], q.stats()["rounds"], ms, wall, nc, ne))
        if s["matched"] == 0 or level + 1 == levels:
            break
        d = q.coarse_device()
        d_vw = d["vweight"]
        q = ga.MatchingProblem(False).init_device(nc, ne, d["row_offsets"], d["col_indices"], d["weights"] if ne else None, seed=seed)
        for key, value in zip(OPTIONS, configs[0]):
            q.set_option(key, value)
        handles.append(q)
    for h in reversed(handles[1:]):
        h.close()
p.close()
if "--mis" in sys.argv:
    q = ga.MisProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr(), seed=seed)
    t = []
    for rep in range(reps + 1):
        q.reset()
        t.append(q.enact(ga.MIS_SET))
    t = sorted(t[1:])
    print("%s MIS set enact ms median %.3f min %.3f" % (name, t[len(t) // 2], t[0]))
    q.close()
if "--no-cpu" not in sys.argv:
    import _matching_checker as k
    t0 = time.perf_counter()
    ref, count = k.rounds(n, a, b, pw, seed)
    cpu = (time.perf_counter() - t0) * 1e3
    assert all(np.array_equal(ref[key], first[key]) for key in ("in_matching", "mate", "medge")) and count == stats[configs[0]]["rounds"], \
        "the numpy rounds form disagrees"
    print("%s numpy rounds form on the CPU: %.1f ms, %d rounds, the same matching" % (name, cpu, count))
