"""Label-propagation timing on a device-built graph, Reset + Enact, median and minimum of `reps`; also usable under rocprofv3
--kernel-trace:  python tools/one_lp.py <scale | gridSIDE> [reps] [--configs "s:lane:wave:slots,..."] [--max-rounds N] [--check]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid4096): the road-like
SIDE x SIDE grid (devgraph.grid_csr_device).  NULL weights, both modes; the classes are gunrock's first-fit colouring, taken and timed
on the device (the cost LP_CLASSES adds).  --configs: strategy:lane_max_row:wave_max_row:table_slots, strategy 0 auto / 1 lane /
2 wave / 3 block; the default is the library's defaults alone.  One handle, the configurations and the modes alternated rep by rep in
one process, so they see the same device state; all configurations of a mode must give the same labels and counters.  --check also
runs the numpy form of tests/_lp_checker.py on the host, compares and prints its time."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph


def flag(name, default=None):
    if name not in sys.argv:
        return default
    value = sys.argv[sys.argv.index(name) + 1]
    args.remove(value)
    return value


args = [a for a in sys.argv[1:] if not a.startswith("--")]
spec = flag("--configs", "0:16:512:1024")
max_rounds = int(flag("--max-rounds", "0"))
what = args[0]
reps = int(args[1]) if len(args) > 1 else 5
configs = [tuple(int(x) for x in c.split(":")) for c in spec.split(",")]
ro, ci = devgraph.grid_csr_device(int(what[4:])) if what.startswith("grid") else devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "lane", 2: "wave", 3: "block"}
MODES = {ga.LP_SYNC: "sync", ga.LP_CLASSES: "classes"}
STATES = {ga.LP_CONVERGED: "converged", ga.LP_PERIOD2: "period-2", ga.LP_CAPPED: "capped"}

# the classes: first-fit colouring on the device, timed like everything else
mis = ga.MisProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr(), None, 0)
colour_ms = []
for rep in range(reps + 1):
    mis.reset(); ms = mis.enact(ga.MIS_COLOR_FIRST_FIT)
    if rep: colour_ms.append(ms)
colours, ncolours = mis.extract()
mis.close()
colour_ms.sort()
print("%s nodes %d entries %d | first-fit colouring: %d colours, enact ms median %.3f min %.3f" % (what, n, m, ncolours, colour_ms[len(colour_ms) // 2], colour_ms[0]))

p = ga.LpProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr(), None)
assert p.set_classes(colours.astype(np.int32) - 1) == 0
p.set_option("max_rounds", max_rounds)
runs = [(mode, c) for mode in (ga.LP_SYNC, ga.LP_CLASSES) for c in configs]
times = {r: [] for r in runs}
stats, results = {}, {}
for rep in range(reps + 1):
    for mode, c in runs:
        p.set_option("mode", mode); p.set_option("strategy", c[0]); p.set_option("lane_max_row", c[1])
        p.set_option("wave_max_row", c[2]); p.set_option("table_slots", c[3])
        p.reset(); ms = p.enact()
        if rep:
            times[(mode, c)].append(ms)
        else:
            stats[(mode, c)] = p.stats()
            results[(mode, c)] = p.extract()
for mode, c in runs:
    first, st = results[(mode, configs[0])], stats[(mode, c)]
    got = results[(mode, c)]
    assert got[0].tobytes() == first[0].tobytes() and got[2] == first[2], "configurations disagree: %s" % ((mode, c),)
    assert all(st[x] == stats[(mode, configs[0])][x] for x in ("rounds", "state", "visits", "entries_read")), "counters disagree: %s" % ((mode, c),)
    t = sorted(times[(mode, c)])
    med = t[len(t) // 2]
    ran = st["rounds"] + (st["state"] == ga.LP_CONVERGED)  # (the closing round changed nothing and is not in "rounds")
    print("%s %s | %s lane_max_row %d wave_max_row %d table_slots %d: enact ms median %.3f min %.3f | build ms %.3f | %s after %d rounds, "
          "%d communities | ms/round %.3f | entries_read %d (%.3f G/s) | visits %d = %.4f of n x rounds | rows lane %d wave %d block %d "
          "fallback %d | launches %d read-backs %d" % (
              what, MODES[mode], NAMES[c[0]], c[1], c[2], c[3], med, t[0], st["build_ms"], STATES[st["state"]], st["rounds"], got[2],
              med / max(ran, 1), st["entries_read"], st["entries_read"] / med / 1e6, st["visits"], st["visits"] / (n * max(ran, 1)),
              st["regime_rows"][0], st["regime_rows"][1], st["regime_rows"][2], st["fallback_rows"], st["kernel_launches"], st["readbacks"]))
if "--check" in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _lp_checker as k
    h_ro, h_ci = ro.cpu().numpy(), ci.cpu().numpy()
    a, b, pw = k.pairs_of(n, h_ro, h_ci)
    for mode in (ga.LP_SYNC, ga.LP_CLASSES):
        t0 = time.time()
        ref = k.run_numpy(n, a, b, pw, mode, colours.astype(np.int32) - 1, None, max_rounds if max_rounds else 2 * n + 64)
        seconds = time.time() - t0
        st = stats[(mode, configs[0])]
        same = np.array_equal(results[(mode, configs[0])][0], ref["labels"]) and all(st[x] == ref[x] for x in k.FIELDS)
        print("%s %s | numpy checker %.3f s, %s" % (what, MODES[mode], seconds, "identical" if same else "DIFFERENT"))
        assert same
p.close()
