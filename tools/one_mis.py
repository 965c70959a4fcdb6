"""Maximal independent set / greedy colouring timing on a device-built graph, Reset + Enact, median of `reps`; also usable under
rocprofv3 --kernel-trace: python tools/one_mis.py <scale | gridSIDE> [reps] [--mode N] [--seed S] [--no-tail] [--trace]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid4096): the road-like
SIDE x SIDE grid (devgraph.grid_csr_device).  Without --mode all three run: 0 set, 1 colouring by rounds, 2 first-fit.
--no-tail keeps one launch per round instead of the device-side tail loop (grx_mis_set_tail)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
seed = option("--seed", 0)
modes = [option("--mode", 0)] if "--mode" in sys.argv else [0, 1, 2]
ro, ci = devgraph.grid_csr_device(int(what[4:])) if what.startswith("grid") else devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "set", 1: "color_rounds", 2: "color_first_fit"}
p = ga.MisProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr(), None, seed).set_tail("--no-tail" not in sys.argv)
for mode in modes:
    times = []
    for rep in range(reps + 1):
        p.reset(); ms = p.enact(mode)
        if rep: times.append(ms)
    _, summary = p.extract(ids=False)
    st = p.stats()
    times.sort()
    print("%s%s nodes %d entries %d mode %s seed %d: enact ms median %.3f min %.3f | %s %d | rounds %d tail sweeps %d "
          "entries read %d (%.3f x CSR) polls %d launches %d" % (
              what, " no-tail" if "--no-tail" in sys.argv else "", n, m, NAMES[mode], seed, times[len(times) // 2], times[0], "set size" if mode == 0 else "colours", summary,
              st["rounds"], st["tail_sweeps"], st["entries_read"], st["entries_read"] / max(m, 1), st["polls"], st["kernel_launches"]))
p.close()
if "--trace" in sys.argv:  # per host-visible round: undecided vertices it started with and its time (events around every round)
    p = ga.MisProblem(True).init_device(n, m, ro.data_ptr(), ci.data_ptr(), None, seed).set_tail("--no-tail" not in sys.argv)
    for mode in modes:
        p.reset(); p.enact(mode)
        for i, r in enumerate(p.round_trace()):
            print("%s round %d vertices %d ms %.3f" % (NAMES[mode], i + 1, r["vertices"], r["ms"]))
        print("instrumented", NAMES[mode], p.stats())
    p.close()
