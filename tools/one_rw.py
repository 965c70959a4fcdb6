"""Random-walk timing on a device-built graph, Reset once + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_rw.py <scale> [reps] [--lengths 8,16,40,80] [--modes uniform,weighted,biased] [--strategies 1,2] [--json FILE]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); one walk from every vertex of degree > 0.
weighted: the (row + col) % 7 + 1 weights, built on the device; biased: bias = (1, 4, 1).  Strategies: 0 auto / 1 lane / 2 tile.
One instrumented handle; the strategies are alternated rep by rep in one process, so they see the same device state, after one
warm-up round; the time is the kernel time of the handle's events (stats()["kernel_ms"]).  All strategies must give the same walks.
Prints steps per second for every cell; --json also writes them to a file."""
import sys, os, json
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
lengths = [int(x) for x in option("--lengths", "8,16,40,80").split(",")]
modes = option("--modes", "uniform,weighted,biased").split(",")
strategies = [int(x) for x in option("--strategies", "1,2").split(",")]
out_json = option("--json", "")
scale = int(args[0])
reps = int(args[1]) if len(args) > 1 else 5
NAMES = {0: "auto", 1: "lane", 2: "tile"}
ro, ci = devgraph.rmat_csr_device(scale, 8)
n, m = ro.shape[0] - 1, ci.shape[0]
deg = ro[1:] - ro[:-1]
rows = torch.repeat_interleave(torch.arange(n, device=ro.device, dtype=torch.int32), deg.to(torch.int64))
w = ((rows + ci) % 7 + 1).to(torch.int32)
starts = torch.nonzero(deg > 0).reshape(-1).to(torch.int32).cpu().numpy()
torch.cuda.synchronize()
p = ga.RwProblem(True).init_device(n, m, ro.data_ptr(), ci.data_ptr(), w.data_ptr())
print("rmat%d nodes %d entries %d walks %d | init ms %.3f" % (scale, n, m, starts.shape[0], p.stats()["build_ms"]), flush=True)
p.reset(starts)
cells = []
for mode in modes:
    p.set_option("weighted", int(mode == "weighted"))
    for name, b in zip(("bias_return", "bias_in", "bias_out"), (1, 4, 1) if mode == "biased" else (1, 1, 1)):
        p.set_option(name, b)
    for length in lengths:
        p.set_option("length", length)
        times = {s: [] for s in strategies}
        stats, lens = {}, {}
        for rep in range(reps + 1):
            for s in strategies:
                p.set_option("strategy", s)
                p.enact()
                st = p.stats()
                if rep:
                    times[s].append(st["kernel_ms"])
                else:
                    stats[s] = st
                    lens[s] = p.extract(walks=length <= 16)[:2]
        for s in strategies:
            assert lens[s][1].tobytes() == lens[strategies[0]][1].tobytes() and stats[s]["steps"] == stats[strategies[0]]["steps"], "strategies disagree"
            assert lens[s][0] is None or lens[s][0].tobytes() == lens[strategies[0]][0].tobytes(), "strategies disagree on the walks"
            t = sorted(times[s])
            med = t[len(t) // 2]
            cell = {"scale": scale, "mode": mode, "length": length, "strategy": NAMES[s], "ms_median": med, "ms_min": t[0], "ms_max": t[-1],
                    "steps": stats[s]["steps"], "gsteps_per_s": stats[s]["steps"] / med / 1e6, "biased_tries": stats[s]["biased_tries"],
                    "forced_fallbacks": stats[s]["forced_fallbacks"], "ended_early": stats[s]["ended_early"]}
            cells.append(cell)
            print("rmat%d %-8s length %3d %s: kernel ms median %.3f min %.3f max %.3f | steps %d (%.3f G/s) | tries %d forced %d ended %d" % (
                scale, mode, length, NAMES[s], med, t[0], t[-1], cell["steps"], cell["gsteps_per_s"], cell["biased_tries"], cell["forced_fallbacks"],
                cell["ended_early"]), flush=True)
p.close()
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(cells, f, indent=1)
