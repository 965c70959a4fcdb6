"""Neighbourhood-sampling timing on a device-built graph, Reset once + Enact, median of `reps`; also usable under rocprofv3 --kernel-trace:
python tools/one_sample.py <scale> [reps] [--seeds 1024,65536] [--fanouts 15,10,5/25,10] [--replace 0,1] [--strategies 1,2] [--gather 66] [--json FILE]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); the seeds are a seeded choice among the
vertices of degree > 0.  Strategies: 0 auto / 1 lane / 2 group.  One instrumented handle; the strategies are alternated rep by rep in
one process, so they see the same device state, after one warm-up round; the times are the kernel times of the handle's events
(stats(): count + scan, sample, renumber, relabel and their sum).  All strategies must give the same arrays.  Prints V, E, the sampled
edges per second over the whole kernel time, and the sample kernel's own rate as a fraction of `--gather` (default 66 G/s, the
random-gather rate DESIGN.md 8 quotes; a yardstick, not a target); --json also writes the cells to a file."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
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
seed_counts = [int(x) for x in option("--seeds", "1024,65536").split(",")]
fanout_lists = [tuple(int(x) for x in part.split(",")) for part in option("--fanouts", "15,10,5/25,10").split("/")]
replaces = [int(x) for x in option("--replace", "0,1").split(",")]
strategies = [int(x) for x in option("--strategies", "1,2").split(",")]
gather = float(option("--gather", "66"))
out_json = option("--json", "")
scale = int(args[0])
reps = int(args[1]) if len(args) > 1 else 7
NAMES = {0: "auto", 1: "lane", 2: "group"}
PHASES = ("count_ms", "sample_ms", "renumber_ms", "relabel_ms")
ro, ci = devgraph.rmat_csr_device(scale, 8)
n, m = ro.shape[0] - 1, ci.shape[0]
candidates = torch.nonzero((ro[1:] - ro[:-1]) > 0).reshape(-1).to(torch.int32).cpu().numpy()
torch.cuda.synchronize()
p = ga.SampleProblem(True).init_device(n, m, ro.data_ptr(), ci.data_ptr())
print("rmat%d nodes %d entries %d | init ms %.3f" % (scale, n, m, p.stats()["build_ms"]), flush=True)
cells = []
for count in seed_counts:
    seeds = np.random.default_rng(count).permutation(candidates)[:count]
    p.reset(seeds)
    for fanouts in fanout_lists:
        p.set_fanouts(fanouts)
        for replace in replaces:
            p.set_option("replace", replace)
            times = {s: {name: [] for name in PHASES + ("kernel_ms",)} for s in strategies}
            results = {}
            for rep in range(reps + 1):
                for s in strategies:
                    p.set_option("strategy", s)
                    p.enact()
                    st = p.stats()
                    if rep:
                        for name in times[s]:
                            times[s][name].append(st[name])
                    else:
                        results[s] = p.extract()
            for s in strategies:
                assert all(results[s][key].tobytes() == results[strategies[0]][key].tobytes() for key in results[s]), "strategies disagree"
                med = {name: sorted(t)[len(t) // 2] for name, t in times[s].items()}
                total = sorted(times[s]["kernel_ms"])
                v, e = int(results[s]["vertices"].shape[0]), int(results[s]["cols"].shape[0])
                cell = {"scale": scale, "seeds": int(seeds.shape[0]), "fanouts": list(fanouts), "replace": replace, "strategy": NAMES[s], "vertices": v,
                        "edges": e, "ms_median": med["kernel_ms"], "ms_min": total[0], "ms_max": total[-1], "gedges_per_s": e / med["kernel_ms"] / 1e6,
                        "sample_gedges_per_s": e / med["sample_ms"] / 1e6, "sample_of_gather": e / med["sample_ms"] / 1e6 / gather}
                cell.update({name: med[name] for name in PHASES})
                cells.append(cell)
                print("rmat%d seeds %6d fanouts %-10s replace %d %-5s: kernel ms median %.3f min %.3f max %.3f = count %.3f + sample %.3f + renumber %.3f "
                      "+ relabel %.3f | V %d E %d (%.3f G edges/s) | sample kernel %.2f G/s = %.3f of the gather rate" % (
                          scale, seeds.shape[0], ",".join(str(f) for f in fanouts), replace, NAMES[s], med["kernel_ms"], total[0], total[-1], med["count_ms"],
                          med["sample_ms"], med["renumber_ms"], med["relabel_ms"], v, e, cell["gedges_per_s"], cell["sample_gedges_per_s"],
                          cell["sample_of_gather"]), flush=True)
p.close()
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as f:
        json.dump(cells, f, indent=1)
