"""Colour-refinement timing on a device-built graph, Reset + Enact, median and minimum of `reps`; also usable under rocprofv3
--kernel-trace:  python tools/one_wl.py <scale | gridSIDE> [reps] [--configs "s:lane:wave,..."] [--max-rounds N] [--check] [--host]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 8 (devgraph.rmat_csr_device); gridSIDE (e.g. grid2048): the road-like
SIDE x SIDE grid (devgraph.grid_csr_device).  No labels.  --configs: strategy:lane_max_row:wave_max_row, strategy 0 auto / 1 lane /
2 wave / 3 block; the default is the library's defaults alone.  One instrumented handle, the configurations alternated rep by rep in
one process, so they see the same device state; all configurations must give the same colouring.  Printed per configuration: the
enact time, the summed kernel time, the time per signature pass, and the effective traffic of a pass -- 4 B per entry for the column,
4 B per entry for the gathered colour, and per vertex 8 B of offsets, 16 B of signature written and read, 20 B of the owner's key
compared, 8 B of table and 12 B of slot and colour -- as a fraction of 8 TB/s.  A checksum of the result (classes, rounds, CRC-32 of
the colouring) is printed for comparison across runs.  --check also runs tests/_wl_checker.py's rounds on the host, compares and
prints its time; --host runs only that, on the oracle's R-MAT (the same graph), without a GPU."""
import sys, os, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def flag(name, default=None):
    if name not in sys.argv:
        return default
    value = sys.argv[sys.argv.index(name) + 1]
    args.remove(value)
    return value


def checksum(colour, rounds):
    return "classes %d rounds %d crc %08x" % (int(colour.max()) + 1, rounds, zlib.crc32(np.ascontiguousarray(colour, np.int32).tobytes()))


def host_check(n, ro, ci, max_rounds):
    import _wl_checker as k
    t0 = time.time()
    ref = k.rounds(n, ro, ci, None, max_rounds)
    return ref, time.time() - t0


args = [a for a in sys.argv[1:] if not a.startswith("--")]
spec = flag("--configs", "0:16:4096")
max_rounds = int(flag("--max-rounds", "-1"))
what = args[0]
reps = int(args[1]) if len(args) > 1 else 5
if "--host" in sys.argv:
    from oracle import gr_oracle as o
    g = o.rmat_seeded(int(what), 8 << int(what))
    ref, seconds = host_check(g.nodes, g.row_offsets, g.col_indices, max_rounds)
    print("%s nodes %d entries %d | checker %.3f s | %s" % (what, g.nodes, g.edges, seconds, checksum(ref["colour"], ref["rounds"])))
    sys.exit(0)

import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

configs = [tuple(int(x) for x in c.split(":")) for c in spec.split(",")]
ro, ci = devgraph.grid_csr_device(int(what[4:])) if what.startswith("grid") else devgraph.rmat_csr_device(int(what), 8)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
NAMES = {0: "auto", 1: "lane", 2: "wave", 3: "block"}
STATES = {ga.WL_STABLE: "stable", ga.WL_CAPPED: "capped"}

p = ga.WlProblem(True).init_device(n, m, ro.data_ptr(), ci.data_ptr())
p.set_option("max_rounds", max_rounds)
times = {c: [] for c in configs}
kernel = {c: [] for c in configs}
stats, results = {}, {}
for rep in range(reps + 1):
    for c in configs:
        p.set_option("strategy", c[0]); p.set_option("lane_max_row", c[1]); p.set_option("wave_max_row", c[2])
        p.reset(); ms = p.enact()
        if rep:
            times[c].append(ms)
            kernel[c].append(p.stats()["kernel_ms"])
        else:
            stats[c] = p.stats()
            results[c] = p.extract()[0].copy()
print("%s nodes %d entries %d" % (what, n, m))
for c in configs:
    st = stats[c]
    assert results[c].tobytes() == results[configs[0]].tobytes(), "configurations disagree: %s" % (c,)
    t, kt = sorted(times[c]), sorted(kernel[c])
    med, kmed = t[len(t) // 2], kt[len(kt) // 2]
    passes = st["readbacks"] - 1
    per_pass = kmed / max(passes, 1)
    bytes_pass = 8.0 * m + (8 + 16 + 16 + 20 + 8 + 12) * n
    print("%s | %s lane_max_row %d wave_max_row %d: enact ms median %.3f min %.3f | kernel ms median %.3f | %s after %d rounds, %d classes, "
          "%d passes, %d certificates, %d repairs | kernel ms/pass %.4f | %.1f MB/pass = %.3f TB/s = %.3f of 8 TB/s | %.2f G entries/s | "
          "rows lane %d wave %d block %d | compared wave %d block %d global %d | launches %d read-backs %d | %s" % (
              what, NAMES[c[0]], c[1], c[2], med, t[0], kmed, STATES[st["state"]], st["rounds"], st["classes"], passes, st["certificate_runs"],
              st["repairs"], per_pass, bytes_pass / 1e6, bytes_pass / per_pass / 1e9, bytes_pass / per_pass / 1e9 / 8.0, m / per_pass / 1e6,
              st["regime_rows"][0], st["regime_rows"][1], st["regime_rows"][2], st["rung_rows"][0], st["rung_rows"][1], st["rung_rows"][2],
              st["kernel_launches"], st["readbacks"], checksum(results[c], st["rounds"])))
if "--check" in sys.argv:
    ref, seconds = host_check(n, ro.cpu().numpy(), ci.cpu().numpy(), max_rounds)
    same = np.array_equal(results[configs[0]], ref["colour"]) and stats[configs[0]]["rounds"] == ref["rounds"]
    print("%s | checker %.3f s, %s" % (what, seconds, "identical" if same else "DIFFERENT"))
    assert same
p.close()
