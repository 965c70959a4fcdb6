"""Minimum spanning forest timing on a device-built R-MAT (mirrored, hashed weights 1..64), Reset + Enact; also usable under
rocprofv3 --kernel-trace: python tools/one_mst.py <scale> [reps] [--trace]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gunrockinst_amd as ga
from gunrockinst_amd import devgraph

scale = int(sys.argv[1]); reps = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 5
ro, ci = devgraph.rmat_csr_device(scale, 8)
n, m = ro.shape[0] - 1, ci.shape[0]
rows = torch.repeat_interleave(torch.arange(n, device=ci.device, dtype=torch.int64), (ro[1:] - ro[:-1]).long())
lo, hi = torch.minimum(rows, ci.long()), torch.maximum(rows, ci.long())
h = (lo * 0x9E3779B1 + hi * 0x85EBCA77) & 0xFFFFFFFF
w = ((h ^ (h >> 15)) % 64 + 1).int().contiguous()
del rows, lo, hi, h
torch.cuda.synchronize()
times = []
p = ga.MstProblem(False).init_device(n, m, ro.data_ptr(), ci.data_ptr(), w.data_ptr())
for rep in range(reps + 1):
    p.reset(); ms = p.enact()
    if rep: times.append(ms)
_, total, forest = p.extract(selected=False)
st = p.stats()
p.close()
times.sort()
print("scale %d nodes %d entries %d: enact ms median %.3f min %.3f | forest edges %d weight %d | %s" % (
    scale, n, m, times[len(times) // 2], times[0], forest, total, st))
if "--trace" in sys.argv:  # per round: entries read by the minimum step and the round's time (events around every round)
    p = ga.MstProblem(True).init_device(n, m, ro.data_ptr(), ci.data_ptr(), w.data_ptr())
    p.reset(); p.enact()
    for i, r in enumerate(p.round_trace()):
        print("round %d entries %d ms %.3f" % (i + 1, r["entries"], r["ms"]))
    print("instrumented", p.stats())
    p.close()
