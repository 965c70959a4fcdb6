"""Sparse-product timing on a device-built graph, median of `reps` Enacts; also usable under rocprofv3 --kernel-trace:
python tools/one_spgemm.py <scale> [reps] [--edge-factor F] [--no-scipy] [--no-torch] [--scipy-max-products N]

<scale>: mirrored R-MAT of 2^scale vertices, edge factor 16 (devgraph.rmat_csr_device), values absent.  A A and A A^T on one handle:
ms per Enact, products/s, output bytes/s (12 bytes an entry), the regime split of the rows and the products, and -- from one Enact of
an instrumented handle -- the kernel time of every regime.  The yardsticks, in the same run and never the code under test:
scipy.sparse int64 on the CPU (once; skipped beyond --scipy-max-products products), whose offsets, columns and values the library's
must equal, and torch.sparse.mm in float64 on the GPU where torch offers it (the vendor's SpGEMM; its values are floats, a time
yardstick only)."""
import sys, os, time
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
edge_factor = int(option("--edge-factor", "16"))
scipy_max = float(option("--scipy-max-products", "3e9"))
scale = int(args[0])
reps = int(args[1]) if len(args) > 1 else 5
ro, ci = devgraph.rmat_csr_device(scale, edge_factor)
n, m = ro.shape[0] - 1, ci.shape[0]
torch.cuda.synchronize()
REGIMES = ("lane", "wave", "block", "global")


def median(t):
    t = sorted(t)
    return t[len(t) // 2], t[0]


def result(p):
    rows, cols, nnz = p.sizes()
    d = p.device_results()
    return (devgraph.as_tensor(d["offsets"], rows + 1, "<i4"), devgraph.as_tensor(d["cols"], nnz, "<i4"), devgraph.as_tensor(d["vals"], nnz, "<i8"))


p = ga.SpgemmProblem(False).init_device((n, n), m, ro.data_ptr(), ci.data_ptr())
q = ga.SpgemmProblem(True).init_device((n, n), m, ro.data_ptr(), ci.data_ptr())
print("rmat%d edge factor %d: nodes %d entries %d" % (scale, edge_factor, n, m), flush=True)
for name, right in (("A A", ga.SPGEMM_SELF), ("A A^T", ga.SPGEMM_TRANSPOSE)):
    p.set_option("right", right)
    q.set_option("right", right)
    try:
        p.enact()  # (the transpose is built here, outside the timed Enacts)
    except ga.SpgemmTooLarge as e:
        print("rmat%d | %s: refused, %s" % (scale, name, e), flush=True)
        continue
    first = [x.clone() for x in result(p)]
    times = []
    for _ in range(reps):
        times.append(p.enact())
        assert all(torch.equal(x, y) for x, y in zip(result(p), first)), "two Enacts disagree"
    st = p.stats()
    med, low = median(times)
    q.enact()
    sq = q.stats()
    assert all(torch.equal(x, y) for x, y in zip(result(q), first)), "the instrumented handle disagrees"
    split = " ".join("%s %d rows (%.1f%%) %d products (%.1f%%) %.3f ms (%.1f%%)" % (
        r, st[r + "_rows"], 100.0 * st[r + "_rows"] / n, st[r + "_products"], 100.0 * st[r + "_products"] / max(st["products"], 1), sq[r + "_ms"],
        100.0 * sq[r + "_ms"] / max(sq["kernel_ms"], 1e-9)) for r in REGIMES)
    print("rmat%d | %s: enact ms median %.3f min %.3f | products %d (%.3f G/s) | nnz %d (%.3f GB/s of output) | table probes %d launches %d "
          "read-backs %d | instrumented kernel ms %.3f | %s" % (scale, name, med, low, st["products"], st["products"] / med / 1e6, st["nnz"],
                                                            12.0 * st["nnz"] / med / 1e6, st["table_probes"], st["kernel_launches"], st["readbacks"],
                                                            sq["kernel_ms"], split), flush=True)
    if "--no-torch" not in sys.argv:
        try:
            ones = torch.ones(m, dtype=torch.float64, device="cuda")
            ta = torch.sparse_csr_tensor(ro.to(torch.int64), ci.to(torch.int64), ones, size=(n, n))
            tb = ta if right == ga.SPGEMM_SELF else ta.to_sparse_coo().t().to_sparse_csr()
            tt = []
            for rep in range(min(reps, 3) + 1):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                tc = torch.sparse.mm(ta, tb)
                stop.record()
                torch.cuda.synchronize()
                if rep:
                    tt.append(start.elapsed_time(stop))
            tm, tl = median(tt)
            print("rmat%d | %s: torch.sparse.mm float64 ms median %.3f min %.3f (nnz %d) | x %.2f of the library's" % (
                scale, name, tm, tl, tc._nnz(), tm / med), flush=True)
            del tc, ta, tb
        except Exception as e:  # a build of torch without sparse CSR products on this device
            print("rmat%d | %s: torch.sparse.mm not offered here: %s" % (scale, name, str(e).splitlines()[0][:200]), flush=True)
    if "--no-scipy" not in sys.argv and st["products"] <= scipy_max:
        import scipy.sparse as sp
        ha = sp.csr_matrix((np.ones(m, dtype=np.int64), ci.cpu().numpy(), ro.cpu().numpy()), shape=(n, n))
        hb = ha if right == ga.SPGEMM_SELF else ha.T.tocsr()
        t0 = time.time()
        hc = ha @ hb
        cpu_ms = (time.time() - t0) * 1e3
        hc.sort_indices()
        same = np.array_equal(hc.indptr, first[0].cpu().numpy()) and np.array_equal(hc.indices, first[1].cpu().numpy()) and \
            np.array_equal(hc.data, first[2].cpu().numpy())
        assert same, "the library's product differs from scipy's"
        print("rmat%d | %s: scipy.sparse int64 on the CPU ms %.1f | x %.1f of the library's | equal to the library's result" % (
            scale, name, cpu_ms, cpu_ms / med), flush=True)
p.close()
q.close()
