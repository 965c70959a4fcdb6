"""The level loop inside the library (grx_pbfs_search) with real peers on the edge-case graphs of tests/_pbfs_lockstep.py:
2, 3 and 5 ranks share the GPU and exchange over gloo (callback transport), so there are ranks that own no vertex, ranks whose
bitmap is shorter than the gathered stride, and P = 5 in the striped division.  Every graph, every option set of
_pbfs_lockstep.LIBRARY_OPTIONS and every source; labels against the serial BFS, parents with the oracle's validator, the
count-only level statistic."""
import os
import socket
import sys
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    # (a stuck exchange raises after a minute instead of hanging)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    from gunrockinst_amd import multi_gpu as mg
    import _pbfs_lockstep as ls

    comm = mg.Comm()
    # No assertion inside the sequence: a rank that left early would strand its peers in a collective.  Every rank makes
    # the same calls; the mismatching cases are collected and reported at the end.
    bad = []
    for name, (n, _, _) in ls.GRAPHS.items():
        ro, ci = ls.slices(name, world)[rank]
        ro_d, ci_d = torch.from_numpy(ro).cuda(), torch.from_numpy(ci).cuda()
        torch.cuda.synchronize()
        eng = mg.HipEngine(n, world, rank, ro_d, ci_d, 0)
        bfs = mg.LibraryBfs(eng, comm, transport="callbacks")
        for key, opt in ls.library_options(name).items():
            ls.configure(bfs, opt)
            for src in ls.sources(name):
                before = bfs.stat("marked_levels")
                levels, _ = bfs.search(src, direction_optimizing=opt["dobfs"])
                labels = mg.assemble_labels(comm, eng.labels(), n)
                preds = mg.assemble_labels(comm, bfs.preds(), n) if opt["mark_pred"] else None  # (same decision on every rank)
                for what in ls.check_library_search(name, src, opt, levels, labels, preds, before, bfs.stat("marked_levels")):
                    bad.append("rank %d: %s %s src=%d: %s" % (rank, name, key, src, what))
        eng.close()
    everyone = [None] * world
    dist.all_gather_object(everyone, bad)
    if rank == 0:
        lines = [line for per_rank in everyone for line in per_rank]
        with open(out, "w") as f:
            f.write("ok" if not lines else "\n".join(lines))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 5])
def test_library_level_loop_with_peers_on_the_edge_graphs(tmp_path, world):
    out = str(tmp_path / "result.txt")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    result = open(out).read()
    assert result == "ok", result
