"""The per-rank steps of the partitioned BFS (grx_pbfs_*: csrc/lib/partitioned_bfs.hip, oprtr/advance/bottom_up.hpp) in
lockstep against the numpy model, and the library's own level loop on one rank.

All P ranks of a search are P HipEngine handles in this process on the one GPU; the exchange is torch.cat
(tests/_pbfs_lockstep.py).  After every step of every rank the send counts and per-owner id sets, the (len, edges) pairs, the
frontier bitmap with its padding, and the labels are compared with the model's; at the end the labels with the serial BFS and
the parents with what the step-wise path promises.  The graphs are the smallest on which the striped arithmetic, the bitmap
tails and the sweeps' step and chunk sizes matter (see _pbfs_lockstep.GRAPHS).

Case matrix per graph (sources: 0, n - 1, the first vertex of highest degree "hub", plus the graph's extras):
  every P in 1, 2, 3, 5, 8 : td_bu_td, trailing words behind every gathered bitmap, from every source;
  every P                  : every schedule (td, bu, td_bu, bu_td, td_bu_td, alt), no trailing words, from the hub and
                             the graph's extras (P = 3: from every source);
  every P                  : walk_queue = 0 with bu and alt, trailing words, from the same sources.
(star_700's extra, leaf 698, is the hub's last row entry: under bu the hub finds it only at the end of its row walk.)
Only the sources are trimmed, because of path_200 (199 levels of a few dozen synchronising calls per rank each).
dag_64 is directed: its schedule is td everywhere (walk_queue only matters to a sweep, so it has no such case).
The engines of a (graph, P) are created once and reused over its cases, so reset() runs after finished and after
switched searches.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pbfs_lockstep as ls  # noqa: E402

pytestmark = pytest.mark.gpu


def matrix(name, parts):
    """[(source, schedule, trailing, walk_queue)] of one (graph, P): fixed here, nothing is skipped at run time."""
    scheds = ls.schedules(name)
    hub = ls.hub(name)
    cases = [(s, "td_bu_td" if "td_bu_td" in scheds else "td", True, 1) for s in ls.sources(name)]
    some = ls.sources(name) if parts == 3 else [hub] + [s for s in ls.EXTRA_SOURCES.get(name, ()) if s != hub]
    cases += [(s, sc, False, 1) for sc in scheds for s in some]
    cases += [(s, sc, True, 0) for sc in ("bu", "alt") if sc in scheds for s in some]
    return cases


def hip_engines(name, parts):
    from gunrockinst_amd import multi_gpu as mg
    n = ls.GRAPHS[name][0]
    parts_csr = [(torch.from_numpy(ro).cuda(), torch.from_numpy(ci).cuda()) for ro, ci in ls.slices(name, parts)]
    torch.cuda.synchronize()
    engines = []
    try:
        for r, (ro, ci) in enumerate(parts_csr):
            engines.append(mg.HipEngine(n, parts, r, ro, ci, 0))
    except Exception:
        close(engines)
        raise
    return engines


def close(engines):
    for e in engines:
        e.close()


def set_option(engine, key, value):
    from gunrockinst_amd.multi_gpu import HipEngine
    HipEngine._check(engine.lib.grx_pbfs_set_option(engine._h, key.encode(), float(value)), "grx_pbfs_set_option(%s)" % key)


def test_matrix_covers_what_it_must():
    for name in ls.GRAPHS:
        for parts in ls.PARTS:
            cases = matrix(name, parts)
            main = "td" if name in ls.DIRECTED else "td_bu_td"
            assert {(s, main, True, 1) for s in ls.sources(name)} <= set(cases)
            assert {sc for _, sc, _, wq in cases if wq == 1} == set(ls.schedules(name))
            if name not in ls.DIRECTED:
                assert {sc for _, sc, _, wq in cases if wq == 0} >= {"bu", "alt"}


@pytest.mark.parametrize("parts", ls.PARTS, ids=lambda p: "P%d" % p)
@pytest.mark.parametrize("name", list(ls.GRAPHS))
def test_steps_side_by_side_with_the_model(name, parts):
    model = ls.model_engines(name, parts)
    hip = hip_engines(name, parts)
    try:
        for src, sched, trailing, walk_queue in matrix(name, parts):
            case = "%s P=%d src=%d %s trailing=%s walk_queue=%d" % (name, parts, src, sched, trailing, walk_queue)
            for e in hip:
                set_option(e, "walk_queue", walk_queue)
            try:
                labels, levels, found_bu = ls.run_side_by_side(model, hip, src, ls.SCHEDULES[sched], trailing)
                ref, depth = ls.serial_bfs(name, src)
                assert np.array_equal(labels, ref), "labels differ from the serial BFS at %s" % np.nonzero(labels != ref)[0].tolist()[:8]
                assert levels in (depth - 1, depth), "levels %d, depth %d" % (levels, depth)
                ls.check_stepwise_preds(name, src, labels, [e.preds() for e in hip], found_bu)
            except AssertionError as exc:
                raise AssertionError("%s: %s" % (case, exc)) from exc
    finally:
        close(hip)


class _SoloComm:
    """world 1 without torch.distributed: what LibraryBfs's callbacks need."""
    world, rank, group, host_staged = 1, 0, None, False

    def all_gather(self, t):
        return t

    def all_to_all_v(self, send, send_counts, recv_counts):
        return send


@pytest.mark.parametrize("name", list(ls.GRAPHS))
def test_library_level_loop_one_rank(name):
    from gunrockinst_amd import multi_gpu as mg
    (eng,) = hip_engines(name, 1)
    try:
        bfs = mg.LibraryBfs(eng, _SoloComm(), transport="callbacks")
        for key, opt in ls.library_options(name).items():
            ls.configure(bfs, opt)
            for src in ls.sources(name):
                before = bfs.stat("marked_levels")
                levels, ms = bfs.search(src, direction_optimizing=opt["dobfs"])
                bad = ls.check_library_search(name, src, opt, levels, eng.labels(), bfs.preds(), before, bfs.stat("marked_levels"))
                assert not bad and ms >= 0.0, "%s %s src=%d: %s" % (name, key, src, "; ".join(bad))
    finally:
        eng.close()
