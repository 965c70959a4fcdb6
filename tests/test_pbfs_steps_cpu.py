"""The lockstep driver of tests/_pbfs_lockstep.py with the numpy model on every rank: every graph, schedule, P, source and both
ways of `trailing` must give the serial BFS labels.  This pins the model and the case list that tests/test_pbfs_steps_gpu.py runs
the HIP engine against; no GPU is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pbfs_lockstep as ls  # noqa: E402


def test_graphs_are_the_shapes_the_cases_are_about():
    from gunrockinst_amd import multi_gpu as mg
    for name, (n, ro, ci) in ls.GRAPHS.items():
        assert ro.shape == (n + 1,) and ro[0] == 0 and ro[-1] == ci.shape[0] and (np.diff(ro) >= 0).all()
        rows = np.repeat(np.arange(n), np.diff(ro))
        assert (rows != ci).all() and np.unique(rows.astype(np.int64) * n + ci).shape[0] == ci.shape[0]  # no loops, no duplicates
        pairs = set(zip(rows.tolist(), ci.tolist()))
        if name in ls.DIRECTED:
            assert (rows < ci).all()
        else:
            assert all((b, a) in pairs for a, b in pairs), name
    local = lambda name, p: [mg.local_count(ls.GRAPHS[name][0], p, r) for r in range(p)]
    assert local("rand_191", 3) == [64, 64, 63] and local("rand_192", 3) == [64, 64, 64] and local("rand_193", 3) == [65, 64, 64]
    assert [mg.mask_words(x) for x in local("rand_193", 3)] == [4, 2, 2]
    assert local("rand_1535", 3) == [512, 512, 511] and local("rand_1537", 3) == [513, 512, 512]
    assert local("sparse_12289", 3) == [4097, 4096, 4096]
    assert local("one_vertex", 8) == [1] + [0] * 7 and local("two", 3) == [1, 1, 0]
    n, ro, ci = ls.GRAPHS["star_700"]
    assert ro[700] - ro[699] == 699 > 512 and ci[ro[700] - 1] == 698 and ls.sources("star_700") == [0, 699, 698]
    n, ro, ci = ls.GRAPHS["path_200"]
    assert (np.diff(ro)[1:-1] == 2).all()
    n, ro, ci = ls.GRAPHS["isolated_tail"]
    assert ci.shape[0] == 10 and (np.diff(ro)[67:] == 0).all()
    n, ro, ci = ls.GRAPHS["sparse_12289"]
    assert (np.diff(ro) == 0).sum() > 500
    n, ro, ci = ls.GRAPHS["dag_64"]
    assert ro[64] == ro[63] and ls.schedules("dag_64") == ["td"]   # a sink: labelled by the filter, never a frontier vertex


@pytest.mark.parametrize("name", list(ls.GRAPHS))
def test_model_on_every_rank_gives_the_serial_bfs(name):
    for src in ls.sources(name):
        ref, depth = ls.serial_bfs(name, src)
        for parts in ls.PARTS:
            engines = ls.model_engines(name, parts)
            for sched in ls.schedules(name):
                for trailing in (False, True):
                    labels, levels = ls.run(engines, src, ls.SCHEDULES[sched], trailing)
                    assert np.array_equal(labels, ref), (name, src, parts, sched, trailing)
                    assert levels in (depth - 1, depth), (name, src, parts, sched, trailing, levels, depth)


def test_check_callback_sees_every_step():
    seen = []
    engines = ls.model_engines("rand_193", 3)
    ls.run(engines, 0, ls.SCHEDULES["alt"], True, check=lambda step, res: seen.append(step))
    assert seen[0] == "reset" and {"advance_local", "filter_received", "queue_to_bitmap", "bottom_up", "bitmap_to_queue", "level"} <= set(seen)
