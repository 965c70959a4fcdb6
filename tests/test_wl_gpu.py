"""Colour refinement on the GPU (grx_wl_*): the colouring, the class sizes, the representatives, the state, the rounds and the round
trace must equal tests/_wl_checker.py's with np.array_equal, under every forced value of the options that are named -- the path of 65
(one split per round), regular graphs (one class, the certificate alone), twin hubs under every strategy and on every rung of the
certificate, the multiset semantics, awkward labels, capped rounds, the history, the repair path at one signature bit, the quotient
through spgemm, relabelling, the isomorphism screen, handle reuse and the refusals, and the goldens."""
import functools
import os

import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _wl_checker as k

pytestmark = pytest.mark.gpu

STRATEGIES = (ga.WL_AUTO, ga.WL_LANE, ga.WL_WAVE, ga.WL_BLOCK)
NOT_READY = "code 600"  # hipErrorNotReady


@functools.lru_cache(maxsize=None)
def _reference(key):
    n, ro, ci, labels = _GRAPHS[key]
    ref = k.rounds(n, ro, ci, labels)
    for a in [ref["colour"]] + ref["history"]:
        a.setflags(write=False)
    return ref


_GRAPHS = {}


def _graph(key, n, ro, ci, labels=None):
    """registers a graph under a name, so that its reference is computed once and shared"""
    if key not in _GRAPHS:
        _GRAPHS[key] = (n, np.asarray(ro, np.int32), np.asarray(ci, np.int32), labels)
    return key


def _compare(p, key, what, max_rounds=-1, repairs=0):
    n, ro, ci, labels = _GRAPHS[key]
    ref = _reference(key)
    h = ref["rounds"] if max_rounds < 0 else min(max_rounds, ref["rounds"])
    want = ref["history"][h]
    colour, size, rep = p.extract()
    st = p.stats()
    print(what, {x: st[x] for x in ("rounds", "state", "classes", "repairs", "certificate_runs", "regime_rows", "rung_rows", "readbacks")})
    assert colour.dtype == np.int32 and np.array_equal(colour, want), "the colouring differs from the checker: " + what
    want_size, want_rep = k.sizes_and_representatives(want)
    assert size.dtype == np.int64 and np.array_equal(size, want_size) and rep.dtype == np.int32 and np.array_equal(rep, want_rep), what
    assert st["classes"] == want_size.shape[0] and st["entries"] == ci.shape[0], what
    assert st["state"] == (ga.WL_CAPPED if 0 <= max_rounds <= ref["rounds"] else ga.WL_STABLE), what
    if repairs is not None:
        assert st["repairs"] == repairs and st["rounds"] == h and p.round_trace().tolist() == ref["trace"][:h + 1], (what, st)
        assert st["readbacks"] == 1 + st["rounds"] + (st["state"] == ga.WL_STABLE), (what, st)
    return st


def _run(key, strategies=(ga.WL_AUTO,), max_rounds=-1, repairs=0, handle=None, **options):
    """the graph under every strategy on one handle, everything against the checker; returns the stats of the last run"""
    n, ro, ci, labels = _GRAPHS[key]
    p = handle if handle is not None else ga.WlProblem().init(n, ro, ci)
    assert p.set_option("max_rounds", max_rounds) == 0
    for name, value in options.items():
        assert p.set_option(name, value) == 0, name
    st = None
    for strategy in strategies:
        assert p.set_option("strategy", strategy) == 0
        p.reset(labels)
        p.enact()
        st = _compare(p, key, "%s strategy %d max_rounds %d %s" % (key, strategy, max_rounds, options), max_rounds, repairs)
        if strategy != ga.WL_AUTO:
            assert sum(st["regime_rows"]) == st["regime_rows"][strategy - 1] > 0
    if handle is None:
        p.close()
    return st


def _path65():
    return _graph("path65", 65, *k.path(65))


def _twins():
    n, ro, ci, _ = k.twin_hubs()
    return _graph("twins", n, ro, ci)


def _golden(golden_dir, name, undirected):
    g = o.build_market(os.path.join(golden_dir, name + ".mtx"), undirected=undirected)
    return _graph("%s-%d" % (name, undirected), g.nodes, g.row_offsets, g.col_indices)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_path_of_65(strategy):
    key = _path65()
    st = _run(key, strategies=(strategy,))
    ref = _reference(key)
    assert (st["classes"], st["rounds"]) == (33, 32) and ref["trace"] == list(range(1, 34))
    assert st["certificate_runs"] == 1, "only the round that split nothing is certified"


@pytest.mark.parametrize("name", ["cycle64", "petersen", "c6_2k3"])
def test_regular_graphs(name):
    n, (ro, ci) = {"cycle64": (64, k.mirrored(64, k.cycle(64))), "petersen": (10, k.petersen()), "c6_2k3": (12, k.c6_and_triangles())}[name]
    st = _run(_graph(name, n, ro, ci), strategies=STRATEGIES)
    assert (st["classes"], st["rounds"], st["certificate_runs"]) == (1, 0, 1)
    assert sum(st["rung_rows"]) == n - 1, "every vertex but 0 is compared with vertex 0"


@pytest.mark.parametrize("strategy", [ga.WL_LANE, ga.WL_WAVE, ga.WL_BLOCK])
def test_twin_hubs_under_every_strategy(strategy):
    key = _twins()
    n = _GRAPHS[key][0]
    st = _run(key, strategies=(strategy,))
    assert st["classes"] == n - 3 and st["certificate_runs"] == 1
    assert sum(st["rung_rows"]) == 3, "the second twin of each of the three pairs is compared with the first"


def test_twin_hubs_on_every_rung():
    key = _twins()
    p = ga.WlProblem().init(*_GRAPHS[key][:3])
    st = _run(key, handle=p)  # the default tables: the 600-entry rows in the workgroup's table, the others in a wave's
    assert st["rung_rows"][0] > 0 and st["rung_rows"][1] > 0 and st["rung_rows"][2] == 0
    st = _run(key, handle=p, table_slots=64, block_slots=256, scratch_mib=1)
    assert min(st["rung_rows"]) > 0, "rows of 10, 40 and 600 entries: a wave's table, the workgroup's, the global counters"
    st = _run(key, handle=p, strategies=(ga.WL_AUTO, ga.WL_WAVE), table_slots=64, block_slots=256, scratch_mib=1, lane_max_row=4, wave_max_row=64)
    assert min(st["rung_rows"]) > 0
    p.close()


def test_multiset_semantics():
    st = _run(_graph("dup", 4, *k.csr_of(4, [0, 0, 1, 2], [3, 3, 3, 3])), strategies=STRATEGIES)  # rows [3, 3] and [3] differ
    assert st["classes"] == 3
    st = _run(_graph("loop", 3, *k.csr_of(3, [0, 0, 1, 1], [0, 2, 2, 2])), strategies=STRATEGIES)  # a self-loop against a duplicate
    assert st["classes"] == 3
    st = _run(_graph("oneway", 3, *k.csr_of(3, [0], [1])), strategies=STRATEGIES)  # only out-rows count: 1 and 2 stay together
    assert st["classes"] == 2
    assert _run(_graph("empty", 5, np.zeros(6, np.int32), np.zeros(0, np.int32)))["classes"] == 1


def test_start_labels():
    ro, ci = k.path(6)
    labels = np.array([2147483647, -5, 2147483647, -2147483648, -5, 2147483646], np.int32)
    key = _graph("labelled", 6, ro, ci, labels)
    _run(key, strategies=STRATEGIES)
    p = ga.WlProblem().init(6, ro, ci)
    _run(key, handle=p, max_rounds=0)
    assert p.extract()[0].tolist() == [0, 1, 0, 2, 1, 3] and p.extract()[2].tolist() == [0, 1, 3, 5]
    p.close()


@pytest.mark.parametrize("h", [0, 1, 2, 40, -1])
def test_max_rounds(h):
    st = _run(_path65(), max_rounds=h)
    assert st["state"] == (ga.WL_CAPPED if 0 <= h <= 32 else ga.WL_STABLE)
    if h >= 0:
        assert st["certificate_runs"] == st["rounds"] + (st["state"] == ga.WL_STABLE), "every round of a capped run is certified"


@pytest.mark.parametrize("sig_bits", [128, 2])
def test_history(golden_dir, sig_bits):
    for key, rounds in ((_path65(), 40), (_golden(golden_dir, "chesapeake", True), 64), (_path65(), 3)):
        n, ro, ci, labels = _GRAPHS[key]
        ref = _reference(key)
        p = ga.WlProblem().init(n, ro, ci)
        for name, value in (("history", 1), ("max_rounds", rounds), ("sig_bits", sig_bits), ("max_repairs", 1 << 20)):
            assert p.set_option(name, value) == 0
        p.enact()
        st = _compare(p, key, "history %s sig_bits %d" % (key, sig_bits), max_rounds=rounds, repairs=None)
        want = ref["history"][:min(rounds, ref["rounds"]) + 1]
        got = p.history()
        assert got.dtype == np.int32 and got.shape == (len(want), n) and all(np.array_equal(a, b) for a, b in zip(got, want))
        assert st["rounds"] == len(want) - 1 and p.round_trace().tolist() == ref["trace"][:len(want)], "rounds stays exact"
        if sig_bits == 128:
            assert st["repairs"] == 0
        elif key == "path65" and rounds == 40:  # 32 certified rounds, each refused with probability 1/4 at the least
            assert st["repairs"] >= 1
        p.close()
    got = ga.gunrock_colour_refinement(*_GRAPHS[_path65()][:3], max_rounds=2, history=True)
    assert got["state"] == ga.WL_CAPPED and got["rounds"] == 2 and np.array_equal(got["history"][2], _reference("path65")["history"][2])


def test_repair_path():
    key = _path65()
    n, ro, ci, _ = _GRAPHS[key]
    p = ga.WlProblem().init(n, ro, ci)
    assert p.set_option("sig_bits", 1) == 0 and p.set_option("max_repairs", 4096) == 0
    p.enact()
    st = _compare(p, key, "path65 sig_bits 1", repairs=None)
    # 32 splits that come one at a time, each found with probability 1/2: no stall has probability 2^-32
    assert 1 <= st["repairs"] <= 4096 and st["certificate_runs"] == st["repairs"] + 1
    assert p.set_option("max_repairs", 0) == 0
    with pytest.raises(ga.WlNotCertified):
        p.enact()
    with pytest.raises(RuntimeError, match=NOT_READY):  # it does not return a partition
        p.extract()
    assert p.set_option("sig_bits", 128) == 0
    p.enact()
    _compare(p, key, "path65 again")
    p.close()


def test_quotient_through_spgemm(golden_dir):
    key = _golden(golden_dir, "chesapeake", True)
    n, ro, ci, _ = _GRAPHS[key]
    got = ga.gunrock_colour_refinement(n, ro, ci)
    assert np.array_equal(got["colour"], _reference(key)["colour"]) and got["state"] == ga.WL_STABLE
    size, colour = got["class_size"], got["colour"]
    q = k.quotient(n, ro, ci, colour)
    t = ga.gunrock_quotient_graph(ro, ci, None, colour)
    dense = np.zeros_like(q)
    rows = np.repeat(np.arange(q.shape[0]), np.diff(t["offsets"]))
    dense[rows, t["cols"]] = t["vals"]
    assert tuple(t["shape"]) == q.shape and np.array_equal(dense, size[:, None] * q), "P^T A P is not s[i] q[i][j]"


def test_relabelling_maps_classes_onto_classes():
    rng = np.random.default_rng(11)
    n, ro, ci, _ = k.random_graph(np.random.default_rng(3), 64)
    while n < 30:
        n, ro, ci, _ = k.random_graph(rng, 64)
    perm = rng.permutation(n)  # vertex v becomes perm[v]
    rows = np.repeat(np.arange(n), np.diff(ro))
    pro, pci = k.csr_of(n, perm[rows], perm[ci], shuffle=rng)
    a = ga.gunrock_colour_refinement(n, ro, ci)["colour"]
    b = ga.gunrock_colour_refinement(n, pro, pci)["colour"]
    assert np.array_equal(a, _reference(_graph("relabel-a", n, ro, ci))["colour"])
    pairs = set(zip(a.tolist(), b[perm].tolist()))
    assert len(pairs) == int(a.max()) + 1 == int(b.max()) + 1, "the classes of the copy are the images of the classes"


def test_wl_test():
    c6, k3k3 = k.mirrored(6, k.cycle(6)), k.mirrored(6, k.cycle(3) + k.cycle(3, 3))
    assert ga.gunrock_wl_test(c6, k3k3) is True  # 1-WL cannot tell two 2-regular graphs apart
    p4, star = k.path(4), k.star(3)
    assert ga.gunrock_wl_test(p4, star) is False
    rng = np.random.default_rng(5)
    n, ro, ci, _ = k.twin_hubs(seed=9, core=100, p=0.1, shared=(20,))
    perm = rng.permutation(n)
    rows = np.repeat(np.arange(n), np.diff(ro))
    copy = k.csr_of(n, perm[rows], perm[ci], shuffle=rng)
    assert ga.gunrock_wl_test((ro, ci), copy) is True
    labels = np.zeros(n, np.int32)
    labels[0] = 1
    moved = np.zeros(n, np.int32)
    moved[perm[0]] = 1
    assert ga.gunrock_wl_test((ro, ci), copy, labels, moved) is True
    assert ga.gunrock_wl_test(c6, k3k3, [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1]) is False  # a marked vertex tells the cycle from the triangles


def test_handle_use(golden_dir):
    import torch
    key = _golden(golden_dir, "chesapeake", True)
    n, ro, ci, _ = _GRAPHS[key]
    p = ga.WlProblem(instrument=True)
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.enact()
    d_ro, d_ci = torch.from_numpy(ro).cuda(), torch.from_numpy(ci).cuda()
    p.init_device(n, ci.shape[0], d_ro.data_ptr(), d_ci.data_ptr())
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.extract()
    assert p.device_results() == {"colour": None, "class_size": None, "representative": None}
    p.enact()  # without a Reset: one class
    _compare(p, key, "borrowed device arrays")
    assert p.stats()["kernel_ms"] > 0 and all(p.device_results().values())
    labels = (np.arange(n) % 3 - 1).astype(np.int32)
    labelled = _graph("chesapeake-labelled", n, ro, ci, labels)
    p.reset(labels)
    with pytest.raises(RuntimeError, match=NOT_READY):  # a Reset takes the result away
        p.extract()
    p.enact()
    _compare(p, labelled, "other labels")
    p.enact()  # again without a Reset: the same labels
    _compare(p, labelled, "the same labels again")
    p.reset(None)
    p.enact()
    _compare(p, key, "no labels again")
    with pytest.raises(RuntimeError, match="code -3"):  # a second init
        p.init(n, ro, ci)
    assert p.set_option("nope", 1) == 1
    for name, value in (("strategy", 4), ("sig_bits", 0), ("sig_bits", 129), ("table_slots", 96), ("max_rounds", -2), ("max_repairs", -1),
                        ("history", 2), ("scratch_mib", 0), ("seed", -1)):
        with pytest.raises(RuntimeError, match="code -1"):
            p.set_option(name, value)
    assert p.set_option("history", 1) == 0
    with pytest.raises(RuntimeError, match="code -1"):  # history asks for max_rounds in 1 .. 64
        p.enact()
    with pytest.raises(RuntimeError, match=NOT_READY):
        p.history()
    p.close()
    bad = ro.copy()
    bad[3] = bad[4] + 1  # offsets that decrease
    q = ga.WlProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        q.init(n, bad, ci)
    with pytest.raises(RuntimeError, match="code -3"):
        q.init(n, ro, ci)
    q.close()
    q = ga.WlProblem()
    with pytest.raises(RuntimeError, match="code -2"):
        q.init(n, ro, np.where(np.arange(ci.shape[0]) == 5, n, ci).astype(np.int32))  # a column that is no vertex
    q.close()


def test_seed_and_sig_bits_change_no_result(golden_dir):
    key = _golden(golden_dir, "chesapeake", False)
    p = ga.WlProblem().init(*_GRAPHS[key][:3])
    for seed, sig_bits in ((0, 128), (12345, 128), (7, 64), (7, 65), (1 << 40, 16)):
        _run(key, handle=p, seed=seed, sig_bits=sig_bits, repairs=None)
    p.close()


@pytest.mark.parametrize("name,undirected", [("chesapeake", True), ("chesapeake", False), ("bips98_606", True), ("bips98_606", False)])
def test_goldens(golden_dir, name, undirected):
    key = _golden(golden_dir, name, undirected)
    st = _run(key, strategies=STRATEGIES)
    assert st["repairs"] == 0 and k.is_equitable(*_GRAPHS[key][:3], _reference(key)["colour"])
