"""The two CPU restatements of colour refinement (tests/_wl_checker.py) against each other, without a GPU: the rounds as defined and
the splitter queue must give the same numbered partition, and it must be equitable, on the hand graphs of the GPU tests, on the
goldens read directed and undirected, and on 200 seeded random graphs with loops, duplicates and one-way entries.  The rounds
truncated at h must be round h of the full run."""
import os

import numpy as np
import pytest

from oracle import gr_oracle as o

import _wl_checker as k


def _both(n, ro, ci, labels=None):
    a = k.rounds(n, ro, ci, labels)
    b = k.splitters(n, ro, ci, labels)
    assert a["colour"].dtype == np.int32 and np.array_equal(a["colour"], b), "the two routes differ"
    assert k.is_equitable(n, ro, ci, a["colour"]) and a["state"] == k.STABLE
    assert a["trace"] == sorted(set(a["trace"])) and len(a["trace"]) == a["rounds"] + 1, "every round splits"
    if labels is not None:  # the partition refines the labels
        assert len(set(zip(a["colour"].tolist(), np.asarray(labels).tolist()))) == int(a["colour"].max()) + 1
    return a


def test_path_of_65():
    ro, ci = k.path(65)
    a = _both(65, ro, ci)
    assert a["rounds"] == 32 and a["trace"] == list(range(1, 34)), "one split per round, 33 classes"
    assert np.array_equal(a["colour"], np.minimum(np.arange(65), 64 - np.arange(65)))


@pytest.mark.parametrize("name", ["cycle64", "petersen", "c6_2k3"])
def test_regular_graphs_are_one_class(name):
    n, (ro, ci) = {"cycle64": (64, k.mirrored(64, k.cycle(64))), "petersen": (10, k.petersen()), "c6_2k3": (12, k.c6_and_triangles())}[name]
    a = _both(n, ro, ci)
    assert a["rounds"] == 0 and not a["colour"].any()


def test_multiset_semantics():
    # rows [1, 1] and [1] differ; 2 and 3 have empty rows
    ro, ci = k.csr_of(4, [0, 0, 1, 2], [3, 3, 3, 3])
    a = _both(4, ro, ci)
    assert a["colour"].tolist() == [0, 1, 1, 2]
    # a self-loop tells two vertices with rows of one length apart: 0 -> {0, 2}, 1 -> {2, 2}
    ro, ci = k.csr_of(3, [0, 0, 1, 1], [0, 2, 2, 2])
    assert _both(3, ro, ci)["colour"].tolist() == [0, 1, 2]
    # one-way entries give only out-rows: 0 -> 1, nothing back
    ro, ci = k.csr_of(3, [0], [1])
    assert _both(3, ro, ci)["colour"].tolist() == [0, 1, 1]


def test_twin_hubs_share_a_class():
    n, ro, ci, twins = k.twin_hubs()
    a = _both(n, ro, ci)
    size, _ = k.sizes_and_representatives(a["colour"])
    for x, y in twins:
        assert a["colour"][x] == a["colour"][y] and size[a["colour"][x]] == 2
    assert int(a["colour"].max()) + 1 == n - len(twins), "the G(n, p) part is rigid"


def test_labels_are_grouped_and_numbered_by_smallest_member():
    ro, ci = k.path(6)
    labels = np.array([2147483647, -5, 2147483647, -2147483648, -5, 2147483646], np.int32)
    a = k.rounds(6, ro, ci, labels, max_rounds=0)
    assert a["colour"].tolist() == [0, 1, 0, 2, 1, 3] and a["state"] == k.CAPPED
    _both(6, ro, ci, labels)


@pytest.mark.parametrize("name,undirected", [("chesapeake", True), ("chesapeake", False), ("bips98_606", True), ("bips98_606", False)])
def test_goldens(golden_dir, name, undirected):
    g = o.build_market(os.path.join(golden_dir, name + ".mtx"), undirected=undirected)
    a = _both(g.nodes, g.row_offsets, g.col_indices)
    assert a["rounds"] >= 1


def test_random_graphs():
    rng = np.random.default_rng(20261020)
    for _ in range(200):
        n, ro, ci, labels = k.random_graph(rng)
        _both(n, ro, ci, labels)


def test_truncated_rounds_are_the_rounds_of_the_full_run():
    rng = np.random.default_rng(7)
    cases = [(65,) + k.path(65) + (None,)] + [k.random_graph(rng) for _ in range(20)]
    for n, ro, ci, labels in cases:
        full = k.rounds(n, ro, ci, labels)
        for h in range(0, min(full["rounds"], 5) + 2):
            cut = k.rounds(n, ro, ci, labels, max_rounds=h)
            want = full["history"][min(h, full["rounds"])]
            assert np.array_equal(cut["colour"], want) and cut["rounds"] == min(h, full["rounds"])
            assert cut["state"] == (k.CAPPED if h <= full["rounds"] else k.STABLE)
