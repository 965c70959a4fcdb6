"""The maximum-flow checker against itself, on the CPU: its three forms (plain-Python Dinic over the canonical pairs, scipy's
maximum_flow with residual = capacity - flow, networkx) agree on the flow value and on both residual reaches for the closed forms and
random cases the GPU tests run, the validator rejects hand-broken flows and cuts, the pair rules reject what init rejects, and the
R-MAT literals the GPU tests compare against are pinned here.  At scale 16 networkx is left out (most of a minute): scipy's Dinic
and the plain-Python Dinic are compared there."""
import numpy as np
import pytest

import _maxflow_checker as k

# scale -> (nodes, arcs, src, sink, value, side 0, side 1, side 2)
RMAT = {10: (1024, 6890, 0, 256, 946, 700, 315, 9), 12: (4096, 29522, 0, 128, 1965, 2562, 1519, 15),
        16: (65536, 503300, 0, 4, 11205, 35368, 30086, 82)}


def _agree(n, rows, cols, caps, s, t, shuffle=None):
    ro, ci, cap = k.csr_from_arcs(n, rows, cols, caps, shuffle)
    assert k.forms_disagree(n, ro, ci, cap, s, t) == []
    return k.solve(n, ro, ci, cap, s, t)


def test_closed_forms():
    assert _agree(2, [0], [1], [5], 0, 1)[4]["value"] == 5
    assert _agree(2, [0], [1], [5], 1, 0)[4]["value"] == 0
    assert _agree(2, [0, 1], [1, 0], [5, 7], 1, 0)[4]["value"] == 7
    ref = _agree(5, [0, 1, 3], [1, 2, 4], [4, 4, 4], 0, 4)[4]
    assert ref["value"] == 0 and ref["side"].tolist() == [0, 0, 0, 2, 2] and not ref["cut"].any()
    assert _agree(4, [0, 0, 0, 1, 2, 1], [1, 2, 1, 3, 3, 3], None, 0, 3)[4]["value"] == 3
    assert _agree(4, [0, 1, 2, 0], [1, 2, 3, 3], [0, 0, 0, 0], 0, 3)[4]["value"] == 0
    assert _agree(3, [0, 0, 0, 1, 1], [1, 1, 1, 2, 2], [2, 3, 4, 5, 1], 0, 2)[4]["value"] == 6
    ref = _agree(4, [0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2], [7, 100, 4, 100, 9, 100], 0, 3)[4]
    assert ref["value"] == 4 and ref["cut"].tolist() == [0, 3, 0]
    big = 2 ** 31 - 1
    assert _agree(3, [0, 0, 1, 1, 2], [0, 1, 1, 2, 2], [big, 3, big, 2, big], 0, 2)[4]["value"] == 2
    assert _agree(4, [0, 0, 1, 1, 2], [1, 2, 2, 3, 3], [10, 1, 10, 1, 10], 0, 3)[4]["value"] == 11
    assert _agree(4, [0, 0, 1, 1, 2], [1, 2, 2, 3, 3], [10, 10, 10, 3, 12], 0, 3)[4]["value"] == 15
    assert _agree(5, [0, 0, 0, 1, 2, 3], [1, 2, 3, 4, 4, 4], [2 ** 30] * 6, 0, 4)[4]["value"] == 3 * 2 ** 30


def test_path_sides():
    n, mid = 2001, 1000
    caps = np.full(n - 1, 10)
    caps[mid] = 3
    ref = _agree(n, np.arange(n - 1), np.arange(1, n), caps, 0, n - 1)[4]
    assert ref["value"] == 3 and np.array_equal(ref["side"], np.where(np.arange(n) <= mid, 0, 2))
    assert ref["cut"][mid] == 3 and int(ref["cut"].sum()) == 3


@pytest.mark.parametrize("seed", range(6))
def test_random_cases(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 300))
    m = int(rng.integers(0, 8 * n))
    rows, cols, caps = rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(0, 12, m)
    s, t = (int(x) for x in rng.choice(n, 2, replace=False))
    ref = _agree(n, rows, cols, caps, s, t, shuffle=rng)[4]
    perm = rng.permutation(n)
    moved = _agree(n, perm[rows], perm[cols], caps, int(perm[s]), int(perm[t]))[4]
    assert moved["value"] == ref["value"] and np.array_equal(moved["side"][perm], ref["side"])


def test_pair_rules():
    half = 2 ** 30
    with pytest.raises(k.Malformed):
        k.pairs_of(*((3,) + k.csr_from_arcs(3, [0, 1, 0], [1, 0, 1], [half, half, 0])))
    with pytest.raises(k.Malformed):
        k.pairs_of(*((3,) + k.csr_from_arcs(3, [0, 1], [1, 2], [3, -1])))
    a, b, cab, cba = k.pairs_of(*((3,) + k.csr_from_arcs(3, [0, 1, 1, 2, 2], [1, 0, 2, 2, 1], [half, half - 1, 0, 9, 0])))
    assert (a.tolist(), b.tolist(), cab.tolist(), cba.tolist()) == ([0, 1], [1, 2], [half, 0], [half - 1, 0])  # capacity 0 is a pair


def test_validator_rejects_broken_flows():
    n, rows, cols, caps = 4, [0, 0, 1, 1, 2], [1, 2, 2, 3, 3], [10, 10, 10, 3, 12]
    ro, ci, cap = k.csr_from_arcs(n, rows, cols, caps)
    a, b, cab, cba, ref = k.solve(n, ro, ci, cap, 0, 3)
    good = k.by_dinic(n, a, b, cab, cba, 0, 3)["flow"]
    assert k.validate_flow(n, a, b, cab, cba, 0, 3, ref["value"], good) == []
    over = good.copy()
    over[a.tolist().index(1) + 1] += 1  # pair (1, 3): one unit more than its capacity
    assert any("outside" in x for x in k.validate_flow(n, a, b, cab, cba, 0, 3, ref["value"], over))
    leak = good.copy()
    leak[0] -= 1  # pair (0, 1): vertex 1 now sends more than it takes
    assert any("conserved" in x for x in k.validate_flow(n, a, b, cab, cba, 0, 3, ref["value"], leak))
    assert k.validate_flow(n, a, b, cab, cba, 0, 3, ref["value"] + 1, good) != []
    short = ref["side"].copy()
    short[2] = 2  # one vertex on the wrong side: the cut loses the pair (2, 3) and takes (0, 2) and (1, 2) instead
    assert k.cut_capacities(a, b, cab, cba, short) != (ref["value"], ref["value"])
    assert k.cut_capacities(a, b, cab, cba, ref["side"]) == (ref["value"], ref["value"])


def test_arc_flow_rule():
    # 0 -> 1 three times (2, 3, 4) in CSR order and 1 -> 0 once; net flow 0 -> 1 of 6 fills 2, 3 and 1
    ro, ci, cap = k.csr_from_arcs(3, [0, 0, 1, 0, 1, 1], [1, 1, 0, 1, 2, 1], [2, 3, 5, 4, 6, 8])
    a, b, _, _ = k.pairs_of(3, ro, ci, cap)
    assert (a.tolist(), b.tolist()) == ([0, 1], [1, 2])
    assert k.expected_arc_flow(3, ro, ci, cap, a, b, np.array([6, 6])).tolist() == [2, 3, 1, 0, 6, 0]
    assert k.expected_arc_flow(3, ro, ci, cap, a, b, np.array([-4, 0])).tolist() == [0, 0, 0, 4, 0, 0]


@pytest.mark.parametrize("scale", [10, 12, 16])
def test_rmat_literals(scale):
    n, ro, ci, cap, s, t = k.rmat_case(scale)
    a, b, cab, cba, ref = k.solve(n, ro, ci, cap, s, t)
    summary = ref["summary"]
    assert (n, ci.shape[0], s, t, summary["value"], summary["side0"], summary["side1"], summary["side2"]) == RMAT[scale]
    if scale < 16:
        assert k.forms_disagree(n, ro, ci, cap, s, t) == []
    else:
        assert k.same(ref, k.by_dinic(n, a, b, cab, cba, s, t))
