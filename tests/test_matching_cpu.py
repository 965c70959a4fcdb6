"""The heavy-edge matching checker (tests/_matching_checker.py) against itself, without a GPU: the sequential greedy pass, the
mutual-best rounds form and the vectorised verify agree, networkx validates, the two contraction forms agree, and the literals the
GPU tests rely on are pinned."""
import os

import numpy as np
import pytest

from oracle import gr_oracle as o

import _matching_checker as k

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (graph, weighted by (row + col) % 7 + 1, seed): (M, matched pairs, total weight, rounds of the rounds form)
LITERALS = {
    ("chesapeake", False, 0): (170, 15, 15, 4),
    ("chesapeake", False, 1): (170, 18, 18, 3),
    ("chesapeake", True, 0): (170, 18, 108, 3),
    ("chesapeake", True, 1): (170, 16, 96, 3),
    ("bips98_606", False, 0): (15190, 2829, 2829, 5),
    ("bips98_606", False, 1): (15190, 2851, 2851, 5),
    ("bips98_606", True, 0): (15190, 2864, 15762, 6),
    ("bips98_606", True, 1): (15190, 2862, 15759, 5),
    ("test_bc", False, 0): (13, 3, 3, 2),
    ("rmat12", False, 1): (27791, 825, 825, 7),
}


def _graph(name):
    if name == "rmat12":
        g = o.rmat_seeded(12, 8 << 12)
    else:
        g = o.build_market(os.path.join(GOLDEN, name + ".mtx"), undirected=True)
    return g.nodes, g.row_offsets, g.col_indices


@pytest.mark.parametrize("case", sorted(LITERALS))
def test_three_forms_agree_and_literals(case):
    name, weighted, seed = case
    n, ro, ci = _graph(name)
    w = k.mod7_weights(n, ro, ci) if weighted else None
    a, b, pw, ref, count = k.solve(n, ro, ci, w, seed)  # (greedy == rounds, verify passes)
    s = ref["summary"]
    assert (s["pairs"], s["matched"], s["weight"], count) == LITERALS[case]
    assert s["unmatched"] == n - 2 * s["matched"]
    k.networkx_validate(n, a, b, pw, ref)
    for vw in (None, np.arange(n) % 5 - 1):
        dense, sparse = k.contract(n, a, b, pw, ref["mate"], vw), k.contract_sparse(n, a, b, pw, ref["mate"], vw)
        assert k.same_coarse(dense, sparse)
        cmap, nc, cro, cci, cw, vweight = dense
        assert nc == n - s["matched"] and int(vweight.sum()) == (n if vw is None else int(vw.sum()))
        assert cro[-1] == cci.shape[0] and cci.shape[0] % 2 == 0
        # a next level reads the coarse graph back unchanged: both copies of a pair carry its weight
        a2, b2, w2 = k.pairs_of(nc, cro, cci, cw)
        assert a2.shape[0] * 2 == cci.shape[0] and int(w2.astype(np.int64).sum()) * 2 == int(cw.astype(np.int64).sum())


def test_verify_catches_a_wrong_matching():
    n, ro, ci = _graph("chesapeake")
    a, b, pw, ref, _ = k.solve(n, ro, ci, None, 0)
    worse = ref["in_matching"].copy()
    worse[np.flatnonzero(worse)[0]] = 0  # valid, consistent with nothing
    assert k.verify(n, a, b, pw, 0, worse, ref["mate"], ref["medge"])
    assert k.verify(n, a, b, pw, 1, ref["in_matching"], ref["mate"], ref["medge"])  # another seed: another matching
    mate = ref["mate"].copy()
    mate[0] = -1 if mate[0] >= 0 else 1
    assert "mate" in k.verify(n, a, b, pw, 0, ref["in_matching"], mate, ref["medge"])


def test_keys_are_what_the_package_helper_computes():
    import gunrockinst_amd as ga
    w = np.array([1, -1, 0, -(2 ** 31), 2 ** 31 - 1, 7, 7], np.int32)
    for seed in (0, 1, 12345):
        key = k.keys_of(w, seed)
        assert key.dtype == np.uint64 and np.array_equal(key, ga.matching_keys(w, seed))
        assert np.unique(key).shape[0] == w.shape[0]
        order = np.argsort(key)
        assert w[order].tolist() == sorted(w.tolist()), "heavier is larger, negative weights included"


def test_path_of_four_by_hand():
    ro, ci, w = k.path(4, [1, 2, 1])
    a, b, pw, ref, count = k.solve(4, ro, ci, w, 0)
    assert pw.tolist() == [1, 2, 1] and ref["mate"].tolist() == [-1, 2, 1, -1] and ref["medge"].tolist() == [-1, 1, 1, -1] and count == 1
    assert ref["summary"] == {"pairs": 3, "matched": 1, "weight": 2, "unmatched": 2, "unmatched_with_neighbours": 2}


def test_the_weight_of_a_pair_is_its_largest_entry():
    # 0 -> 1 twice (3, 9), 1 -> 0 once (5), 1 -> 2 (-4), a self-loop with a huge weight
    ro, ci, w = np.array([0, 3, 5, 5], np.int32), np.array([1, 1, 0, 0, 2], np.int32), np.array([3, 9, 2 ** 31 - 1, 5, -4], np.int32)
    a, b, pw = k.pairs_of(3, ro, ci, w)
    assert (a.tolist(), b.tolist(), pw.tolist()) == ([0, 1], [1, 2], [9, -4])


def test_monotone_path_needs_a_round_per_pair():
    ro, ci, w = k.path(2001, np.arange(2000) + 1)
    _, _, _, ref, count = k.solve(2001, ro, ci, w, 0)
    assert (ref["summary"]["matched"], count) == (1000, 1000) and ref["mate"][0] == -1 and ref["mate"][2000] == 1999


def test_hashed_path():
    ro, ci, _ = k.path(2001)
    _, _, _, ref, count = k.solve(2001, ro, ci, None, 0)
    assert (ref["summary"]["matched"], count) == (860, 3)


def test_contraction_overflow():
    # the triangle's two heavy pairs fall on one coarse pair when 0 and 1 are matched: 2^30 + 2^30 > 2^31 - 1
    ro, ci, w = k.csr_from_pairs(3, [0, 0, 1], [1, 2, 2], [2 ** 31 - 1, 2 ** 30, 2 ** 30])
    a, b, pw, ref, _ = k.solve(3, ro, ci, w, 0)
    assert ref["mate"].tolist() == [1, 0, -1]
    for form in (k.contract, k.contract_sparse):
        with pytest.raises(k.Overflow):
            form(3, a, b, pw, ref["mate"])
        with pytest.raises(k.Overflow):  # vertex weights overflow too
            form(3, a, b, np.array([1, 1, 1], np.int32), ref["mate"], np.array([2 ** 31 - 1, 1, 0]))
    ok = k.contract(3, a, b, np.array([1, 2 ** 30, 2 ** 30 - 1], np.int32), ref["mate"])
    assert ok[1] == 2 and ok[4].tolist() == [2 ** 31 - 1, 2 ** 31 - 1] and ok[5].tolist() == [2, 1]
