"""The bipartite checker (tests/_bipartite_checker.py) against scipy and networkx, the theorem the feature rests on -- parts, cover
and blocks are the same from two different maximum matchings --, literals with answers written by hand, and the exported names.
No GPU."""
import os
import re

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import maximum_bipartite_matching, structural_rank

import gunrockinst_amd as ga
from gunrockinst_amd import capi

import _bipartite_checker as k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LITERAL = [(0, 0), (0, 1), (0, 2), (1, 2), (1, 3), (1, 4), (2, 2), (2, 3), (3, 4), (4, 4)]


def literal(drop=None):
    pairs = [p for p in LITERAL if p != drop]
    return k.from_pairs((5, 5), [p[0] for p in pairs], [p[1] for p in pairs])


def scipy_matrix(matrix):
    (rows, cols), ro, ci = matrix
    a = sp.csr_matrix((np.ones(len(ci), np.int8), ci.copy(), ro.copy()), shape=(rows, cols))  # (sum_duplicates works in place)
    a.sum_duplicates()
    return a


def other_matching(matrix, seed):
    """scipy's maximum matching of a row- and column-permuted copy, mapped back: (mate_row, mate_col)"""
    (rows, cols), ro, ci = matrix
    rng = np.random.default_rng(seed)
    pr, pc = rng.permutation(rows), rng.permutation(cols)  # new index of every row / column
    r = np.repeat(np.arange(rows), np.diff(ro))
    permuted = k.from_pairs((rows, cols), pr[r], pc[ci]) if len(ci) else matrix
    mate_of_new_row = maximum_bipartite_matching(scipy_matrix(permuted), perm_type="column") if rows and cols else np.full(rows, -1)
    inv_c = np.argsort(pc)
    mate_row = np.full(rows, -1, np.int32)
    mate_col = np.full(cols, -1, np.int32)
    for old in range(rows):
        c = int(mate_of_new_row[pr[old]])
        if c >= 0:
            mate_row[old] = inv_c[c]
            mate_col[inv_c[c]] = old
    return mate_row, mate_col


def random_pattern(rng):
    rows, cols = int(rng.integers(0, 41)), int(rng.integers(0, 41))
    count = int(rng.integers(0, 3 * max(rows, cols) + 1)) if rows and cols else 0
    return k.from_pairs((rows, cols), rng.integers(0, max(rows, 1), count), rng.integers(0, max(cols, 1), count))


def check_against_references(matrix, seed, networkx_cover=True):
    (rows, cols), ro, ci = matrix
    mine = k.decompose(matrix)
    a = scipy_matrix(matrix)
    if rows and cols:
        assert mine["size"] == structural_rank(a)
        assert mine["size"] == int((maximum_bipartite_matching(a, perm_type="column") >= 0).sum())
    else:
        assert mine["size"] == 0
    # networkx: the cardinality always; to_vertex_cover, which is quadratic, on the small inputs only
    g = nx.Graph()
    top = [("r", r) for r in range(rows)]
    g.add_nodes_from(top, bipartite=0)
    g.add_nodes_from((("c", c) for c in range(cols)), bipartite=1)
    g.add_edges_from((("r", int(r)), ("c", int(c))) for r, c in zip(np.repeat(np.arange(rows), np.diff(ro)), ci))
    m = nx.bipartite.hopcroft_karp_matching(g, top_nodes=top)
    assert len(m) == 2 * mine["size"]
    if networkx_cover:
        assert len(nx.bipartite.to_vertex_cover(g, m, top_nodes=top)) == mine["size"]
    # König: the cover covers, and is as large as the matching
    r = np.repeat(np.arange(rows), np.diff(ro))
    assert np.all(mine["row_cover"][r].astype(bool) | mine["col_cover"][ci].astype(bool))
    assert int(mine["row_cover"].sum()) + int(mine["col_cover"].sum()) == mine["size"]
    # the theorem: everything but the matching itself is the same from another maximum matching
    theirs = k.decompose(matrix, other_matching(matrix, seed))
    assert theirs["size"] == mine["size"]
    for name in ("row_part", "col_part", "row_cover", "col_cover", "row_block", "col_block"):
        assert np.array_equal(mine[name], theirs[name]), name
    assert mine["part_sizes"] == theirs["part_sizes"] and mine["blocks"] == theirs["blocks"]
    return mine


def test_random_patterns():
    rng = np.random.default_rng(606)
    seen_parts = set()
    for case in range(150):
        got = check_against_references(random_pattern(rng), case)
        seen_parts |= {i for i, s in enumerate(got["part_sizes"]) if s}
    assert seen_parts == set(range(6))


@pytest.fixture(scope="module")
def bips(golden_dir):
    return k.read_pattern(os.path.join(golden_dir, "bips98_606.mtx"))


def test_chesapeake(golden_dir):
    m = k.read_pattern(os.path.join(golden_dir, "chesapeake.mtx"))
    assert m[0] == (39, 39) and len(m[2]) == 340
    got = check_against_references(m, 1)
    assert got["size"] == 39 and got["blocks"] == 1 and got["part_sizes"] == [0, 39, 0, 0, 39, 0]


def test_bips98_606(bips):
    assert bips[0] == (7135, 7135) and len(bips[2]) == 34738
    got = check_against_references(bips, 2, networkx_cover=False)  # (to_vertex_cover takes minutes here)
    assert got["size"] == 7135 and got["blocks"] == 1299 and got["part_sizes"] == [0, 7135, 0, 0, 7135, 0]


@pytest.mark.parametrize("cut", ["rows", "cols"])
def test_bips98_606_slices(bips, cut):
    m = k.take_rows(bips, 5000) if cut == "rows" else k.take_cols(bips, 5000)
    got = check_against_references(m, 3, networkx_cover=False)
    # the wide slice has a horizontal and a square part, the tall one a square and a vertical part: all three between them
    assert got["size"] == 5000
    assert got["part_sizes"] == ([3874, 1126, 0, 6009, 1126, 0] if cut == "rows" else [0, 832, 6303, 0, 832, 4168])
    assert got["blocks"] == (1122 if cut == "rows" else 779)


def test_literal():
    m = literal()
    got = check_against_references(m, 4)
    assert got["size"] == 4
    assert got["row_part"].tolist() == [0, 1, 1, 2, 2] and got["col_part"].tolist() == [0, 0, 1, 1, 2]
    assert got["row_cover"].tolist() == [1, 1, 1, 0, 0] and got["col_cover"].tolist() == [0, 0, 0, 0, 1]
    assert got["part_sizes"] == [1, 2, 2, 2, 2, 1]
    assert got["blocks"] == 1 and got["row_block"].tolist() == [-1, 1, 1, -1, -1] and got["col_block"].tolist() == [-1, -1, 1, 1, -1]
    split = check_against_references(literal(drop=(2, 2)), 5)
    assert split["size"] == 4 and split["row_part"].tolist() == [0, 1, 1, 2, 2] and split["col_part"].tolist() == [0, 0, 1, 1, 2]
    assert split["blocks"] == 2 and split["row_block"].tolist() == [-1, 1, 2, -1, -1] and split["col_block"].tolist() == [-1, -1, 1, 2, -1]


def test_more_literals():
    # nothing at all; no entries; one entry; a full column and a full row
    assert k.decompose(((0, 0), np.zeros(1, np.int32), np.zeros(0, np.int32)))["size"] == 0
    empty = k.decompose(k.from_pairs((2, 3), [], []))
    assert empty["size"] == 0 and empty["row_part"].tolist() == [2, 2] and empty["col_part"].tolist() == [0, 0, 0] and empty["blocks"] == 0
    assert empty["row_cover"].tolist() == [0, 0] and empty["col_cover"].tolist() == [0, 0, 0]
    one = k.decompose(k.from_pairs((1, 1), [0], [0]))
    assert one["size"] == 1 and one["row_part"].tolist() == [1] and one["row_block"].tolist() == [0] and one["col_block"].tolist() == [0]
    tall = k.decompose(k.from_pairs((3, 1), [0, 1, 2], [0, 0, 0]))
    assert tall["size"] == 1 and tall["row_part"].tolist() == [2, 2, 2] and tall["col_part"].tolist() == [2] and tall["col_cover"].tolist() == [1]
    wide = k.decompose(k.from_pairs((1, 3), [0, 0, 0], [0, 1, 2]))
    assert wide["size"] == 1 and wide["row_part"].tolist() == [0] and wide["col_part"].tolist() == [0, 0, 0] and wide["row_cover"].tolist() == [1]
    # a 2 x 2 triangle: rows 0 -> {0, 1}, 1 -> {1}: two blocks, upper triangular
    tri = k.decompose(k.from_pairs((2, 2), [0, 0, 1], [0, 1, 1]))
    assert tri["size"] == 2 and tri["blocks"] == 2 and tri["row_block"].tolist() == [0, 1] and tri["col_block"].tolist() == [0, 1]
    # the chain with its forced start: one augmenting path of 2 k + 1 edges
    kk = 6
    chain = k.from_pairs((kk + 1, kk + 1), list(range(kk + 1)) + list(range(kk)), list(range(kk + 1)) + list(range(1, kk + 1)))
    start = np.array(list(range(1, kk + 1)) + [-1], np.int32)
    mate_col = np.full(kk + 1, -1, np.int32)
    mate_col[start[:kk]] = np.arange(kk)
    assert k.validate(chain, start, mate_col) == kk
    assert k.decompose(chain)["size"] == kk + 1


def test_validate_refuses():
    m = literal()
    mr, mc = k.hopcroft_karp(m)
    bad = mr.copy()
    bad[3], bad[4] = 4, 4  # a column twice
    with pytest.raises(AssertionError):
        k.validate(m, bad, mc)
    no_entry_r, no_entry_c = np.full(5, -1, np.int32), np.full(5, -1, np.int32)
    no_entry_r[4], no_entry_c[0] = 0, 4  # (4, 0) is no entry
    with pytest.raises(AssertionError):
        k.validate(m, no_entry_r, no_entry_c)
    with pytest.raises(AssertionError):  # not maximum: the parts notice
        k.parts(m, np.full(5, -1, np.int32), np.full(5, -1, np.int32))


def test_exports():
    names = ("BipartiteProblem", "BipartiteNotCertified", "BipartiteNotMaximum", "gunrock_bipartite_matching", "gunrock_structural_rank",
             "gunrock_vertex_cover", "gunrock_dulmage_mendelsohn", "BIPARTITE_AUTO", "BIPARTITE_LANE", "BIPARTITE_WAVE", "BIPARTITE_BLOCK",
             "BIPARTITE_HORIZONTAL", "BIPARTITE_SQUARE", "BIPARTITE_VERTICAL", "BIPARTITE_MAXIMUM", "BIPARTITE_CAPPED", "BIPARTITE_NOT_CERTIFIED",
             "BIPARTITE_BAD_MATCHING", "BIPARTITE_NOT_MAXIMUM", "BIPARTITE_SCHEDULE_AUTO", "BIPARTITE_ROUNDS", "BIPARTITE_DEVICE_LOOP")
    for name in names:
        assert name in ga.__all__ and hasattr(ga, name), name
    assert (ga.BIPARTITE_AUTO, ga.BIPARTITE_LANE, ga.BIPARTITE_WAVE, ga.BIPARTITE_BLOCK) == (0, 1, 2, 3)
    assert (ga.BIPARTITE_HORIZONTAL, ga.BIPARTITE_SQUARE, ga.BIPARTITE_VERTICAL) == (0, 1, 2) == (k.HORIZONTAL, k.SQUARE, k.VERTICAL)
    assert (ga.BIPARTITE_MAXIMUM, ga.BIPARTITE_CAPPED) == (0, 1)
    assert (ga.BIPARTITE_NOT_CERTIFIED, ga.BIPARTITE_BAD_MATCHING, ga.BIPARTITE_NOT_MAXIMUM) == (-4, -5, -6)
    assert (ga.BIPARTITE_SCHEDULE_AUTO, ga.BIPARTITE_ROUNDS, ga.BIPARTITE_DEVICE_LOOP) == (0, 1, 2)
    assert issubclass(ga.BipartiteNotCertified, RuntimeError) and issubclass(ga.BipartiteNotMaximum, RuntimeError)
    assert not hasattr(capi, "BipartiteProblem")  # the class lives in gunrockinst_amd.bipartite; capi.py only binds the symbols
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_bipartite_[a-z0-9_]+)\s*\(", text))
    assert len(declared) == 14 and declared <= set(capi.exported_symbols())
    for value, name in ((0, "GRX_BIPARTITE_HORIZONTAL"), (1, "GRX_BIPARTITE_SQUARE"), (2, "GRX_BIPARTITE_VERTICAL"), (-4, "GRX_BIPARTITE_NOT_CERTIFIED"),
                        (-5, "GRX_BIPARTITE_BAD_MATCHING"), (-6, "GRX_BIPARTITE_NOT_MAXIMUM")):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    for method in ("init", "init_device", "set_option", "reset", "enact", "stats", "phase_trace", "extract_matching", "extract_parts",
                   "extract_cover", "square_graph", "blocks", "device_results"):
        assert callable(getattr(ga.BipartiteProblem, method))
