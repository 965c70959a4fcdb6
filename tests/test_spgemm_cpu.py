"""The sparse product without a GPU: the two forms of tests/_spgemm_checker.py against each other, against scipy.sparse (exactly on
non-negative inputs; after eliminate_zeros() on both sides on signed ones, since scipy drops the entries whose products cancel and the
library keeps them as explicit zeros) and against closed forms, so that the GPU tests compare the library with something that has
been checked itself."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import gunrockinst_amd as ga
from gunrockinst_amd import capi
from oracle import gr_oracle as o

import _spgemm_checker as k
from _tc_checker import oriented, simple_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy(m):
    return sp.csr_matrix((k.values_of(m), np.asarray(m[2]), np.asarray(m[1])), shape=m[0], dtype=np.int64)


def _as_scipy(c):
    return sp.csr_matrix((c["vals"], c["cols"], c["offsets"]), shape=c["shape"], dtype=np.int64)


def _agree(a, b):
    d, e = k.dense(a, b), k.expand(a, b)
    assert k.same(d, e) is None, k.same(d, e)
    assert d["offsets"].dtype == np.int32 and d["cols"].dtype == np.int32 and d["vals"].dtype == np.int64
    for i in range(d["shape"][0]):  # strictly ascending rows
        assert np.all(np.diff(d["cols"][d["offsets"][i]:d["offsets"][i + 1]]) > 0)
    return d


def _random(rng, rows, cols, entries, lo, hi, values=True):
    r, c = rng.integers(0, max(rows, 1), entries if rows and cols else 0), rng.integers(0, max(cols, 1), entries if rows and cols else 0)
    return k.from_coo((rows, cols), r, c, rng.integers(lo, hi + 1, len(r)) if values else None)


def _mirrored(n, ro, ci):
    """the simple undirected 0/1 graph of a CSR as a square matrix without values"""
    a, b = simple_edges(n, ro, ci)
    return k.from_coo((n, n), np.concatenate([a, b]), np.concatenate([b, a]))


def _golden(golden_dir, name, undirected=True):
    g = o.build_market(os.path.join(golden_dir, name + ".mtx"), undirected=undirected)
    return k.matrix((g.nodes, g.nodes), g.row_offsets, g.col_indices)


@pytest.mark.parametrize("seed", range(6))
def test_forms_agree_and_match_scipy_on_non_negative_inputs(seed):
    rng = np.random.default_rng(seed)
    rows, inner, cols = (int(x) for x in rng.integers(1, 60, 3))
    a = _random(rng, rows, inner, int(rng.integers(0, 6 * rows)), 0 if seed % 2 else 1, 9, values=seed != 3)  # duplicates, stored zeros
    b = _random(rng, inner, cols, int(rng.integers(0, 6 * inner)), 1, 9, values=seed != 4)
    got = _agree(a, b)
    ref = _scipy(a) @ _scipy(b)
    ref.sort_indices()
    if seed % 2 == 0:  # nothing stored is 0: the structures are the same, entry for entry
        assert np.array_equal(got["offsets"], ref.indptr) and np.array_equal(got["cols"], ref.indices) and np.array_equal(got["vals"], ref.data)
    assert (_as_scipy(got) != ref).nnz == 0


@pytest.mark.parametrize("seed", range(4))
def test_signed_inputs_match_scipy_after_eliminate_zeros(seed):
    rng = np.random.default_rng(100 + seed)
    rows, inner, cols = (int(x) for x in rng.integers(20, 70, 3))
    a, b = _random(rng, rows, inner, 8 * rows, -5, 5), _random(rng, inner, cols, 8 * inner, -5, 5)
    got = _agree(a, b)
    assert np.count_nonzero(got["vals"] == 0) > 0, "the case has no cancelled entry"
    mine, ref = _as_scipy(got), _scipy(a) @ _scipy(b)
    mine.eliminate_zeros()
    ref.eliminate_zeros()
    ref.sort_indices()
    assert np.array_equal(mine.indptr, ref.indptr) and np.array_equal(mine.indices, ref.indices) and np.array_equal(mine.data, ref.data)


def test_cancelled_entries_are_stored():
    a = k.from_coo((1, 2), [0, 0], [0, 1], [1, -1])
    b = k.from_coo((2, 2), [0, 1, 1], [0, 0, 1], [3, 3, 2])
    got = _agree(a, b)
    assert got["offsets"].tolist() == [0, 2] and got["cols"].tolist() == [0, 1] and got["vals"].tolist() == [0, -2]


@pytest.mark.parametrize("name", ["chesapeake", "test_bc"])
def test_goldens(golden_dir, name):
    a = _golden(golden_dir, name)
    n = a[0][0]
    for left, right in ((a, a), (a, k.transpose(a)), (k.crop(a, n // 2 + 1, n), k.crop(a, n, n // 3 + 1))):
        got = _agree(left, right)
        ref = _scipy(left) @ _scipy(right)
        ref.sort_indices()
        assert np.array_equal(got["offsets"], ref.indptr) and np.array_equal(got["cols"], ref.indices) and np.array_equal(got["vals"], ref.data)


def test_transpose_and_shuffle_keep_the_matrix():
    rng = np.random.default_rng(5)
    a = _random(rng, 30, 50, 200, -3, 3)
    assert np.array_equal(k.toarray(k.transpose(a)), k.toarray(a).T) and k.transpose(a)[0] == (50, 30)
    assert np.array_equal(k.toarray(k.shuffled(a, rng)), k.toarray(a))


@pytest.mark.parametrize("n", [1, 2, 5, 17])
def test_complete_graph(n):
    r, c = np.nonzero(1 - np.eye(n, dtype=np.int64))
    got = _agree(*(k.from_coo((n, n), r, c),) * 2)
    sq = _as_scipy(got).toarray()
    assert np.array_equal(np.diag(sq), np.full(n, n - 1)) and np.all(sq[~np.eye(n, dtype=bool)] == n - 2)
    if n > 2:
        assert got["cols"].shape[0] == n * n


def test_path_and_star():
    n = 9
    i = np.arange(n - 1)
    path = k.from_coo((n, n), np.concatenate([i, i + 1]), np.concatenate([i + 1, i]))
    sq = _as_scipy(_agree(path, path)).toarray()
    want = np.zeros((n, n), dtype=np.int64)
    want[np.arange(n), np.arange(n)] = [1] + [2] * (n - 2) + [1]
    want[i[:-1], i[:-1] + 2] = want[i[:-1] + 2, i[:-1]] = 1
    assert np.array_equal(sq, want)
    leaves = np.arange(1, n)
    star = k.from_coo((n, n), np.concatenate([np.zeros(n - 1, dtype=np.int64), leaves]), np.concatenate([leaves, np.zeros(n - 1, dtype=np.int64)]))
    sq = _as_scipy(_agree(star, star)).toarray()
    want = np.ones((n, n), dtype=np.int64)
    want[0, :] = want[:, 0] = 0
    want[0, 0] = n - 1
    assert np.array_equal(sq, want)


@pytest.mark.parametrize("name", ["chesapeake", "test_bc"])
def test_degrees_and_triangles(golden_dir, name):
    g = _golden(golden_dir, name)
    n = g[0][0]
    a = _mirrored(n, g[1], g[2])
    tri, total, deg, _, _ = oriented(n, g[1], g[2])
    aat = _agree(a, k.transpose(a))
    diag = _as_scipy(aat).diagonal()
    assert np.array_equal(diag, deg)
    sq = _agree(a, a)
    cube = k.expand(k.matrix(sq["shape"], sq["offsets"], sq["cols"], sq["vals"]), a)
    assert int(_as_scipy(cube).diagonal().sum()) == 6 * total and np.array_equal(_as_scipy(cube).diagonal(), 2 * tri)


def test_rules():
    # the regime rule at its borders, default and low thresholds, a forced strategy as a floor
    assert [k.regime(w) for w in (0, 64, 65, 512, 513, 4096, 4097)] == [k.LANE, k.LANE, k.WAVE, k.WAVE, k.BLOCK, k.BLOCK, k.GLOBAL]
    low = dict(lane_max=8, table_slots=64, block_slots=256)
    assert [k.regime(w, **low) for w in (0, 1, 8, 9, 32, 33, 128, 129)] == [1, 1, 1, 2, 2, 3, 3, 4]
    for s in (k.WAVE, k.BLOCK, k.GLOBAL):
        assert [k.regime(w, s, **low) for w in (0, 9, 33, 129)] == [max(s, r) for r in (2, 2, 3, 4)]
    assert k.regime(5, k.LANE, **low) == k.LANE and k.regime(9, k.LANE, **low) == k.WAVE
    # twelve bytes a slot with values: the default workgroup table takes 96 KiB
    assert k.lds_bytes(8192, True) == 96 * 1024 and k.lds_bytes(1024, True, k.WAVES) == 48 * 1024 and k.lds_bytes(8192, False) == 32 * 1024
    assert k.slot_words(65) == 67 and k.slot_words(64) == 65 and k.slot_words(1) == 2 and k.slot_words(0) == 0
    assert k.global_slots(1024, 1, 140000) == 1 and k.global_slots(3, 1024, 10) == 3
    assert k.global_slots(1024, 1024, 1 << 20) == 126  # 128 x 64 / 65, rounded down
    # the bound
    a = k.from_coo((2, 2), [0, 0, 1], [0, 1, 1], [-2, 3, 1])
    b = k.from_coo((2, 3), [0, 0, 1], [0, 2, 1], [5, -7, 4])
    assert k.bound(a, b) == 2 * 12 + 3 * 4 and k.work(a, b).tolist() == [3, 1]
    big = k.from_coo((1, 1), [0] * 4, [0] * 4, [-2 ** 31] * 4)
    assert k.bound(big, big) == k.SATURATED  # 4 x (2^31 x 2^33) = 2^66 saturates
    assert k.fits(k.INT_MAX, k.INT_MAX) and not k.fits(k.INT_MAX + 1, 0) and not k.fits(0, k.INT_MAX + 1)


def test_exports():
    names = ("SpgemmProblem", "SpgemmTooLarge", "SpgemmOverflow", "gunrock_spgemm", "gunrock_quotient_graph", "SPGEMM_AUTO", "SPGEMM_LANE",
             "SPGEMM_WAVE", "SPGEMM_BLOCK", "SPGEMM_GLOBAL", "SPGEMM_SELF", "SPGEMM_TRANSPOSE", "SPGEMM_GIVEN", "SPGEMM_TOO_LARGE", "SPGEMM_OVERFLOW")
    for name in names:
        assert name in ga.__all__ and hasattr(ga, name), name
    assert (ga.SPGEMM_AUTO, ga.SPGEMM_LANE, ga.SPGEMM_WAVE, ga.SPGEMM_BLOCK, ga.SPGEMM_GLOBAL) == (0, 1, 2, 3, 4)
    assert (ga.SPGEMM_SELF, ga.SPGEMM_TRANSPOSE, ga.SPGEMM_GIVEN, ga.SPGEMM_TOO_LARGE, ga.SPGEMM_OVERFLOW) == (0, 1, 2, -4, -7)
    assert issubclass(ga.SpgemmTooLarge, ArithmeticError) and issubclass(ga.SpgemmOverflow, ArithmeticError)
    text = open(os.path.join(ROOT, "include", "gunrock", "gunrock_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(grx_spgemm_[a-z0-9_]+)\s*\(", text))
    assert len(declared) == 13 and declared <= set(capi.exported_symbols())
    for method in ("init", "init_device", "set_right", "set_right_device", "set_option", "reset", "enact", "stats", "sizes", "extract",
                   "device_results"):
        assert callable(getattr(ga.SpgemmProblem, method))
