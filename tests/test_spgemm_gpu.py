"""The sparse product on the GPU (grx_spgemm_*): `offsets`, `cols` and `vals` must equal tests/_spgemm_checker.py's forms with
np.array_equal, dtype included; none of them may move under anything that is not the two matrices: the regime, the thresholds, the
scratch budget, the grid, the order inside the rows of A and of B, host or device init.  Which regime took a row is asserted from
stats against the checker's restatement of the rule."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import gunrockinst_amd as ga
from oracle import gr_oracle as o

import _spgemm_checker as k

pytestmark = pytest.mark.gpu

STRATEGIES = (ga.SPGEMM_AUTO, ga.SPGEMM_LANE, ga.SPGEMM_WAVE, ga.SPGEMM_BLOCK, ga.SPGEMM_GLOBAL)
LOW = {"lane_max": 8, "table_slots": 64, "block_slots": 256}  # the borders at w = 8, 32 and 128
DEFAULTS = {"strategy": ga.SPGEMM_AUTO, "pattern_only": 0, "lane_max": 64, "table_slots": 1024, "block_slots": 8192, "scratch_mib": 1024,
            "count_limit": 2.0 ** 62}
RULE = ("strategy", "lane_max", "table_slots", "block_slots")


def _set(p, options):
    for key, value in {**DEFAULTS, **options}.items():
        assert p.set_option(key, value) == 0, key


def _problem(a, b=None, transpose=False, **kw):
    p = ga.SpgemmProblem(**kw).init(a[0], a[1], a[2], a[3])
    if b is not None:
        assert p.set_right(b[0], b[1], b[2], b[3]) == 0
    elif transpose:
        assert p.set_option("right", ga.SPGEMM_TRANSPOSE) == 0
    return p


def _run(p, grid=0, **options):
    _set(p, options)
    p.enact(grid)
    got = p.extract(values=not options.get("pattern_only"))
    assert got["offsets"].dtype == np.int32 and got["cols"].dtype == np.int32
    assert p.sizes() == (got["shape"][0], got["shape"][1], got["cols"].shape[0])
    return got, p.stats()


def _check(got, st, a, b, ref=None, **options):
    ref = k.dense(a, b) if ref is None else ref
    assert k.same(got, ref, values=not options.get("pattern_only")) is None, (k.same(got, ref), options)
    want = k.regime_stats(a, b, **{key: value for key, value in options.items() if key in RULE})
    assert {key: st[key] for key in want} == want, (st, options)
    assert st["products"] == int(k.work(a, b).sum()) and st["nnz"] == ref["cols"].shape[0] and st["readbacks"] == (3 if a[0][0] else 0)
    assert st["bound"] == float(k.bound(a, b))


def _golden(golden_dir, name):
    g = o.build_market(os.path.join(golden_dir, name + ".mtx"), undirected=name != "bips98_606")
    m = k.matrix((g.nodes, g.nodes), g.row_offsets, g.col_indices)
    return (m[0], m[1].astype(np.int32), m[2].astype(np.int32), None)


def _random(rng, rows, cols, entries, lo=-4, hi=4, values=True):
    r, c = rng.integers(0, rows, entries), rng.integers(0, cols, entries)
    return k.from_coo((rows, cols), r, c, rng.integers(lo, hi + 1, entries) if values else None)


# ---------------- goldens ----------------

@pytest.mark.parametrize("name", ["chesapeake", "test_bc", "bips98_606"])
def test_goldens(golden_dir, name):
    a = _golden(golden_dir, name)
    n = a[0][0]
    small = n < 1000
    form = k.dense if small else k.expand
    # A^2 and A A^T on one handle
    p = _problem(a)
    got, st = _run(p)
    _check(got, st, a, a, form(a, a))
    assert p.set_option("right", ga.SPGEMM_TRANSPOSE) == 0
    at = k.transpose(a)
    ref = form(a, at)
    got, st = _run(p)
    _check(got, st, a, at, ref)
    got, st = _run(p, **LOW)  # (the transpose is kept: the same again under low thresholds)
    _check(got, st, a, at, ref, **LOW)
    p.close()
    # a rectangular product: the top rows of A times its left columns
    left, right = k.crop(a, n // 2 + 1, n), k.crop(a, n, n // 3 + 1)
    p = _problem(left, right)
    got, st = _run(p)
    _check(got, st, left, right, form(left, right))
    assert got["shape"] == (n // 2 + 1, n // 3 + 1)
    p.close()
    scipy_ref = sp.csr_matrix((np.ones(len(a[2]), dtype=np.int64), a[2], a[1]), shape=a[0])
    scipy_ref = scipy_ref @ scipy_ref.T
    scipy_ref.sort_indices()
    assert np.array_equal(ref["offsets"], scipy_ref.indptr) and np.array_equal(ref["vals"], scipy_ref.data)


def test_one_shot_forms(golden_dir):
    a = _golden(golden_dir, "chesapeake")
    ref = k.dense(a, a)
    assert k.same(ga.gunrock_spgemm((a[1], a[2])), ref) is None
    assert k.same(ga.gunrock_spgemm((a[0], a[1], a[2])), ref) is None
    assert k.same(ga.gunrock_spgemm((a[1], a[2]), transpose_right=True), k.dense(a, k.transpose(a))) is None
    got = ga.gunrock_spgemm((a[1], a[2]), pattern_only=True)
    assert got["vals"] is None and k.same(got, ref, values=False) is None
    rng = np.random.default_rng(3)
    left, right = _random(rng, 1, 7, 5), _random(rng, 7, 4, 12)
    assert k.same(ga.gunrock_spgemm(left, right), k.dense(left, right)) is None
    assert k.same(ga.gunrock_spgemm(left[:3], right[:3]), k.dense(left[:3] + (None,), right[:3] + (None,))) is None
    got = ga.gunrock_spgemm(([0, 1], [0], [5]))  # (offsets, cols, vals) of one row: two offsets are no shape
    assert got["shape"] == (1, 1) and got["offsets"].tolist() == [0, 1] and got["cols"].tolist() == [0] and got["vals"].tolist() == [25]


# ---------------- the borders of the regimes ----------------

WIDTHS = (0, 1, 8, 9, 32, 33, 128, 129, 3000)


def _border_case(values, rng):
    """row 2 t: one entry of A onto a row of B with WIDTHS[t] distinct columns (nnz = w); row 2 t + 1: WIDTHS[t] entries of A onto
    rows of B that hold column 7 alone (nnz = 1, the value w without values)"""
    top, units = len(WIDTHS), max(WIDTHS)
    ar, ac, br, bc = [], [], [], []
    for t, w in enumerate(WIDTHS):
        ar.append(np.full(1, 2 * t))
        ac.append(np.full(1, t))
        br.append(np.full(w, t))
        bc.append(rng.permutation(units)[:w])
        ar.append(np.full(w, 2 * t + 1))
        ac.append(top + rng.permutation(units)[:w])
    br.append(top + np.arange(units))
    bc.append(np.full(units, 7))
    ar, ac, br, bc = (np.concatenate(x) for x in (ar, ac, br, bc))
    a = k.from_coo((2 * top, top + units), ar, ac, rng.integers(-3, 4, len(ar)) if values else None)
    b = k.from_coo((top + units, units), br, bc, rng.integers(-3, 4, len(br)) if values else None)
    return a, b


@pytest.mark.parametrize("values", [False, True])
def test_borders(values):
    a, b = _border_case(values, np.random.default_rng(11))
    assert k.work(a, b).tolist() == [w for w in WIDTHS for _ in range(2)]
    ref = k.expand(a, b)
    assert np.diff(ref["offsets"]).tolist() == [x for w in WIDTHS for x in (w, min(w, 1))]
    if not values:
        assert ref["vals"][ref["offsets"][1::2][np.asarray(WIDTHS) > 0]].tolist() == [w for w in WIDTHS if w]
    p = _problem(a, b)
    got, st = _run(p, **LOW)
    _check(got, st, a, b, ref, **LOW)
    assert [st[name + "_rows"] for name in k.REGIMES] == [6, 4, 4, 4]
    for strategy in STRATEGIES:
        for grid in (0, 1):
            got, st = _run(p, grid, strategy=strategy, **LOW)
            _check(got, st, a, b, ref, strategy=strategy, **LOW)
    got, st = _run(p)  # the defaults: 3000 products are a workgroup's
    _check(got, st, a, b, ref)
    assert st["block_rows"] == 2 and st["global_rows"] == 0
    p.close()


# ---------------- invariance ----------------

def test_invariance(golden_dir):
    rng = np.random.default_rng(21)
    a = _golden(golden_dir, "chesapeake")
    a = (a[0], a[1], a[2], rng.integers(-3, 4, len(a[2])).astype(np.int32))
    b = _random(rng, a[0][1], 65, 400)
    ref = k.dense(a, b)
    runs = [dict(strategy=s, **low) for s in STRATEGIES for low in ({}, LOW)]
    runs += [dict(scratch_mib=1, strategy=ga.SPGEMM_GLOBAL), dict(scratch_mib=1, **LOW)]
    p = _problem(a, b, instrument=True)
    for options in runs:
        for grid in (0, 1, 3):
            got, st = _run(p, grid, **options)
            _check(got, st, a, b, ref, **options)
            assert st["kernel_launches"] >= 3 and st["kernel_ms"] > 0
    p.close()
    # the order inside the rows of A and of B
    for seed in range(3):
        sa, sb = k.shuffled(a, np.random.default_rng(seed)), k.shuffled(b, np.random.default_rng(seed + 9))
        p = _problem(sa, sb)
        got, st = _run(p, **LOW)
        _check(got, st, sa, sb, ref, **LOW)
        p.close()


def test_scratch_of_one_slot():
    """140 000 columns: a slot is more than the 1 MiB of scratch_mib = 1, so the GLOBAL regime runs one workgroup"""
    rng = np.random.default_rng(22)
    cols = 140000
    assert k.global_slots(1024, 1, cols) == 1
    a, b = _random(rng, 40, 30, 300), _random(rng, 30, cols, 2000)
    ref = k.expand(a, b)
    p = _problem(a, b)
    for options in (dict(scratch_mib=1, strategy=ga.SPGEMM_GLOBAL), dict(strategy=ga.SPGEMM_GLOBAL), dict(pattern_only=1, scratch_mib=1, strategy=ga.SPGEMM_GLOBAL)):
        got, st = _run(p, **options)
        _check(got, st, a, b, ref, **options)
        assert st["global_rows"] == 40
    p.close()


def test_host_and_device_init():
    import torch
    rng = np.random.default_rng(23)
    a, b = _random(rng, 70, 90, 600), _random(rng, 90, 50, 700)
    ref = k.dense(a, b)
    dev = [[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in m[1:]] for m in (a, b)]
    p = ga.SpgemmProblem().init_device(a[0], len(a[2]), *[t.data_ptr() for t in dev[0]])
    assert p.set_right_device(b[0], len(b[2]), *[t.data_ptr() for t in dev[1]]) == 0
    got, st = _run(p, **LOW)
    _check(got, st, a, b, ref, **LOW)
    d = p.device_results()
    assert all(d[name] for name in ("offsets", "cols", "vals"))
    p.close()
    p = ga.SpgemmProblem().init_device(a[0], len(a[2]), *[t.data_ptr() for t in dev[0][:2]])  # no values: 1 each
    assert p.set_option("right", ga.SPGEMM_TRANSPOSE) == 0
    plain = (a[0], a[1], a[2], None)
    got, st = _run(p)
    _check(got, st, plain, k.transpose(plain))
    p.close()


# ---------------- contents ----------------

def test_duplicates_cancellation_and_absent_values():
    rng = np.random.default_rng(31)
    a, b = _random(rng, 60, 20, 900, -2, 2), _random(rng, 20, 25, 600, -2, 2)  # 900 entries in 1200 places: duplicates
    ref = k.dense(a, b)
    assert np.count_nonzero(ref["vals"] == 0) > 0 and k.same(ref, k.expand(a, b)) is None
    for left, right in ((a, b), ((a[0], a[1], a[2], None), b), (a, (b[0], b[1], b[2], None)), ((a[0], a[1], a[2], None), (b[0], b[1], b[2], None))):
        want = k.dense(left, right)
        p = _problem(left, right)
        for options in ({}, LOW, dict(strategy=ga.SPGEMM_GLOBAL)):
            got, st = _run(p, **options)
            _check(got, st, left, right, want, **options)
            pattern, st = _run(p, pattern_only=1, **options)
            assert pattern["vals"] is None and np.array_equal(pattern["offsets"], got["offsets"]) and np.array_equal(pattern["cols"], got["cols"])
            with pytest.raises(RuntimeError, match="code -1"):
                p.extract(values=True)
        p.close()
    mine = sp.csr_matrix((ref["vals"], ref["cols"], ref["offsets"]), shape=ref["shape"])
    theirs = sp.csr_matrix((k.values_of(a), a[2], a[1]), shape=a[0]) @ sp.csr_matrix((k.values_of(b), b[2], b[1]), shape=b[0])
    mine.eliminate_zeros()
    theirs.eliminate_zeros()
    theirs.sort_indices()
    assert np.array_equal(mine.indptr, theirs.indptr) and np.array_equal(mine.indices, theirs.indices) and np.array_equal(mine.data, theirs.data)


def test_large_values_stay_exact():
    """the largest products the default count_limit admits, and the smallest it refuses: (-2^31)^2 = 2^62"""
    big = 2 ** 31 - 1
    a = k.from_coo((2, 2), [0, 1], [0, 1], [big, -big - 1])
    b = k.from_coo((2, 1), [0, 1], [0, 0], [big, big])
    ref = k.dense(a, b)
    assert ref["vals"].tolist() == [big * big, -(big + 1) * big] and k.bound(a, b) == (big + 1) * big < 2 ** 62
    for options in ({}, dict(strategy=ga.SPGEMM_WAVE), dict(strategy=ga.SPGEMM_BLOCK), dict(strategy=ga.SPGEMM_GLOBAL)):
        p = _problem(a, b)
        got, st = _run(p, **options)
        _check(got, st, a, b, ref, **options)
        p.close()
    a = k.from_coo((1, 1), [0], [0], [-big - 1])
    assert k.bound(a, a) == 2 ** 62
    p = _problem(a)
    with pytest.raises(ga.SpgemmOverflow):
        p.enact()
    p.close()


# ---------------- degenerate shapes ----------------

@pytest.mark.parametrize("strategy", [ga.SPGEMM_AUTO, ga.SPGEMM_WAVE, ga.SPGEMM_GLOBAL])
def test_degenerate_shapes(strategy):
    rng = np.random.default_rng(41)
    empty = np.zeros(0, dtype=np.int32)
    cases = [
        (((0, 5), np.zeros(1, dtype=np.int32), empty, None), _random(rng, 5, 4, 9)),                      # rows = 0
        (((6, 5), np.zeros(7, dtype=np.int32), empty, None), _random(rng, 5, 4, 9)),                      # nnz(A) = 0
        (_random(rng, 6, 5, 12), ((5, 4), np.zeros(6, dtype=np.int32), empty, None)),                     # an all-empty B
        (_random(rng, 9, 1, 6), _random(rng, 1, 8, 5)),                                                   # inner = 1
        (_random(rng, 9, 7, 30), _random(rng, 7, 1, 5)),                                                  # cols = 1
        (_random(rng, 20, 12, 150), _random(rng, 12, 65, 500)),                                           # cols = 65: a partial last word
        (_random(rng, 5, 0 + 3, 0), _random(rng, 3, 0 + 2, 0)),                                           # nothing stored anywhere
    ]
    for a, b in cases:
        p = _problem(a, b)
        got, st = _run(p, strategy=strategy, **LOW)
        _check(got, st, a, b, strategy=strategy, **LOW)
        assert got["shape"] == (a[0][0], b[0][1]) and got["offsets"].shape[0] == a[0][0] + 1
        p.close()


# ---------------- refusals ----------------

def test_overflow_refusal_and_recovery():
    rng = np.random.default_rng(51)
    a, b = _random(rng, 30, 30, 200, 1, 9), _random(rng, 30, 30, 200, 1, 9)
    limit = k.bound(a, b)
    p = _problem(a, b)
    _set(p, dict(count_limit=limit))
    with pytest.raises(ga.SpgemmOverflow):
        p.enact()
    assert p.stats()["bound"] == float(limit) and p.stats()["nnz"] == 0
    with pytest.raises(RuntimeError, match="code 600"):  # hipErrorNotReady: no result
        p.sizes()
    got, st = _run(p, count_limit=limit + 1)
    _check(got, st, a, b)
    got, st = _run(p)
    _check(got, st, a, b)
    p.close()


def test_shape_refusals():
    rng = np.random.default_rng(52)
    a = _random(rng, 6, 9, 20)
    p = _problem(a)
    with pytest.raises(RuntimeError, match="code -1"):  # SELF on a non-square A
        p.enact()
    assert p.set_option("right", ga.SPGEMM_GIVEN) == 0
    with pytest.raises(RuntimeError, match="code -1"):  # GIVEN without a right operand
        p.enact()
    wrong = _random(rng, 8, 4, 10)
    assert p.set_right(wrong[0], wrong[1], wrong[2], wrong[3]) == -1  # B's rows are not A's inner
    bad = _random(rng, 9, 4, 10)
    assert p.set_right(bad[0], bad[1], np.where(bad[2] == bad[2].max(), 4, bad[2]), bad[3]) == -2  # a column outside B
    b = _random(rng, 9, 4, 10)
    assert p.set_right(b[0], b[1], b[2], b[3]) == 0
    got, st = _run(p)
    _check(got, st, a, b)
    assert p.set_option("right", ga.SPGEMM_TRANSPOSE) == 0  # the handle takes every right operand in turn
    got, st = _run(p)
    _check(got, st, a, k.transpose(a))
    p.close()
    with pytest.raises(RuntimeError, match="code -2"):
        ga.SpgemmProblem().init((2, 2), [0, 3, 2], [0, 1], None)
    assert ga.SpgemmProblem().set_option("lane_max", 64) == 0
    with pytest.raises(RuntimeError, match="code -1"):
        ga.SpgemmProblem().set_option("lane_max", 65)


# ---------------- the quotient graph ----------------

def test_quotient_graph(golden_dir):
    g = o.build_market(os.path.join(golden_dir, "chesapeake.mtx"), undirected=True)
    n, ro, ci = g.nodes, np.asarray(g.row_offsets), np.asarray(g.col_indices)
    w = ((np.repeat(np.arange(n), np.diff(ro)) + ci) % 7 + 1).astype(np.int32)
    community = ga.gunrock_label_propagation(n, ro, ci, w)[1]
    random_map = np.random.default_rng(61).integers(0, 11, n).astype(np.int32)
    random_map[:11] = np.arange(11)  # onto 0 .. 10
    for labels in (community, random_map):
        c = int(labels.max()) + 1
        for weights in (w, None):
            got = ga.gunrock_quotient_graph(ro, ci, weights, labels)
            a = sp.csr_matrix((np.ones(len(ci), dtype=np.int64) if weights is None else weights.astype(np.int64), ci, ro), shape=(n, n))
            proj = sp.csr_matrix((np.ones(n, dtype=np.int64), (np.arange(n), labels)), shape=(n, c))
            ref = (proj.T @ a @ proj).tocsr()
            ref.sum_duplicates()
            ref.sort_indices()
            assert got["shape"] == (c, c) and got["vals"].dtype == np.int64
            assert np.array_equal(got["offsets"], ref.indptr) and np.array_equal(got["cols"], ref.indices) and np.array_equal(got["vals"], ref.data)
            assert int(got["vals"].sum()) == (len(ci) if weights is None else int(w.sum()))
