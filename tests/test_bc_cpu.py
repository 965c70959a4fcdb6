"""tests/_bc_checker.py against the oracle, against its own closed forms, and against a float32 simulation of what the GPU
computes -- no GPU needed.  The GPU tests (test_bc_gpu.py) rest on the checker's answer AND on its error bound, so both are pinned
here: the answer equals the oracle's Brandes pass to 1e-12, and the bound is neither vacuous (it stays below 1e-4 on these graphs)
nor too tight (a float32 Brandes with shuffled edge order stays inside it with room to spare)."""
import os

import numpy as np
import pytest

import _bc_checker as k
from oracle import gr_oracle as o


def _simple_graphs(golden, golden_dir):
    f, u = golden["fixture7"], golden["bc_undirected7"]
    yield "fixture7", o.Csr(7, f["row_offsets"], f["col_indices"])
    yield "bc_undirected7", o.Csr(7, u["row_offsets"], u["col_indices"])
    for name in ("test_bc.mtx", "test_cc.mtx", "chesapeake.mtx"):
        yield name, o.build_market(os.path.join(golden_dir, name), undirected=True)
    yield "rmat8 mirrored", o.rmat_seeded(8, 8 << 8)
    yield "rmat8 directed", o.rmat_seeded(8, 8 << 8, undirected=False)
    yield "sinks", o.Csr(4, [0, 1, 3, 3, 3], [1, 2, 3])  # test_directed_graphs_with_sinks


def _same(a, b):
    return np.all(np.abs(a - b) <= 1e-12 * np.abs(b))


def test_brandes_equals_the_oracle_on_simple_graphs(golden, golden_dir):
    for name, g in _simple_graphs(golden, golden_dir):
        deg = np.diff(g.row_offsets)
        for src in sorted({0, int(np.argmax(deg)), g.nodes - 1}):
            ref = k.brandes(g.nodes, g.row_offsets, g.col_indices, src)
            want, want_sigma = o.bc(g, src)
            assert _same(ref.bc, want) and np.array_equal(ref.sigma, want_sigma), (name, src)
            assert np.array_equal(ref.labels, o.bfs(g, src)[0]), (name, src)
        ref = k.brandes_all(g.nodes, g.row_offsets, g.col_indices)
        assert _same(ref.bc, o.bc(g, -1)[0]), name
        assert ref.bound.max() < 1e-4, name


def test_oracle_reads_a_raw_csr_as_a_multigraph():
    """The oracle walks the entries as they are: a parallel entry counts again and a self loop fails its label test, which is the
    checker's reading.  They agree, so the GPU test of this graph could use either; it uses the checker."""
    n, ro, ci = k.messy(np.random.default_rng(5))
    rows = np.repeat(np.arange(n), np.diff(ro))
    assert (rows == ci).sum() >= 40 and len(set(zip(rows.tolist(), ci.tolist()))) < ci.shape[0]  # loops and parallel entries
    g = o.Csr(n, ro, ci)
    for src in (0, int(np.argmax(np.diff(ro))), -1):
        ref = k.brandes_all(n, ro, ci) if src < 0 else k.brandes(n, ro, ci, src)
        assert _same(ref.bc, o.bc(g, src)[0])
    # and it differs from the simple graph underneath: the multigraph reading is not vacuous here
    pairs = np.unique(np.stack([rows, ci])[:, rows != ci], axis=1)
    sn, sro, sci = k.csr_from_edges(n, pairs[0], pairs[1])
    assert not _same(k.brandes(sn, sro, sci, 0).bc, k.brandes(n, ro, ci, 0).bc)
    # a parallel entry is a parallel edge: 0 => 1 (twice) -> 2 has two shortest paths to 1 and to 2
    ref = k.brandes(3, [0, 2, 3, 3], [1, 1, 2], 0)
    assert ref.sigma.tolist() == [1, 2, 2] and ref.bc.tolist() == [0, 0.5, 0]
    # a self loop contributes nothing
    assert k.brandes(3, [0, 2, 4, 4], [0, 1, 1, 2], 0).bc.tolist() == [0, 0.5, 0]


TILE = k.advance_tile()
CLOSED = [("path 0", lambda: k.path(3000, 0)), ("path mid", lambda: k.path(3000, 1500)), ("path end", lambda: k.path(3000, 2999)),
          ("star", lambda: k.star(TILE + 1)), ("broom", lambda: k.broom(5, TILE + 1)), ("cycle even", lambda: k.cycle(1000)),
          ("cycle odd", lambda: k.cycle(1001)), ("tree root", lambda: k.binary_tree(10, 0)), ("tree leaf", lambda: k.binary_tree(10, 2046)),
          ("tree inner", lambda: k.binary_tree(6, 11)), ("diamonds 24", lambda: k.diamond_chain(24)),
          ("diamonds 126", lambda: k.diamond_chain(126)), ("diamonds 130 / 100", lambda: k.diamond_chain(130, 100)),
          ("diamonds 9 / 9", lambda: k.diamond_chain(9, 9))]


@pytest.mark.parametrize("name,build", CLOSED, ids=[c[0] for c in CLOSED])
def test_closed_forms_equal_brandes(name, build):
    n, ro, ci, src, sigma, bc = build()
    assert ro.dtype == ci.dtype == np.int32 and sigma.dtype == bc.dtype == np.float32 and ro[-1] == ci.shape[0]
    ref = k.brandes(n, ro, ci, src)
    assert np.array_equal(sigma.astype(np.float64), ref.sigma) and np.array_equal(bc.astype(np.float64), ref.bc)
    assert k.assert_bc(sigma, bc, ref) == 0.0


def test_tile_is_the_policys():
    assert TILE == 1024  # KernelPolicy<256, 4, ...>: 256 threads x 4 edge slots


def test_float32_brandes_is_bit_exact_on_diamond_chains():
    rng = np.random.default_rng(3)
    for kk in (24, 25, 126, 127):
        n, ro, ci, src, sigma, bc = k.diamond_chain(kk)
        got_sigma, got_bc = k.simulate_f32(n, ro, ci, src, rng)
        assert np.array_equal(got_sigma, sigma) and np.array_equal(got_bc, bc), kk


def _bounded_graphs():
    rng = np.random.default_rng(11)
    n, ro, ci = k.hubby(3000, 9000, 3, rng)
    deg = np.diff(ro)
    for src in (0, int(np.argsort(deg)[n // 2]), int(np.flatnonzero(deg)[-1])):  # a hub, a median-degree vertex, the last one with edges
        yield "hubby %d" % src, n, ro, ci, src
    yield ("grid",) + k.grid(13, 13) + (0,)
    yield ("layered mirrored",) + k.layered(65, 6, True) + (0,)
    yield ("layered directed",) + k.layered(65, 6, False) + (0,)
    yield ("hub in the middle",) + k.hub_in_the_middle(TILE + 1, rng) + (0,)


def test_float32_simulation_stays_inside_the_bound():
    rng = np.random.default_rng(7)
    worst = {}
    for name, n, ro, ci, src in _bounded_graphs():
        ref = k.brandes(n, ro, ci, src)
        nonzero = ref.bc > 0
        assert nonzero.any() and ref.bound[nonzero].max() < 1e-4 and ref.bound[nonzero].min() >= 3 * k.U, name
        got_sigma, got_bc = k.simulate_f32(n, ro, ci, src, rng)
        worst[name] = k.assert_bc(got_sigma, got_bc, ref)  # (asserts 2 x bound, zeros and path counts)
        assert worst[name] <= 1.0, (name, worst[name])  # in fact inside the unscaled bound
    print(worst)
    assert max(worst.values()) > 0.01  # the bound is within two orders of what float32 really does: not vacuous
    # path counts above 2^24 occur (65^5) and the grid's binomials stay below
    assert k.brandes(*k.layered(65, 6, True), 0).sigma.max() == 65.0 ** 5 > 2.0 ** 24
    assert k.brandes(*k.grid(13, 13), 0).sigma.max() == 2704156 < 2.0 ** 24


def test_assert_bc_has_teeth():
    """one dropped, doubled or invented contribution on a low-centrality vertex fails, which 1e-3 relative + 1e-3 absolute let pass"""
    g = o.rmat_seeded(14, 8 << 14)
    src = int(np.argsort(np.diff(g.row_offsets))[g.nodes // 2])  # a median-degree vertex: the hubs are levels away
    ref = k.brandes(g.nodes, g.row_offsets, g.col_indices, src)
    good = ref.bc.astype(np.float32)
    k.assert_bc(ref.sigma.astype(np.float32), good, ref)
    small = int(np.argmin(np.where(ref.bc > 0, ref.bc, np.inf)))
    assert 0 < ref.bc[small] < 1e-3
    zero = int(np.flatnonzero((ref.bc == 0) & (ref.labels > 0))[0])
    for v, value in ((small, 0.0), (small, 2 * good[small]), (zero, 1e-6), (small, np.nan)):
        bad = good.copy()
        bad[v] = value
        assert np.all(np.abs(np.nan_to_num(bad) - ref.bc) <= 1e-3 * ref.bc + 1e-3)  # the old comparison
        with pytest.raises(AssertionError):
            k.assert_bc(None, bad, ref)
    sig = ref.sigma.astype(np.float32)
    sig[small] += 1
    with pytest.raises(AssertionError):
        k.assert_bc(sig, good, ref)
