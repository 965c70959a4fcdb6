"""The tiled closing label pass of BFS (label_pass = 1, DESIGN §3.3 l) against the per-lane kernels it replaces (label_pass = 0)
and against the oracle.  Every comparison is exact.

Labels of the two passes are compared on the same problem, search by search.  Predecessors are checked with check_bfs_preds
for both passes and compared for their unreached (-2) / source (-1) pattern; they are compared value by value where the
search is bottom-up only: there every vertex takes the first visited in-neighbour of its row, whereas the parent a top-down
level records is whichever claim wins, so two searches of one graph may legitimately differ in it.

Kept level bitmaps are frontiers of different levels and never overlap (both passes let the last listed one win if they
did); labels equal to the oracle's in every configuration below is what checks that."""
import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

pytestmark = pytest.mark.gpu

MODES = [(False, False), (True, False), (False, True), (True, True)]


def _csr(n, edges):
    """symmetric CSR from undirected pairs"""
    rows, cols = [], []
    for u, v in edges:
        rows.append(u); cols.append(v)
        if u != v:
            rows.append(v); cols.append(u)
    rows = np.array(rows, np.int64); cols = np.array(cols, np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    ro = np.zeros(n + 1, np.int32)
    if rows.size:
        np.add.at(ro, rows + 1, 1)
    return o.Csr(n, np.cumsum(ro).astype(np.int32), cols.astype(np.int32))


def _problem(g, mark_pred=True, idempotence=True, hubs=None, bottom_up_only=False):
    p = ga.BfsProblem(mark_pred, idempotence).init(g.nodes, g.row_offsets, g.col_indices)
    if hubs is not None:
        p.set_option("relabel_hubs", hubs)
    if bottom_up_only:
        p.set_inverse_graph(alpha=1e12, beta=1e12)
        p.set_tuning(tail_edge_limit=0)
    else:
        p.set_inverse_graph()
    return p


def _run(p, src, label_pass, mode=2):
    p.set_option("label_pass", label_pass)
    p.reset(src)
    p.enact(src, traversal_mode=mode)
    labels, preds = p.extract()
    return labels, preds, p.stats()["search_depth"]


def _check(g, p, src, mode=2, exact_preds=False):
    """label_pass 1 against label_pass 0 on the same problem, both against the oracle"""
    ref, _, _ = o.bfs(g, src)
    new, new_p, new_d = _run(p, src, 1, mode)
    old, old_p, old_d = _run(p, src, 0, mode)
    assert np.array_equal(new, old), "label_pass=1 labels differ from label_pass=0 (src %d)" % src
    assert np.array_equal(new, ref), "labels differ from the oracle (src %d)" % src
    assert new_d == old_d
    if new_p is not None:
        assert o.check_bfs_preds(g, src, new, new_p) == 0, "label_pass=1 predecessors are not valid parents (src %d)" % src
        assert o.check_bfs_preds(g, src, old, old_p) == 0
        assert np.array_equal(np.minimum(new_p, 0), np.minimum(old_p, 0))
        if exact_preds:
            assert np.array_equal(new_p, old_p)
    return new_d


def _sources(g):
    deg = np.diff(g.row_offsets)
    out = {int(np.argmax(deg)), g.nodes - 1, 0}
    edgeless = np.nonzero(deg == 0)[0]
    if edgeless.size:
        out.add(int(edgeless[0]))
        out.add(int(edgeless[-1]))
    with_edges = np.nonzero(deg > 0)[0]
    if with_edges.size:
        out.add(int(with_edges[-1]))
    return sorted(out)


def test_option_is_known_and_flips_between_searches():
    g = o.rmat_seeded(10, 8 << 10)
    p = _problem(g)
    src = int(np.argmax(np.diff(g.row_offsets)))
    ref, _, _ = o.bfs(g, src)
    for relabel in (1, 0):
        p.set_option("relabel", relabel)
        for label_pass in (1, 0, 0, 1, 1):
            assert np.array_equal(_run(p, src, label_pass)[0], ref)
    p.close()


@pytest.mark.parametrize("scale,ef", [(8, 8), (10, 8), (12, 8), (14, 2), (16, 2)])
@pytest.mark.parametrize("mark_pred,idempotence", MODES)
def test_rmat_all_modes_and_hub_tiers(scale, ef, mark_pred, idempotence):
    g = o.rmat_seeded(scale, ef << scale)
    deg = np.diff(g.row_offsets)
    sources = [int(np.argmax(deg)), g.nodes - 1, int(np.nonzero(deg == 0)[0][0]) if (deg == 0).any() else 1]
    for hubs in (0, 1, 64, 65536):   # (two tiers interleaved inside one tile)
        p = _problem(g, mark_pred, idempotence, hubs)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            for src in sources:
                _check(g, p, src)
        p.close()


def _block_graph(prefix, block=300, seed=7):
    """`prefix` edgeless vertices, then a connected block in which every 7th vertex is edgeless too: on the relabelled copy the
    window of the quad at caller vertex v0 starts at bit (v0 - prefix - gaps) & 63"""
    rng = np.random.default_rng(seed + prefix)
    live = [prefix + i for i in range(block) if i % 7 != 3]
    edges = [(live[i], live[i + 1]) for i in range(0, len(live) - 1, 3)]          # (not a path: some links are missing ...)
    edges += [(live[int(a)], live[int(b)]) for a, b in rng.integers(0, len(live), (3 * len(live), 2))]  # ... chords connect it
    return _csr(prefix + block, edges)


@pytest.mark.parametrize("bottom_up_only", [False, True])
def test_windows_at_every_bit_offset(bottom_up_only):
    offsets = set()
    for prefix in range(64):
        g = _block_graph(prefix)
        deg = np.diff(g.row_offsets)
        live = np.nonzero(deg > 0)[0]
        first_of_quad = live[np.r_[True, live[1:] // 4 != live[:-1] // 4]]   # (no hub tier: its new id is its rank among `live`)
        offsets.update((np.searchsorted(live, first_of_quad) & 63).tolist())
        for hubs in (0, 16):
            p = _problem(g, True, True, hubs, bottom_up_only)
            for relabel in (1, 0):
                p.set_option("relabel", relabel)
                for src in (int(live[0]), int(live[-1]), 0, g.nodes - 1):
                    _check(g, p, src, exact_preds=bottom_up_only)
            p.close()
    assert offsets == set(range(64))


@pytest.mark.parametrize("n", [1, 5, 63, 65, 1023, 1025, 4099, 4 * 4096 + 2])
def test_sizes_off_the_quad_the_word_and_the_tile(n):
    g = _csr(n, [(i, (i * 7 + 3) % n) for i in range(0, n, 2)] + [(i, i + 1) for i in range(0, n - 1, 5)])
    for bottom_up_only in (False, True):
        for hubs in (0, 64):
            p = _problem(g, True, True, hubs, bottom_up_only)
            for relabel in (1, 0):
                p.set_option("relabel", relabel)
                for src in _sources(g) + [max(0, n - 2), (n // 4) * 4 if (n // 4) * 4 < n else 0]:   # (the last partial quad)
                    _check(g, p, src, exact_preds=bottom_up_only)
            p.close()


def test_edgeless_graph_and_edgeless_sources():
    empty = o.Csr(200, np.zeros(201, np.int32), np.zeros(0, np.int32))
    for mark_pred, idempotence in MODES:
        p = ga.BfsProblem(mark_pred, idempotence).init(empty.nodes, empty.row_offsets, empty.col_indices)
        p.set_inverse_graph()
        for src in (0, 63, 64, 199):
            for mode in (0, 2):
                _check(empty, p, src, mode)
        p.close()
    g = _csr(1030, [(i, i + 3) for i in range(8, 1000)] + [(8, 500), (9, 10)])   # vertices 0..7 and the last 27 have no edges
    for mark_pred, idempotence in MODES:
        p = _problem(g, mark_pred, idempotence)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            for src in (0, 7, 1003, 1027, 1028, 1029):
                labels = _run(p, src, 1)[0]
                assert labels[src] == 0 and int((labels >= 0).sum()) == 1
                _check(g, p, src)
        p.close()


def test_directed_graph_through_auto_inverse():
    """the never mask is "no in-edge", not "no edge at all": vertices with out-edges only stay -1 unless they are the source"""
    g = o.rmat_seeded(13, 8 << 13, undirected=False)
    outdeg = np.diff(g.row_offsets)
    indeg = np.bincount(g.col_indices, minlength=g.nodes)
    out_only = np.nonzero((outdeg > 0) & (indeg == 0))[0]
    assert out_only.size
    for mark_pred in (False, True):
        p = ga.BfsProblem(mark_pred, True).init(g.nodes, g.row_offsets, g.col_indices)
        enabled, built, _ = p.auto_inverse()
        assert enabled and built
        for src in (int(np.argmax(outdeg)), int(out_only[0]), int(out_only[-1]), g.nodes - 1):
            _check(g, p, src)
        p.close()


@pytest.mark.parametrize("chain_sweeps", [0, 1, 4])
@pytest.mark.parametrize("chain_closing", [0, 1])
@pytest.mark.parametrize("speculative_emit", [0, 1])
def test_every_way_the_pass_is_reached(chain_sweeps, chain_closing, speculative_emit):
    g = o.rmat_seeded(15, 8 << 15)
    deg = np.diff(g.row_offsets)
    sources = [int(np.argmax(deg)), int(np.nonzero(deg == 1)[0][0]), int(np.nonzero(deg == 0)[0][0])]
    for mark_pred in (False, True):
        p = _problem(g, mark_pred, True)
        p.set_option("chain_sweeps", chain_sweeps)
        p.set_option("chain_closing", chain_closing)
        p.set_option("speculative_emit", speculative_emit)
        # (a small persistent edge limit: the closing levels hand back early and the search goes on after a speculative pass)
        for persistent in (1 << 20, 256):
            p.set_persistent_limit(persistent)
            for relabel in (1, 0):
                p.set_option("relabel", relabel)
                for src in sources:
                    _check(g, p, src)
        p.close()


def test_label_deferral_off():
    """no kept bitmaps at all: on the copy the pass translates labels written at discovery (every visited vertex is a gather)"""
    g = o.rmat_seeded(14, 8 << 14)
    for mark_pred, idempotence in MODES:
        p = _problem(g, mark_pred, idempotence, 64)
        p.set_label_deferral(0)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            for src in _sources(g):
                for mode in (0, 1, 2):
                    _check(g, p, src, mode)
        p.close()


def test_mid_search_flush_then_a_full_pass():
    """a path searched bottom-up only through a pool of 4 (and 5, 12) bitmaps: the partial flush runs, then the full pass"""
    n = 3000
    g = _csr(n, [(i, i + 1) for i in range(n - 1)])
    for mask_limit, chain in ((4, 3), (12, 6), (4, 0), (5, 6)):
        p = _problem(g, True, True, bottom_up_only=True)
        p.set_label_deferral(1, mask_limit)
        p.set_option("chain_sweeps", chain)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            before = p.mask_flushes()
            for src in (0, n // 2):
                _check(g, p, src, exact_preds=True)
            assert p.mask_flushes() > before
        p.close()


@pytest.mark.parametrize("chain_sweeps", [0, 4])
def test_ten_kept_levels_in_one_full_pass(chain_sweeps):
    """ten layers behind the source, complete between neighbours, searched bottom-up only with the pool at its full 12: no
    flush happens, so one full pass sees ten kept bitmaps (codes up to 10, the widest list a search produces)"""
    layers, width = 10, 70
    first = lambda k: 1 + (k - 1) * width
    edges = [(0, first(1) + i) for i in range(width)]
    for k in range(1, layers):
        edges += [(first(k) + i, first(k + 1) + j) for i in range(width) for j in range(width) if (i + j) % 3 != 1]
    n = first(layers + 1) + 9   # (a few vertices without edges at the end)
    g = _csr(n, edges)
    ref, _, _ = o.bfs(g, 0)
    assert ref.max() == layers
    for hubs in (0, 64):
        p = _problem(g, True, True, hubs, bottom_up_only=True)
        p.set_label_deferral(1, 12)
        p.set_option("chain_sweeps", chain_sweeps)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            before = p.mask_flushes()
            _check(g, p, 0, exact_preds=True)
            assert p.mask_flushes() == before, "the kept levels were flushed: fewer than ten reached the full pass"
        p.close()


def test_scale24_device_compare():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(24, 8)
    n, m = 1 << 24, int(ci.shape[0])
    src0, _ = devgraph.largest_degree_source(ro)
    deg = ro[1:] - ro[:-1]
    edgeless = int(torch.nonzero(deg == 0)[1000].item())
    sources = [src0] + devgraph.seeded_sources(ro, 1, 0x6772) + [edgeless]
    del deg
    p = ga.BfsProblem(mark_pred=False, idempotence=True)
    p.init_device(n, m, ro.data_ptr(), ci.data_ptr())
    p.set_inverse_graph()
    assert 0 < p.relabel_info()["with_edges"] < n
    labels_t = devgraph.as_tensor(p.device_results()[0], n)
    for relabel in (1, 0):
        p.set_option("relabel", relabel)
        for s in sources:
            out = []
            for label_pass in (1, 0):
                p.set_option("label_pass", label_pass)
                p.reset(s)
                p.enact(s, traversal_mode=2)
                torch.cuda.synchronize()
                out.append((labels_t.clone(), p.stats()["search_depth"]))
            assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
            assert int(out[0][0][s].item()) == 0
            if s == edgeless:
                assert int((out[0][0] >= 0).sum().item()) == 1
    p.close()
