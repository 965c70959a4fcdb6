"""BFS on the relabelled copy (hub-first, edgeless-last renumbering, DESIGN §3.3 k): labels bit-exact against the oracle and
identical with relabel 0 / 1, predecessors valid parents in the caller's numbering, whatever the tier sizes and enactor knobs."""
import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o

pytestmark = pytest.mark.gpu

MODES = [(False, False), (True, False), (False, True), (True, True)]


def _csr(n, edges):
    """symmetric CSR from undirected pairs, entries kept as listed (self-loops and duplicates included)"""
    rows, cols = [], []
    for u, v in edges:
        rows.append(u); cols.append(v)
        if u != v:
            rows.append(v); cols.append(u)
    rows = np.array(rows, np.int64); cols = np.array(cols, np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    ro = np.zeros(n + 1, np.int32)
    np.add.at(ro, rows + 1, 1)
    return o.Csr(n, np.cumsum(ro).astype(np.int32), cols.astype(np.int32))


def _problem(g, mark_pred=True, idempotence=True, hubs=None):
    p = ga.BfsProblem(mark_pred, idempotence).init(g.nodes, g.row_offsets, g.col_indices)
    if hubs is not None:
        p.set_option("relabel_hubs", hubs)
    p.set_inverse_graph()
    return p


def _search(p, src, mode=2, relabel=1):
    p.set_option("relabel", relabel)
    p.reset(src)
    p.enact(src, traversal_mode=mode)
    labels, preds = p.extract()
    return labels, preds, p.stats()["search_depth"]


def _sources(g):
    deg = np.diff(g.row_offsets)
    out = {int(np.argmax(deg)), g.nodes - 1, 0}
    edgeless = np.nonzero(deg == 0)[0]
    if edgeless.size:
        out.add(int(edgeless[0]))
    with_edges = np.nonzero(deg > 0)[0]
    if with_edges.size:
        out.add(int(with_edges[-1]))
        out.add(int(with_edges[with_edges.size // 2]))
    return sorted(out)


def _check_both(g, p, src, mode=2):
    ref, _, _ = o.bfs(g, src)
    l1, p1, d1 = _search(p, src, mode, 1)
    assert np.array_equal(l1, ref), "relabel=1 labels differ from the oracle (src %d, mode %d)" % (src, mode)
    if p1 is not None:
        assert o.check_bfs_preds(g, src, l1, p1) == 0, "relabel=1 predecessors are not valid parents (src %d)" % src
    l0, p0, d0 = _search(p, src, mode, 0)
    assert np.array_equal(l0, ref) and d0 == d1
    if p0 is not None:
        assert o.check_bfs_preds(g, src, l0, p0) == 0


def test_relabel_info_and_option_errors():
    g = o.rmat_seeded(10, 1 << 10)
    p = _problem(g, hubs=16)
    info = p.relabel_info()
    deg = np.diff(g.row_offsets)
    assert 0 < info["hubs"] <= 16 and info["with_edges"] == int((deg > 0).sum())
    assert int((deg >= info["threshold"]).sum()) == info["hubs"] and info["bytes"] > 0
    p.close()
    q = ga.BfsProblem(True, True).init(g.nodes, g.row_offsets, g.col_indices)   # no inverse graph: no copy
    assert q.relabel_info()["hubs"] == -1
    with pytest.raises(RuntimeError):
        q.set_option("relabel", 1)
    q.close()


@pytest.mark.parametrize("mark_pred,idempotence", MODES)
def test_golden_fixture_all_modes(golden, mark_pred, idempotence):
    f = golden["fixture7"]   # (directed: mirrored here, the copy is built for symmetric problems; mirrored pairs come out duplicated)
    ro, ci = f["row_offsets"], f["col_indices"]
    g = _csr(7, [(u, ci[i]) for u in range(7) for i in range(ro[u], ro[u + 1])])
    for hubs in (0, 1, 3, 100):
        p = _problem(g, mark_pred, idempotence, hubs)
        for src in range(7):
            for mode in (0, 1, 2):
                _check_both(g, p, src, mode)
        p.close()


@pytest.mark.parametrize("scale,ef", [(8, 1), (10, 2), (12, 8), (14, 1), (16, 2), (16, 8)])
def test_rmat_scales(scale, ef):
    g = o.rmat_seeded(scale, ef << scale)
    for mark_pred, idempotence in MODES:
        p = _problem(g, mark_pred, idempotence)
        for src in _sources(g):
            for mode in ((0, 1, 2) if mark_pred and idempotence else (2,)):
                _check_both(g, p, src, mode)
        p.close()


def test_mid_search_flush_on_the_copy():
    """mask_limit 4: the kept level bitmaps run out and are flushed into the work labels (FlushLevelMasks) mid-search"""
    g = o.rmat_seeded(16, 8 << 16)
    p = _problem(g, True, True)
    p.set_label_deferral(1, 4)
    flushed_on_copy = 0
    for chain in (0, 4):
        p.set_option("chain_sweeps", chain)
        for src in _sources(g):
            before = p.mask_flushes()
            ref, _, _ = o.bfs(g, src)
            labels, preds, _ = _search(p, src, 2, 1)   # (on the copy)
            assert np.array_equal(labels, ref) and o.check_bfs_preds(g, src, labels, preds) == 0
            flushed_on_copy += p.mask_flushes() - before
            _check_both(g, p, src)
    assert flushed_on_copy > 0
    p.close()


def test_default_uses_the_copy_on_large_graphs_only():
    g = o.rmat_seeded(12, 8 << 12)
    p = _problem(g, True, True)
    src = _sources(g)[0]
    ref, _, _ = o.bfs(g, src)
    p.reset(src)                                  # default relabel = -1: 4096 vertices < relabel_min_nodes
    p.enact(src, traversal_mode=2)
    labels, preds = p.extract()
    assert np.array_equal(labels, ref) and o.check_bfs_preds(g, src, labels, preds) == 0
    p.set_option("relabel", -1)
    p.set_option("relabel_min_nodes", 1)          # the same rule, now on: the copy is searched
    p.reset(src)
    p.enact(src, traversal_mode=2)
    labels, preds = p.extract()
    assert np.array_equal(labels, ref) and o.check_bfs_preds(g, src, labels, preds) == 0
    p.close()


@pytest.mark.parametrize("hubs", [0, 1, 64, 65536, 1 << 20])
def test_hub_sizes_and_knobs(hubs):
    g = o.rmat_seeded(13, 4 << 13)
    src = _sources(g)
    p = _problem(g, True, True, hubs)
    info = p.relabel_info()
    assert info["hubs"] <= hubs
    if hubs > 0:   # ids on either side of the tier boundary (the last hub and the first non-hub, in the caller's order)
        deg = np.diff(g.row_offsets)
        hub_ids = np.nonzero(deg >= info["threshold"])[0]
        rest = np.nonzero((deg > 0) & (deg < info["threshold"]))[0]
        src += [int(x) for x in (hub_ids[-1:].tolist() + rest[:1].tolist())]
    for chain in (0, 4):
        p.set_option("chain_sweeps", chain)
        for defer, limit in ((1, 12), (0, 12), (1, 4)):
            p.set_label_deferral(defer, limit)
            for s in src:
                _check_both(g, p, s)
    p.set_label_deferral(1, 12)
    p.set_head_pass(1, 0)           # heads pass on every eligible level
    p.set_binned_min_edges(1)       # every top-down level binned
    for s in src[:3]:
        _check_both(g, p, s)
    p.close()


def _special_graphs():
    star = _csr(33, [(0, i) for i in range(1, 33)])
    path = _csr(50, [(i, i + 1) for i in range(49)])
    full = _csr(65, [(i, (i + 1) % 65) for i in range(65)] + [(0, 32)])          # no vertex without edges
    empty = o.Csr(40, np.zeros(41, np.int32), np.zeros(0, np.int32))             # every vertex without edges
    loops = _csr(10, [(0, 1), (1, 1), (1, 2), (1, 2), (3, 3), (4, 5), (5, 4)])  # a self-loop, duplicates, a loop-only vertex
    one = o.Csr(1, np.zeros(2, np.int32), np.zeros(0, np.int32))
    sizes = [_csr(n, [(i, (i * 7 + 3) % n) for i in range(0, n, 2)]) for n in (63, 65, 127)]
    return [star, path, full, empty, loops, one] + sizes


@pytest.mark.parametrize("k", range(9))
def test_special_graphs(k):
    g = _special_graphs()[k]
    for mark_pred, idempotence in MODES:
        for hubs in (0, 1, 64):
            p = _problem(g, mark_pred, idempotence, hubs)
            for src in _sources(g):
                for mode in (0, 2):
                    _check_both(g, p, src, mode)
            p.close()


def test_toggle_keeps_device_pointers():
    import torch
    from gunrockinst_amd import devgraph
    g = o.rmat_seeded(12, 8 << 12)
    p = _problem(g, True, True)
    dl, dp = p.device_results()
    labels_t = devgraph.as_tensor(dl, g.nodes)
    preds_t = devgraph.as_tensor(dp, g.nodes)
    for k, relabel in enumerate((1, 0, 1, 1, 0)):
        src = _sources(g)[k % len(_sources(g))]
        p.set_option("relabel", relabel)
        p.reset(src)
        p.enact(src, traversal_mode=2 if k != 3 else 0)
        torch.cuda.synchronize()
        assert p.device_results() == (dl, dp)
        labels = labels_t.cpu().numpy()
        ref, _, _ = o.bfs(g, src)
        assert np.array_equal(labels, ref)
        preds = preds_t.cpu().numpy()
        assert o.check_bfs_preds(g, src, labels, preds) == 0
        assert preds[ref == -1].tolist() == [-2] * int((ref == -1).sum())
    p.close()


def test_scale24_device_compare():
    import torch
    from gunrockinst_amd import devgraph
    ro, ci = devgraph.rmat_csr_device(24, 8)
    n, m = 1 << 24, int(ci.shape[0])
    src0, _ = devgraph.largest_degree_source(ro)
    sources = [src0] + devgraph.seeded_sources(ro, 4, 0x6772)
    p = ga.BfsProblem(mark_pred=False, idempotence=True)
    p.init_device(n, m, ro.data_ptr(), ci.data_ptr())
    p.set_inverse_graph()
    assert 0 < p.relabel_info()["with_edges"] < n      # (the copy exists; default hub tier: empty)
    labels_t = devgraph.as_tensor(p.device_results()[0], n)
    for s in sources:
        out = []
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            p.reset(s)
            p.enact(s, traversal_mode=2)
            torch.cuda.synchronize()
            out.append((labels_t.clone(), p.stats()["search_depth"]))
        assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    p.close()
