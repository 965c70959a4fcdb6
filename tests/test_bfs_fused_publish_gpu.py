"""The closing read-back of BFS published by the tiled label pass (fused_publish = 1, DESIGN §3.3 o) against the publishing
kernel behind the pass (fused_publish = 0) and against the oracle.  Every comparison is exact.

Each check runs the same search with both settings on one handle: labels equal to each other and to the oracle, predecessors
valid parents (check_bfs_preds) with the same unreached (-2) / source (-1) pattern, `total_queued` and `search_depth` equal,
and the handle's stream idle right after every enact -- Enact returns only when the label pass behind its last read-back has
finished, whichever way the search ended.  `fused_publications` (read-backs a label pass published, over the handle's life)
says whether the path was taken: it never moves with fused_publish = 0, and the cases that are built to reach the path assert
that it does with 1.

The overflow case overflows the queue a top-down level writes right before the search turns bottom-up: that queue is never
read (the bitmap of the level comes from the visited-bitmap difference), the flag stays set and the search still ends through
the sweeps, the closing levels and the publishing label pass, which must report it.  It does not overflow the queue a chained
sweep emits: consumers of an overflowed queue read past its allocation."""
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


def _problem(g, mark_pred=True, idempotence=True, **inverse):
    p = ga.BfsProblem(mark_pred, idempotence).init(g.nodes, g.row_offsets, g.col_indices)
    p.set_inverse_graph(**inverse)
    p.set_option("relabel_min_nodes", 1)
    return p


LAST = {}   # of the last _run: elapsed milliseconds of its enact, publications its label passes carried


def _run(p, src, fused, mode=2):
    p.set_option("fused_publish", fused)
    before = p.fused_publications()
    p.reset(src)
    LAST["ms"] = p.enact(src, traversal_mode=mode)
    assert p.stream_idle(), "Enact returned with work still on its stream (fused_publish=%d, src %d)" % (fused, src)
    LAST["carried"] = p.fused_publications() - before
    assert fused or LAST["carried"] == 0, "fused_publish=0 and a label pass published all the same (src %d)" % src
    labels, preds = p.extract()
    s = p.stats()
    return labels, preds, (s["total_queued"], s["search_depth"])


_REFS = {}


def _ref(g, src):
    key = (id(g), src)
    if key not in _REFS:
        _REFS[key] = (g, o.bfs(g, src)[0])   # (the graph is kept so that its id stays its own)
    return _REFS[key][1]


def _check(g, p, src, mode=2, carried=None):
    """fused_publish 1 against 0 on the same problem, both against the oracle; carried: publications the passes of the
    fused_publish=1 search must have carried at least (0: exactly none)"""
    ref = _ref(g, src) if 0 <= src < g.nodes else np.full(g.nodes, -1, np.int32)
    new, new_p, new_s = _run(p, src, 1, mode)
    if carried is not None:
        assert LAST["carried"] >= carried and (carried > 0 or LAST["carried"] == 0), \
            "label passes carried %d publications, expected %s%d (src %d)" % (LAST["carried"], ">= " if carried else "", carried, src)
    old, old_p, old_s = _run(p, src, 0, mode)
    assert np.array_equal(new, old), "fused_publish=1 labels differ from fused_publish=0 (src %d)" % src
    assert np.array_equal(new, ref), "labels differ from the oracle (src %d)" % src
    assert new_s == old_s, "statistics differ (src %d): %r, %r" % (src, new_s, old_s)
    if new_p is not None and 0 <= src < g.nodes:
        assert o.check_bfs_preds(g, src, new, new_p) == 0, "fused_publish=1 predecessors are not valid parents (src %d)" % src
        assert o.check_bfs_preds(g, src, old, old_p) == 0
        assert np.array_equal(np.minimum(new_p, 0), np.minimum(old_p, 0))
    return new_s


def _sources(g):
    deg = np.diff(g.row_offsets)
    out = {int(np.argmax(deg)), g.nodes - 1, 0}
    edgeless = np.nonzero(deg == 0)[0]
    if edgeless.size:
        out.add(int(edgeless[0]))
    return sorted(out)


@pytest.fixture(scope="module")
def rmat13():
    return o.rmat_seeded(13, 8 << 13)


@pytest.mark.parametrize("chain_sweeps", [0, 4])
@pytest.mark.parametrize("chain_closing", [0, 1])
@pytest.mark.parametrize("speculative_emit", [0, 1])
def test_every_way_the_pass_is_reached(rmat13, chain_sweeps, chain_closing, speculative_emit):
    g = rmat13
    deg = np.diff(g.row_offsets)
    sources = [int(np.argmax(deg)), int(np.nonzero(deg == 1)[0][0]), int(np.nonzero(deg == 0)[0][0])]
    for mark_pred in (False, True):
        p = _problem(g, mark_pred, True)
        p.set_option("chain_sweeps", chain_sweeps)
        p.set_option("chain_closing", chain_closing)
        p.set_option("speculative_emit", speculative_emit)
        # the hub's search turns bottom-up; with chains and the closing levels behind them a gated pass is queued behind every
        # chain, and it carries the chain's read-back.  Without the speculative pass nothing is ever handed over.
        hub_carries = 1 if (speculative_emit and chain_closing and chain_sweeps) else None
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            for src in sources:
                _check(g, p, src, carried=0 if not speculative_emit else (hub_carries if src == sources[0] else None))
        p.close()


@pytest.mark.parametrize("chain_sweeps", [0, 4])
def test_the_closing_launch_hands_its_read_back_over(rmat13, chain_sweeps):
    """beta 4: the search returns to top-down as soon as a sweep finds fewer than a quarter of the vertices; without closing
    levels behind the chain that is the host's closing launch (RunTail), whose speculative pass carries its read-back"""
    g = rmat13
    src = int(np.argmax(np.diff(g.row_offsets)))
    for mark_pred in (False, True):
        p = _problem(g, mark_pred, True, beta=4.0)
        p.set_option("chain_sweeps", chain_sweeps)
        p.set_option("chain_closing", 0)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            _check(g, p, src, carried=1)
        p.close()


def test_a_gate_that_says_do_not_run(rmat13):
    """no sweep emits its finds as a queue (emit_queue_factor 0), so the closing levels and the label pass queued behind every
    chain exit at their gate: the pass publishes all the same, and the search goes on with read-backs of the publishing kernel
    (the bitmap -> queue conversion, then the closing launch and its pass), their sequence numbers in step"""
    g = rmat13
    for mark_pred in (False, True):
        p = _problem(g, mark_pred, True)
        p.set_option("emit_queue_factor", 0)
        for label_pass in (1, 0):   # (0: the per-lane kernels never publish)
            p.set_option("label_pass", label_pass)
            for relabel in (1, 0):
                p.set_option("relabel", relabel)
                hub = int(np.argmax(np.diff(g.row_offsets)))
                for src in _sources(g):
                    _check(g, p, src, carried=0 if not label_pass else (1 if src == hub else None))
        p.close()


def test_a_search_that_goes_on_after_a_pass_that_ran():
    """a path of 7600 vertices hung on a complete core of 64: the sweeps find the core, the closing levels walk the path until
    their level limit (4096) and hand back, the pass behind them has run and published; the search goes on (one more sweep,
    closing levels, a second pass that covers the rest), so the completion event is recorded a second time.  An event left
    behind the first pass would end the timed interval there, with 3500 of the 7600 levels still to run: the elapsed time of
    the search must not fall below 3/4 of what it takes with fused_publish=0 (the same kernels but two 5 us launches of a
    search of several milliseconds; the stale event would leave 4100 / 7600 = 0.54 of it).  Best of three each."""
    core, tail = 64, 7600
    edges = [(i, j) for i in range(core) for j in range(i + 1, core)]
    edges += [(core - 1 + i, core + i) for i in range(tail)]
    g = _csr(core + tail, edges)
    assert _ref(g, 0).max() == tail + 1
    p = _problem(g, True, True, alpha=1e12)
    p.set_tuning(tail_edge_limit=0)
    p.set_option("sparse_sweep_div", 1)
    for relabel in (1, 0):
        p.set_option("relabel", relabel)
        total_queued, depth = _check(g, p, 0, carried=2)
        assert depth >= tail
        ms = {}
        for fused in (1, 0):
            ms[fused] = min((_run(p, 0, fused), LAST["ms"])[1] for _ in range(3))
        print("elapsed ms, fused_publish 1 / 0: %.3f / %.3f" % (ms[1], ms[0]))
        assert ms[1] >= 0.75 * ms[0], "the timed interval ends before the search does: %.3f ms against %.3f" % (ms[1], ms[0])
    p.close()


def test_mid_search_flush():
    """a path searched bottom-up only through a pool of 4 bitmaps: partial flushes (which never publish) between chains whose
    gated pass publishes and exits, then the full pass of FinishSearch behind the last read-back"""
    n = 1000
    g = _csr(n, [(i, i + 1) for i in range(n - 1)])
    for chain in (3, 0):
        p = _problem(g, True, True, alpha=1e12, beta=1e12)
        p.set_tuning(tail_edge_limit=0)
        p.set_label_deferral(1, 4)
        p.set_option("chain_sweeps", chain)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            before = p.mask_flushes()
            for src in (0, n // 2):
                _check(g, p, src)
            assert p.mask_flushes() > before
        p.close()


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_sizes(n):
    """block 0 of the pass is the only block, a partial tile, one of several"""
    g = _csr(n, [(i, (i * 7 + 3) % n) for i in range(0, n, 2)] + [(i, i + 1) for i in range(0, n - 1, 5)])
    for mark_pred in (False, True):
        p = _problem(g, mark_pred, True)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            for src in _sources(g) + [n // 2]:
                _check(g, p, src)
        p.close()


def test_edgeless_graph_edgeless_source_and_source_out_of_range():
    empty = o.Csr(200, np.zeros(201, np.int32), np.zeros(0, np.int32))
    for mark_pred, idempotence in MODES:
        p = ga.BfsProblem(mark_pred, idempotence).init(empty.nodes, empty.row_offsets, empty.col_indices)
        p.set_inverse_graph()
        for src in (0, 64, 199, -1, 200):
            for mode in (0, 2):
                _check(empty, p, src, mode)
        p.close()
    g = _csr(1030, [(i, i + 3) for i in range(8, 1000)] + [(8, 500), (9, 10)])   # vertices 0..7 and the last 27 have no edges
    for mark_pred, idempotence in MODES:
        p = _problem(g, mark_pred, idempotence)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            for src in (0, 7, 1003, 1029, -1, 1030, 1 << 30):
                labels = _run(p, src, 1)[0]
                assert int((labels >= 0).sum()) == (1 if 0 <= src < g.nodes else 0)
                _check(g, p, src)
        p.close()


def test_overflow_is_still_reported():
    """queues of 1024 entries (queue_sizing at its floor); the level behind the hub holds more and is written top-down
    (lite_factor 0: no count-only level; tail_edge_limit 0: no tail kernel), then the search turns bottom-up and ends through
    the label pass.  Both settings must report the overflow, and leave the stream idle; with room in the queues neither does."""
    g = o.rmat_seeded(14, 8 << 14)
    deg = np.diff(g.row_offsets)
    src = int(np.argmax(deg))
    ref = _ref(g, src)
    levels = np.bincount(ref[ref >= 0])
    # what makes this safe and what makes it overflow: level 1 does not fit, no later queue holds more than a level that does,
    # and the frontier behind level 1 is heavy enough for the direction rule (alpha = 10), so nobody reads the overflowed queue
    assert levels[1] > 1024 and levels[3:].max() < 1024 and levels.size > 3
    assert float(deg[ref == 1].sum()) * 10.0 > g.edges - int(deg[src])
    assert g.edges > 8 * g.nodes    # (not a low-degree graph: no TWC / persistent levels in front of the direction rule)
    for fused in (1, 0):
        for queue_sizing, overflows in ((1e-9, True), (1.0, False)):
            p = _problem(g, False, True)     # (a fresh handle: queues never shrink)
            p.set_tuning(lite_factor=0.0, tail_edge_limit=0)
            p.set_option("fused_publish", fused)
            p.reset(src, queue_sizing)
            if overflows:
                with pytest.raises(RuntimeError):
                    p.enact(src, traversal_mode=2)
            else:
                p.enact(src, traversal_mode=2)
                assert np.array_equal(p.extract()[0], ref)
            assert p.stream_idle()
            p.close()


def test_option_flipped_between_searches_and_two_handles_alternating(rmat13):
    g = rmat13
    src = int(np.argmax(np.diff(g.row_offsets)))
    ref = _ref(g, src)
    a, b = _problem(g), _problem(g, False, True)
    for relabel in (1, 0):
        a.set_option("relabel", relabel)
        b.set_option("relabel", relabel)
        seen = []
        for fa, fb in ((1, 0), (0, 1), (0, 0), (1, 1), (1, 0)):
            la, _, sa = _run(a, src, fa)
            lb, _, sb = _run(b, g.nodes - 1, fb)
            assert np.array_equal(la, ref) and np.array_equal(lb, _ref(g, g.nodes - 1))
            seen.append((sa, sb))
        assert all(s == seen[0] for s in seen)
    a.close()
    b.close()


@pytest.mark.parametrize("mark_pred,idempotence", MODES)
def test_random_rmat_graphs(mark_pred, idempotence):
    """30 seeded R-MAT graphs of scale 10-12"""
    for k in range(30):
        scale = 10 + k % 3
        g = o.rmat_seeded(scale, 8 << scale, seed=0x6772 + 977 * k)
        deg = np.diff(g.row_offsets)
        rng = np.random.default_rng(k)
        p = _problem(g, mark_pred, idempotence)
        p.set_option("relabel", k & 1)
        for src in (int(np.argmax(deg)), int(rng.integers(0, g.nodes))):
            _check(g, p, src)
        p.close()
    _REFS.clear()
