"""The hub slice of the dense bottom-up sweeps (option hub_slice, DESIGN §3.3 n): probes of ids below S are answered from an LDS
copy of the frontier bitmap's first ceil(S / 32) words, all others from global memory.  Every comparison is exact: labels against
oracle.bfs and against the same problem run with hub_slice = 0; predecessors with check_bfs_preds, and value by value against
hub_slice = 0 where the search is forced bottom-up (both give a vertex its first head in the frontier, else the first
in-frontier entry of its row).

"Boundary" graphs put the level-1 frontier on eight consecutive ids f .. f+7 that straddle a 32-bit word of the bitmap
(f = 316: the word ends at 319), and every vertex of level 2 has exactly one of them as its only in-frontier neighbour.  Every
vertex has edges, so the relabelled copy with an empty hub tier keeps the caller's ids, and with S = f+4 the ids S-1, S and S+1
are each the only way to find some vertex.  Ids, in order: two decoy hubs (everybody's adjacency heads, found at level 3), low
fillers, the frontier, high fillers, leaves, the source, then the rows under test:
  walkers   [hub, hub, pos-2 low fillers, frontier vertex, 0..3 high fillers]: both heads miss, the row walk finds the frontier
            vertex at row position `pos` (the last entry when no high filler follows)
  first     [frontier vertex]                      the first head
  pair      [frontier vertex, leaf]                the first head of a two-entry row
  flagged   [hub, frontier vertex]                 the second head of a two-entry row (stored flagged: HeadIsLast)
  second    [hub, frontier vertex, leaf]           the second head of a longer row
  closed    [hub, hub]                             a flagged head that misses: no walk, found through the hubs later

A second family has the frontier on ids 380 .. 387, across the 128-id boundary 384: the fill copies 16 bytes at a time, so an LDS
word past ceil(S / 32) is missing only where that count is a multiple of four (S = 384), and one word short shows at S = 385 .. 388.

Mutations of HubSliceLookup / SliceFill, each built in a scratch copy of this tree and run against the whole file:
  boundary test `x <= slice`                         test_boundary_at_a_four_word_boundary[3] and [256], nothing else
  fill one word short                                23 tests; first test_option_is_known_and_flips_between_searches, every test_boundary_rows
  LDS word index taken from the unselected address   48 tests; the same first ones
  selection inverted for the second head only        48 tests; the same first ones
`x + 1 < slice` changes no result and no test can see it: id S-1 then goes to global memory, which is always right."""
import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o
from test_bfs_walk_queue_gpu import _csr_pairs, _degree_sequence_graph

pytestmark = pytest.mark.gpu

MODES = [(False, False), (True, False), (False, True), (True, True)]
POSITIONS = [2, 3, 8, 9, 34, 35, 256]
F = 316                 # first frontier id: f .. f+7 = 316 .. 323, the 32-bit word boundary is 320
N_FRONT = 8
N_HIGH = 3
N_WALKERS = 72          # nine per frontier vertex, in two 64-vertex words
SLICES = [1, 31, 32, 33, 63, 64, 65, 100, F - 1, F, F + 1, F + 3, F + 4, F + 5, F + 7, F + 8, F + 9, 352]
# the fill copies 16 bytes at a time, so a word past ceil(S / 32) is missing from LDS only where that count is a multiple of four:
# a second family of boundary graphs has its frontier on ids 380 .. 387, across the 128-id boundary 384 (LDS word 12)
F4 = 380
SLICES4 = [F4 - 1, F4, F4 + 1, F4 + 3, F4 + 4, F4 + 5, F4 + 6, F4 + 7, F4 + 8, F4 + 9, 416, 100]
CAP = 4096 * 32         # ids the LDS array holds (bottom_up.hpp kHubSliceWords)


class Boundary:
    def __init__(self, pos, first=F):
        assert 2 <= pos <= first
        self.hubs = (0, 1)
        self.low = 2
        self.front = first
        self.high = first + N_FRONT
        nxt = self.high + N_HIGH
        u, v = [], []

        def row(w, entries):
            e = np.asarray(entries, np.int64)
            u.append(np.full(e.size, w, np.int64)); v.append(e)

        def fresh(count):
            nonlocal nxt
            ids = list(range(nxt, nxt + count))
            nxt += count
            return ids

        self.src = fresh(1)[0]
        row(self.src, range(self.front, self.front + N_FRONT))
        for f in range(self.low, self.front):       # every low filler hangs off both hubs: it has edges, the hubs stay the largest
            row(f, self.hubs)
        for f in range(self.high, self.high + N_HIGH):
            row(f, [self.hubs[0]])
        self.walkers = fresh(N_WALKERS)
        for k, w in enumerate(self.walkers):
            trail = 0 if k % 3 == 0 else k % (N_HIGH + 1)     # (0: the frontier vertex is the row's last entry)
            row(w, list(self.hubs) + list(range(self.low, self.low + pos - 2)) + [self.front + k % N_FRONT] +
                list(range(self.high, self.high + trail)))
        self.first, self.pair, self.flagged, self.second = fresh(N_FRONT), fresh(N_FRONT), fresh(N_FRONT), fresh(N_FRONT)
        for k in range(N_FRONT):
            fk = self.front + k
            row(self.first[k], [fk])
            row(self.pair[k], [fk] + fresh(1))
            row(self.flagged[k], [self.hubs[0], fk])
            row(self.second[k], [self.hubs[0], fk] + fresh(1))
        self.closed = fresh(1)[0]
        row(self.closed, self.hubs)
        self.nodes = nxt + 5                          # (a vertex count off 64; the last five have no edges)
        self.g = _csr_pairs(self.nodes, np.concatenate(u), np.concatenate(v))
        self.with_edges = nxt


_GRAPHS = {}


def _boundary(pos, first=F):
    if (pos, first) not in _GRAPHS:
        b = Boundary(pos, first)
        b.ref = o.bfs(b.g, b.src)[0]
        _GRAPHS[(pos, first)] = b
    return _GRAPHS[(pos, first)]


def _problem(g, mark_pred=True, idempotence=True, forced=True, hubs=0):
    p = ga.BfsProblem(mark_pred, idempotence).init(g.nodes, g.row_offsets, g.col_indices)
    p.set_option("relabel_hubs", hubs)
    if forced:   # every level bottom-up
        p.set_inverse_graph(alpha=1e12, beta=1e12)
        p.set_tuning(tail_edge_limit=0)
    else:
        p.set_inverse_graph()
    p.set_option("relabel_min_nodes", 1)
    p.set_option("relabel", 1)                        # small graphs: the copy is searched
    return p


def _run(p, src, hub_slice, grid=0):
    p.set_option("hub_slice", hub_slice)
    p.reset(src)
    p.enact(src, max_grid_size=grid, traversal_mode=2)
    return p.extract()


def _check(g, p, src, ref, slices, grid=0, exact_preds=True):
    old, old_p = _run(p, src, 0, grid)
    assert np.array_equal(old, ref), "hub_slice=0 labels differ from the oracle (src %d, grid %d)" % (src, grid)
    if old_p is not None:
        assert o.check_bfs_preds(g, src, old, old_p) == 0
    for s in slices:
        new, new_p = _run(p, src, s, grid)
        assert np.array_equal(new, ref), "hub_slice=%d labels differ from the oracle (src %d, grid %d)" % (s, src, grid)
        assert np.array_equal(new, old), "hub_slice=%d labels differ from hub_slice=0 (src %d, grid %d)" % (s, src, grid)
        if new_p is not None:
            assert o.check_bfs_preds(g, src, new, new_p) == 0, "hub_slice=%d predecessors are not valid parents (src %d, grid %d)" % (s, src, grid)
            if exact_preds:
                assert np.array_equal(new_p, old_p), "hub_slice=%d predecessors differ from hub_slice=0 in a bottom-up-only search" % s


def test_boundary_graph_is_what_the_construction_says():
    for pos, first in [(pos, F) for pos in POSITIONS] + [(3, F4), (256, F4)]:
        b = _boundary(pos, first)
        g, lab = b.g, b.ref
        deg = np.diff(g.row_offsets)
        assert (deg[:b.with_edges] > 0).all() and (deg[b.with_edges:] == 0).all()         # relabel_hubs = 0 keeps the ids
        assert deg[list(b.hubs)].min() > deg[2:].max()                                       # the hubs are every walker's heads
        assert (lab[b.front:b.front + N_FRONT] == 1).all() and (lab == 1).sum() == N_FRONT   # the frontier of the first sweep
        assert (lab[list(b.hubs)] == 3).all() and lab[b.closed] == 4
        for rows in (b.walkers, b.first, b.pair, b.flagged, b.second):
            assert (lab[rows] == 2).all()
        w = b.walkers[1]
        assert g.col_indices[g.row_offsets[w] + pos] == b.front + 1                         # row position `pos`
        assert g.col_indices[g.row_offsets[b.walkers[0] + 1] - 1] == b.front                # ... and the row's last entry
        assert g.nodes % 64 != 0


def test_option_is_known_and_flips_between_searches():
    b = _boundary(9)
    p = _problem(b.g)
    assert p.relabel_info()["hubs"] == 0
    for s in (F + 4, 0, -1, F + 4, 32, 0, 0, CAP, 10 * CAP, F + 3):
        assert np.array_equal(_run(p, b.src, s)[0], b.ref)
    for relabel in (0, 1):                 # an explicit slice is honoured in the caller's numbering too
        p.set_option("relabel", relabel)
        _check(b.g, p, b.src, b.ref, [F + 4, -1])
    p.close()


@pytest.mark.parametrize("pos", POSITIONS)
def test_boundary_rows(pos):
    """the only in-frontier neighbour at id S-1, S, S+1: as first head, second head, flagged head, and at row position `pos` / last"""
    b = _boundary(pos)
    p = _problem(b.g)
    slices = SLICES + [b.with_edges + 1, b.nodes + 7, 2 * b.nodes + 64, CAP]
    for walk_queue in (1, 0):
        p.set_option("walk_queue", walk_queue)
        for chain in (0, 4):
            p.set_option("chain_sweeps", chain)
            _check(b.g, p, b.src, b.ref, slices)
    p.close()


@pytest.mark.parametrize("pos", [3, 256])
def test_boundary_at_a_four_word_boundary(pos):
    """S = 384 .. 388: ids 384 .. 387 are in the frontier and LDS word 12 is the first of a 16-byte unit, filled only when S > 384"""
    b = _boundary(pos, F4)
    p = _problem(b.g)
    for walk_queue in (1, 0):
        p.set_option("walk_queue", walk_queue)
        for chain in (0, 4):
            p.set_option("chain_sweeps", chain)
            _check(b.g, p, b.src, b.ref, SLICES4)
    p.set_head_pass(1, 0)
    _check(b.g, p, b.src, b.ref, SLICES4, exact_preds=False)
    p.close()


@pytest.mark.parametrize("mark_pred,idempotence", MODES)
def test_boundary_modes_and_schedules(mark_pred, idempotence):
    """every (mark_pred, idempotence) mode; dense-only and default sweeps; label deferral; grids of 1 and 2; heads, then the rest"""
    slices = [33, F, F + 4, F + 5, CAP]
    for pos in (3, 256):
        b = _boundary(pos)
        for forced in (True, False):
            p = _problem(b.g, mark_pred, idempotence, forced)
            for div, defer, grid in ((0, 1, 0), (6, 0, 1), (6, 1, 2)):
                p.set_option("sparse_sweep_div", div)
                p.set_label_deferral(defer)
                _check(b.g, p, b.src, b.ref, slices, grid, exact_preds=forced)
            p.set_head_pass(1, 0)          # a heads-only pass on every eligible level, the rest of the level after it
            for chain in (0, 4):
                p.set_option("chain_sweeps", chain)
                _check(b.g, p, b.src, b.ref, slices, exact_preds=False)
            p.close()


@pytest.mark.parametrize("hubs", [0, 1, 64])
def test_hub_tier_differs_from_the_slice(hubs):
    """the slice covers ids [0, S) whatever the tier sizes are: hub tiers of 0, 1 and 64 vertices under every S"""
    b = _boundary(35)
    p = _problem(b.g, hubs=hubs)
    assert p.relabel_info()["hubs"] <= hubs
    _check(b.g, p, b.src, b.ref, SLICES + [-1, CAP])
    p.set_option("relabel_hubs", 2)       # the copy is rebuilt under the same handle
    _check(b.g, p, b.src, b.ref, [1, 2, 3, F + 4, -1])
    p.close()


def test_graph_inside_one_bitmap_word():
    """28 vertices: a star whose centre is id 0, a path behind one of its leaves, and an edgeless vertex"""
    n = 28
    u = [0] * 20 + [20, 21, 22, 23, 24, 25]
    v = list(range(1, 21)) + [21, 22, 23, 24, 25, 26]
    g = _csr_pairs(n, u, v)
    for src in (0, 26, 5, 27):
        ref = o.bfs(g, src)[0]
        for hubs in (0, 1):
            p = _problem(g, hubs=hubs)
            _check(g, p, src, ref, [1, 2, 20, 27, 28, 31, 32, 33, 64, 100, CAP, -1])
            p.close()


SEEDED = [(s, k) for s in (10, 11, 12) for k in range(10)]


@pytest.mark.parametrize("scale,k", SEEDED)
def test_seeded_rmat(scale, k):
    """30 seeded R-MAT graphs: forced bottom-up and the default schedule, hub tiers 64 and 0, the default slice among the sizes"""
    g = o.rmat_seeded(scale, (4 + k) << scale, seed=0x6873 + 16 * scale + k)
    deg = np.diff(g.row_offsets)
    sources = sorted({int(np.argmax(deg)), int(np.nonzero(deg > 0)[0][-1])})
    refs = {s: o.bfs(g, s)[0] for s in sources}
    edged = int((deg > 0).sum())
    slices = [-1, 33, 64 + k, 1000 + 37 * k, edged - 1, edged + 1, g.nodes + 1, CAP]
    for forced in (True, False):
        p = _problem(g, True, True, forced, hubs=64 if k % 2 == 0 else 0)
        p.set_option("walk_queue", k % 3 != 2)
        for src in sources:
            _check(g, p, src, refs[src], slices, grid=k % 3, exact_preds=forced)
        p.close()


def test_heavy_tailed_multigraph():
    """repeated entries and self-loops (a configuration-model multigraph), the slice at sizes off every word boundary"""
    g = _degree_sequence_graph(4099, 7)
    src = int(np.argmax(np.diff(g.row_offsets)))
    ref = o.bfs(g, src)[0]
    for hubs in (0, 64):
        p = _problem(g, hubs=hubs)
        _check(g, p, src, ref, [1, 31, 33, 65, 100, 1023, 2049, 4098, 4099, 4100, -1])
        p.close()
