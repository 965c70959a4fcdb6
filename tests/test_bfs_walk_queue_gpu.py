"""The per-wave walk queue of the dense bottom-up sweep (walk_queue = 1, DESIGN §3.3 m) against the step-by-step walk loop it
replaces (walk_queue = 0) and against the oracle.  Every comparison is exact.

Every case is compared three ways: labels against oracle.bfs, labels against the same problem run with walk_queue = 0, and
predecessors with check_bfs_preds.  Where the search is forced bottom-up (alpha = beta = 1e12, no tail kernel) predecessors
are also compared value by value: both forms give a vertex its first head in the frontier, else the first in-frontier entry
of its row in row order.

"Decoy" graphs make the dense sweep walk.  Two hubs of the largest degree are every walker's adjacency heads, and are not in
the frontier when the walkers are asked (they are found through the walkers, one level later).  A walker's row is, in row
order: the two hubs, `pos - 2` low fillers, one vertex of the level-1 frontier at row position `pos` (0-based), and `trail`
high fillers.  Fillers are found through the walkers, so no filler is in the frontier either.  A walker without the frontier
vertex walks its whole row in vain, twice, and is found through its heads two levels later.  Walkers sit at chosen offsets of
512-vertex steps (the caller's numbering, relabel = 0); the other vertices of those steps have no edges.

Mutations of DenseSweepQueued and the first test that fails for each (run against this file):
  the flagged second head taken for "none" (flag decode)      test_option_is_known_and_flips_between_searches
  the partial round at the end of a batch dropped             test_decoy_forced_bottom_up[False-False]
  the late-find OR into the batch's found words dropped       test_decoy_forced_bottom_up[False-False]
  the `count >= 64` test shifted by one                       none, and none can: with `> 64` at most 64 entries wait before an
      append of at most 64, which the 128-slot ring holds exactly; with `>= 63` a round of 63 leaves earlier.  Either way every
      walker is still walked once and results are unchanged; only how full the rounds are moves.  What guards the bound is the
      static_assert on kWalkDrain and kWalkQueue in bottom_up.hpp (a drain threshold above 64 does not compile)."""
import numpy as np
import pytest

import gunrockinst_amd as ga
from oracle import gr_oracle as o
from test_bfs_label_pass_gpu import _sources

pytestmark = pytest.mark.gpu

MODES = [(False, False), (True, False), (False, True), (True, True)]
POSITIONS = [3, 8, 9, 10, 32, 33, 34, 35, 256, 257, 1025]
STEP = 512
N_LOW = 1024          # low fillers: enough for the frontier vertex at row position 1025
N_HIGH = 3            # high fillers: entries after the frontier vertex
N_FRONT = 8           # level-1 vertices the walkers find
N_PAD = 64            # leaves on both hubs: their degree stays above every filler's


def _csr_pairs(n, u, v):
    """symmetric CSR (rows sorted by column) from undirected pairs; a repeated pair is a repeated entry, (x, x) is one self-loop"""
    u = np.asarray(u, np.int64)
    v = np.asarray(v, np.int64)
    loop = u == v
    rows = np.concatenate([u, v[~loop]])
    cols = np.concatenate([v, u[~loop]])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    ro = np.zeros(n + 1, np.int64)
    np.add.at(ro, rows + 1, 1)
    return o.Csr(n, np.cumsum(ro).astype(np.int32), cols.astype(np.int32))


class Decoy:
    """ids: hubs 0 1 | low fillers | frontier vertices | high fillers | path, pads, specials, source | (512-aligned) walker steps | tail"""

    def __init__(self, tail=0):
        self.u, self.v = [], []
        self.hubs = (0, 1)
        self.low = 2
        self.front = self.low + N_LOW
        self.high = self.front + N_FRONT
        nxt = self.high + N_HIGH
        self.src = nxt
        self.path = [nxt + 1, nxt + 2, nxt + 3]
        nxt += 4
        # the hubs hang off a path from the source (level 4 that way; the walkers bring them in at level 3)
        self._edge(self.src, self.path[0]); self._edge(self.path[0], self.path[1]); self._edge(self.path[1], self.path[2])
        for h in self.hubs:
            self._edge(self.path[2], h)
            for k in range(N_PAD):
                self._edge(h, nxt + k)
        nxt += N_PAD
        for k in range(N_FRONT):
            self._edge(self.src, self.front + k)
        self.free = nxt                       # specials are handed out from here
        self.special_end = nxt + 64
        self.base = (self.special_end + STEP - 1) // STEP * STEP
        self.steps = 0
        self.tail = tail
        self.walkers = 0

    def _edge(self, a, b):
        self.u.append(np.array([a])); self.v.append(np.array([b]))

    def _row(self, w, entries):
        e = np.asarray(entries, np.int64)
        self.u.append(np.full(e.size, w, np.int64)); self.v.append(e)

    def walker(self, w, pos, trail=0, hubs=True):
        """pos: row position of the frontier vertex (None: the row has none); the hubs are positions 0 and 1"""
        row = list(self.hubs) if hubs else []
        fill = (pos - 2) if pos is not None else 9 + (w % 40)
        assert 0 <= fill <= N_LOW and trail <= N_HIGH
        row += list(range(self.low, self.low + fill))
        if pos is not None:
            row.append(self.front + w % N_FRONT)
        row += list(range(self.high, self.high + trail))
        self._row(w, row)
        self.walkers += 1

    def special(self, entries):
        w = self.free
        self.free += 1
        assert self.free <= self.special_end
        self._row(w, entries)
        return w

    def step(self, offsets, pos=None):
        """one 512-vertex step with walkers at `offsets`; their frontier positions cycle through POSITIONS, every 7th has none"""
        first = self.base + self.steps * STEP
        for i, off in enumerate(offsets):
            w = first + int(off)
            k = self.walkers
            if pos is not None:
                self.walker(w, pos, trail=k % (N_HIGH + 1))
            elif k % 7 == 6:
                self.walker(w, None)
            else:
                p = POSITIONS[k % len(POSITIONS)]
                self.walker(w, p, trail=0 if k % 3 else k % (N_HIGH + 1))   # (trail 0: the frontier vertex is the row's last entry)
        self.steps += 1
        return first

    def csr(self):
        n = self.base + self.steps * STEP + self.tail
        return _csr_pairs(n, np.concatenate(self.u), np.concatenate(self.v))


def _spread(count, seed):
    return np.sort(np.random.default_rng(seed).choice(STEP, count, replace=False))


def _problem(g, mark_pred=True, idempotence=True, forced=True):
    p = ga.BfsProblem(mark_pred, idempotence).init(g.nodes, g.row_offsets, g.col_indices)
    if forced:   # every level bottom-up
        p.set_inverse_graph(alpha=1e12, beta=1e12)
        p.set_tuning(tail_edge_limit=0)
    else:
        p.set_inverse_graph()
    return p


def _run(p, src, walk_queue, grid=0):
    p.set_option("walk_queue", walk_queue)
    p.reset(src)
    p.enact(src, max_grid_size=grid, traversal_mode=2)
    labels, preds = p.extract()
    return labels, preds


_REF = {}


def _ref(g, src, key):
    if (key, src) not in _REF:
        _REF[(key, src)] = o.bfs(g, src)[0]
    return _REF[(key, src)]


def _check(g, p, src, key, grid=0, exact_preds=True):
    ref = _ref(g, src, key)
    new, new_p = _run(p, src, 1, grid)
    old, old_p = _run(p, src, 0, grid)
    assert np.array_equal(new, ref), "walk_queue=1 labels differ from the oracle (src %d, grid %d)" % (src, grid)
    assert np.array_equal(new, old), "walk_queue=1 labels differ from walk_queue=0 (src %d, grid %d)" % (src, grid)
    if new_p is not None:
        assert o.check_bfs_preds(g, src, new, new_p) == 0, "walk_queue=1 predecessors are not valid parents (src %d, grid %d)" % (src, grid)
        assert o.check_bfs_preds(g, src, old, old_p) == 0
        if exact_preds:
            assert np.array_equal(new_p, old_p), "predecessors differ from walk_queue=0 in a bottom-up-only search (src %d, grid %d)" % (src, grid)
    return new


def _sweep_options(g, p, src, key, exact_preds, grids=(0, 1, 2)):
    """relabel x chain_sweeps x sparse_sweep_div x label deferral x grid"""
    for relabel in (0, 1):
        p.set_option("relabel", relabel)
        for chain in (0, 4):
            p.set_option("chain_sweeps", chain)
            for div in (0, 6):   # 0: always the dense sweep; 6: the default (the compacting sweep takes the late levels)
                p.set_option("sparse_sweep_div", div)
                for defer in (1, 0):
                    p.set_label_deferral(defer)
                    for grid in grids:
                        _check(g, p, src, key, grid, exact_preds)


def _main_graph():
    """walkers per step 0, 1, 63, 64, 65, 127, 128, 129, 512; last word only then first word only; a vertex count off 64 and 512"""
    d = Decoy(tail=37)
    for i, count in enumerate((0, 1, 63, 64, 65, 127, 128, 129, 512)):
        d.step(_spread(count, i))
    d.step(np.arange(448, 512))      # only the last word of a step ...
    d.step(np.arange(0, 64))         # ... and only the first word of the next
    d.step(_spread(200, 99))
    # short rows and odd rows (ids below the walker steps)
    h1, h2 = d.hubs
    f = d.front
    d.specials = {
        "len0": d.special([]),
        "len1_front": d.special([f]),
        "len1_hub": d.special([h1]),
        "len2_hubs": d.special([h1, h2]),            # both heads miss and the row ends with them: no walk
        "len2_hub_front": d.special([h1, f + 1]),
        "len3": d.special([h1, h2, f + 2]),
        "dup_head": d.special([h1, h1, h2, f + 3]),
        "dup_pair": d.special([h1, h1]),
    }
    w = d.free
    d.specials["self_loop"] = d.special([h1, h2, w, f + 4])
    return d, d.csr()


@pytest.fixture(scope="module")
def main_graph():
    return _main_graph()


def test_option_is_known_and_flips_between_searches():
    g = o.rmat_seeded(10, 8 << 10)
    p = _problem(g)
    src = int(np.argmax(np.diff(g.row_offsets)))
    ref = o.bfs(g, src)[0]
    for relabel in (1, 0):
        p.set_option("relabel", relabel)
        for walk_queue in (1, 0, 0, 1, 1):
            assert np.array_equal(_run(p, src, walk_queue)[0], ref)
    p.close()


def test_decoy_levels_are_what_the_construction_says(main_graph):
    d, g = main_graph
    labels = _ref(g, d.src, "main")
    s = d.specials
    assert labels[d.front] == 1 and labels[d.hubs[0]] == 3 and labels[d.low] == 3
    assert labels[s["len0"]] == -1 and labels[s["len1_front"]] == 2 and labels[s["len1_hub"]] == 4
    assert labels[s["len2_hubs"]] == 4 and labels[s["len2_hub_front"]] == 2 and labels[s["len3"]] == 2
    assert labels[s["dup_head"]] == 2 and labels[s["dup_pair"]] == 4 and labels[s["self_loop"]] == 2
    walkers = np.arange(d.base, d.base + d.steps * STEP)
    deg = np.diff(g.row_offsets)[walkers]
    assert set(np.unique(labels[walkers][deg > 0]).tolist()) == {2, 4}     # found by walking / no frontier entry: through the heads later
    assert g.nodes % 64 != 0 and g.nodes % 512 != 0
    assert np.diff(g.row_offsets)[list(d.hubs)].min() > np.diff(g.row_offsets)[2:].max()   # the hubs are everybody's heads


@pytest.mark.parametrize("mark_pred,idempotence", MODES)
def test_decoy_forced_bottom_up(main_graph, mark_pred, idempotence):
    d, g = main_graph
    p = _problem(g, mark_pred, idempotence, forced=True)
    _sweep_options(g, p, d.src, "main", exact_preds=True)
    p.close()


@pytest.mark.parametrize("mark_pred,idempotence", MODES)
def test_decoy_default_schedule(main_graph, mark_pred, idempotence):
    d, g = main_graph
    p = _problem(g, mark_pred, idempotence, forced=False)
    _sweep_options(g, p, d.src, "main", exact_preds=False, grids=(0, 1))
    p.close()


@pytest.mark.parametrize("pos", POSITIONS + [2])
def test_every_frontier_position_alone(pos):
    """all walkers of the graph have their frontier vertex at the same row position, last (trail 0) and not last"""
    d = Decoy(tail=5)
    d.step(_spread(70, pos), pos=pos)
    d.step(_spread(130, pos + 1), pos=pos)
    g = d.csr()
    p = _problem(g)
    for relabel in (0, 1):
        p.set_option("relabel", relabel)
        for grid in (0, 1):
            labels = _check(g, p, d.src, ("pos", pos), grid)
            assert (labels[d.base:d.base + 2 * STEP][np.diff(g.row_offsets)[d.base:d.base + 2 * STEP] > 0] == 2).all()
    p.close()


@pytest.mark.parametrize("counts", [(63, 1), (64, 64), (65, 63), (1, 1, 1, 1, 60, 1), (127, 1, 0, 0, 0, 0, 0, 0, 1), (40,) * 13])
def test_queue_carried_across_steps_and_batches(counts):
    """a queue that is not empty at a step's end, at a batch's end (one workgroup: a wave runs many steps), and at the sweep's end"""
    d = Decoy(tail=1)
    for i, c in enumerate(counts):
        d.step(_spread(c, 10 * len(counts) + i), pos=9 if i % 2 else None)
    g = d.csr()
    p = _problem(g)
    for chain in (0, 4):
        p.set_option("chain_sweeps", chain)
        p.set_option("sparse_sweep_div", 0)
        for relabel in (0, 1):
            p.set_option("relabel", relabel)
            for grid in (1, 2, 0):
                _check(g, p, d.src, ("carry", counts), grid)
    p.close()


def _degree_sequence_graph(n, seed):
    """a configuration-model multigraph over a heavy-tailed degree sequence: repeated entries and self-loops occur"""
    rng = np.random.default_rng(seed)
    deg = np.minimum((rng.pareto(1.3, n) + 1).astype(np.int64), n // 4)
    deg[rng.integers(0, n, n // 10)] = 0
    stubs = np.repeat(np.arange(n), deg)
    rng.shuffle(stubs)
    half = stubs.size // 2
    return _csr_pairs(n, stubs[:half], stubs[half:2 * half])


SEEDED = [("rmat", s, k) for s in (10, 11, 12) for k in range(5)] + [("deg", n, k) for n in (1000, 4099, 20000) for k in range(5)]


@pytest.mark.parametrize("kind,size,k", SEEDED)
def test_seeded_sweep(kind, size, k):
    if kind == "rmat":
        g = o.rmat_seeded(size, (4 + 3 * k) << size, seed=0x6772 + k)
    else:
        g = _degree_sequence_graph(size, 100 + k)
    for forced in (True, False):
        p = _problem(g, True, True, forced)
        for relabel in (1, 0):
            p.set_option("relabel", relabel)
            for src in _sources(g):
                for grid in (0, 1):
                    _check(g, p, src, (kind, size, k), grid, exact_preds=forced)
        p.close()
