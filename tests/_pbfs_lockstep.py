"""Lockstep driver for the per-rank steps of the partitioned BFS.  TEST INFRASTRUCTURE.

All P ranks of a search are held as P engines in ONE process (NumpyEngine, tests/_numpy_engine.py, or multi_gpu.HipEngine:
the same interface) and the "collectives" are torch.cat, so a search can be run step by step under any schedule of
top-down and bottom-up levels -- not only the direction rule's -- and two engine lists can be advanced side by side with
every intermediate result compared: what a rank sends to which owner, what filter_received claims, the frontier bitmap
word for word with its padding, the (len, edges) every step returns, the labels after every level.

The second value of bottom_up is not part of the contract (the dense sweep reports 0, the model the degree sum; the level
loops do not use it while the search stays bottom-up and bitmap_to_queue recomputes it), so it is not compared.

No GPU is touched at import: the graphs and the case lists below are plain numpy.
"""
import functools

import numpy as np
import torch

from gunrockinst_amd import multi_gpu as mg

TRAILING_WORDS = (0xFFFFFFFF, 0x5A5A5A5A)  # ride behind every rank's gathered bitmap when trailing=True: never vertex bits

SCHEDULES = {
    "td": ["td"],
    "bu": ["bu"],
    "td_bu": ["td", "bu"],
    "bu_td": ["bu", "td"],
    "td_bu_td": ["td", "bu", "td"],
    "alt": ["td", "bu", "td", "bu", "td", "bu", "td"],
}
PARTS = (1, 2, 3, 5, 8)


# ------------------------------------------------------------------------------------------------------------------
# graphs: name -> (n, row_offsets, col_indices)
# ------------------------------------------------------------------------------------------------------------------
def csr_from_pairs(n, pairs, symmetric=True):
    """COO -> CSR (int32): pairs mirrored when symmetric, self loops and duplicates dropped, rows sorted."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if symmetric:
        pairs = np.concatenate([pairs, pairs[:, ::-1]])
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    keys = np.unique(pairs[:, 0] * n + pairs[:, 1])
    rows, cols = keys // n, keys % n
    ro = np.zeros(n + 1, dtype=np.int32)
    ro[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return n, ro, cols.astype(np.int32)


def _random_pairs(n, count, seed):
    return np.random.default_rng(seed).integers(0, n, size=(count, 2))


def _build_graphs():
    g = {}
    g["one_vertex"] = csr_from_pairs(1, [])                                   # P > 1: ranks that own no vertex
    g["two"] = csr_from_pairs(2, [(0, 1)])                                    # P >= 3: empty ranks
    g["path_200"] = csr_from_pairs(200, [(i, i + 1) for i in range(199)])     # depth 199, interior rows of exactly two entries
    g["star_700"] = csr_from_pairs(700, [(699, i) for i in range(699)])       # leaf 698: the hub's last entry, past the 512-entry head scan
    g["k_8_40"] = csr_from_pairs(48, [(a, 8 + b) for a in range(8) for b in range(40)])  # owners receive duplicates from every peer
    g["rand_191"] = csr_from_pairs(191, _random_pairs(191, 600, 191))         # P = 3: n_local 64/64/63
    g["rand_192"] = csr_from_pairs(192, _random_pairs(192, 600, 192))         # 64/64/64
    g["rand_193"] = csr_from_pairs(193, _random_pairs(193, 600, 193))         # 65/64/64: rank 0's bitmap has 4 words, the others' 2
    g["rand_1535"] = csr_from_pairs(1535, _random_pairs(1535, 3000, 1535))    # 512/512/511: one sweep step of 512 vertices
    g["rand_1537"] = csr_from_pairs(1537, _random_pairs(1537, 3000, 1537))    # 513/512/512
    g["sparse_12289"] = csr_from_pairs(12289, _random_pairs(12289, 14000, 12289))  # 4097/4096/4096: one compacting-sweep chunk
    g["isolated_tail"] = csr_from_pairs(130, [(0, 1), (1, 2), (2, 3), (64, 65), (65, 66)])  # edgeless vertices, the last word included
    lo_hi = np.sort(_random_pairs(64, 150, 64), axis=1)
    g["dag_64"] = csr_from_pairs(64, lo_hi, symmetric=False)                  # directed, lower -> higher id: top-down only, sinks labelled
    return g


GRAPHS = _build_graphs()
DIRECTED = ("dag_64",)
EXTRA_SOURCES = {"star_700": (698,)}


def sources(name):
    """0, n - 1, the first vertex of highest degree, and the graph's extras (duplicates dropped, order kept)."""
    n, ro, _ = GRAPHS[name]
    out = []
    for s in (0, n - 1, int(np.argmax(np.diff(ro)))) + tuple(EXTRA_SOURCES.get(name, ())):
        if s not in out:
            out.append(s)
    return out


def hub(name):
    return int(np.argmax(np.diff(GRAPHS[name][1])))


def schedules(name):
    return ["td"] if name in DIRECTED else list(SCHEDULES)


def slices(name, parts):
    _, ro, ci = GRAPHS[name]
    return [mg.partition_csr_host(ro, ci, r, parts) for r in range(parts)]


def model_engines(name, parts):
    from _numpy_engine import NumpyEngine
    n = GRAPHS[name][0]
    return [NumpyEngine(n, parts, r, ro, ci) for r, (ro, ci) in enumerate(slices(name, parts))]


def oracle_graph(name):
    from oracle import gr_oracle as o
    return o.Csr(*GRAPHS[name])


@functools.lru_cache(maxsize=None)
def serial_bfs(name, src):
    """(labels, depth) of the oracle's serial BFS: computed once per (graph, source), shared, read-only."""
    from oracle import gr_oracle as o
    labels, _, depth = o.bfs(oracle_graph(name), src)
    labels.flags.writeable = False
    return labels, depth


# ------------------------------------------------------------------------------------------------------------------
# option list of the level loop inside the library (grx_pbfs_search), shared by the one-rank and the real-peer tests
# ------------------------------------------------------------------------------------------------------------------
# The library's defaults; every option dict below overrides some of them and ALL of them are set before every search.
DEFAULTS = dict(dobfs=True, mark_pred=False, alpha=12.0, lite_factor=230.0, sparse_sweep_div=6, walk_queue=1)
ALWAYS = 1e9   # alpha: bottom-up from the first level on
# The two lite_factor cases run with alpha = 1e-3, so that the direction rule itself (frontier edges * alpha > unexplored
# edges) never fires on these graphs (frontier edges <= m) and the count-only rule (frontier edges * alpha * lite_factor >
# unexplored edges, m < 1e5 here) decides alone: with 1e9 the first level of a source with edges is count-only, with 0 none is.
LIBRARY_OPTIONS = {
    "top_down": dict(dobfs=False),
    "do": dict(),
    "do_pred": dict(mark_pred=True),
    "always_pred": dict(alpha=ALWAYS, mark_pred=True),
    "lite_0": dict(alpha=1e-3, lite_factor=0.0),
    "lite_1e9": dict(alpha=1e-3, lite_factor=1e9),
    "always_sparse_0": dict(alpha=ALWAYS, sparse_sweep_div=0),
    "always_sparse_1": dict(alpha=ALWAYS, sparse_sweep_div=1),           # the compacting sweep on every bottom-up level
    "always_sparse_1_pred": dict(alpha=ALWAYS, sparse_sweep_div=1, mark_pred=True),
    "always_walk_0": dict(alpha=ALWAYS, sparse_sweep_div=0, walk_queue=0),
    "do_walk_0_pred": dict(walk_queue=0, mark_pred=True),
}


def library_options(name):
    """The option dicts (defaults filled in) a graph runs; a directed graph never searches bottom-up."""
    out = {}
    for key, opt in LIBRARY_OPTIONS.items():
        full = dict(DEFAULTS, **opt)
        if name in DIRECTED and full["dobfs"]:
            continue
        out[key] = full
    return out


def configure(bfs, opt):
    """Sets every option of a LibraryBfs for the next search."""
    from gunrockinst_amd.multi_gpu import HipEngine
    HipEngine._check(bfs.lib.grx_pbfs_set_options(bfs._h, int(opt["mark_pred"]), 0.0), "grx_pbfs_set_options")
    for key in ("alpha", "lite_factor", "sparse_sweep_div", "walk_queue"):
        bfs.set_option(key, opt[key])


def check_library_search(name, src, opt, levels, labels, preds, marked_before, marked_after):
    """What a finished grx_pbfs_search must satisfy; returns a list of complaints (empty: fine)."""
    from oracle import gr_oracle as o
    bad = []
    ref, depth = serial_bfs(name, src)
    if not np.array_equal(labels, ref):
        bad.append("labels differ at %s" % np.nonzero(labels != ref)[0].tolist()[:8])
    if levels not in (depth - 1, depth):
        bad.append("levels %d, depth %d" % (levels, depth))
    if opt["mark_pred"] and o.check_bfs_preds(oracle_graph(name), src, labels, preds) != 0:
        bad.append("preds are not valid parents")
    n, ro, _ = GRAPHS[name]
    if opt["dobfs"] and not opt["mark_pred"] and opt["lite_factor"] >= 1e9 and opt["alpha"] < 1.0 and ro[src + 1] > ro[src]:
        if marked_after <= marked_before:
            bad.append("marked_levels did not grow (%d)" % marked_after)
    if opt["lite_factor"] == 0.0 and marked_after != marked_before:
        bad.append("marked_levels moved under lite_factor 0 (%d -> %d)" % (marked_before, marked_after))
    return bad


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------
def _fence(t):
    """The engine's kernels run on its own non-blocking stream, torch.cat on torch's: a device tensor built here is complete
    before an engine reads it (what Comm._fence does for RCCL)."""
    if t.is_cuda:
        torch.cuda.synchronize()
    return t


def _steps(engines, src, schedule, trailing):
    """Generator: runs one search and yields (step, results of all ranks) after every step; returns (labels, levels)."""
    parts = len(engines)
    n = engines[0].n_global
    res = [e.reset(src) for e in engines]
    yield "reset", res
    total = sum(r[0] for r in res)
    mode, levels = "td", 0
    while total > 0:
        assert levels <= n + 2, "the search did not end within n + 2 levels"
        want = schedule[min(levels, len(schedule) - 1)]
        if want != mode:
            if want == "bu":
                for e in engines:
                    e.queue_to_bitmap()
                yield "queue_to_bitmap", None
            else:
                res = [e.bitmap_to_queue() for e in engines]
                yield "bitmap_to_queue", res
                total = sum(r[0] for r in res)
            mode = want
            if total == 0:
                break
        if mode == "td":
            sent = [e.advance_local() for e in engines]
            yield "advance_local", sent
            segments = []
            for counts, buf in sent:
                assert len(counts) == parts and int(buf.numel()) == sum(counts)
                segments.append(torch.split(buf, [int(c) for c in counts]))
            res = []
            for q, e in enumerate(engines):  # owner q receives segment q of ranks 0..P-1, in rank order
                res.append(e.filter_received(_fence(torch.cat([segments[p][q] for p in range(parts)]))))
            yield "filter_received", res
        else:
            bitmaps = [e.frontier_bitmap() for e in engines]
            words = int(bitmaps[0].numel())
            assert all(int(b.numel()) == words for b in bitmaps)
            if trailing:
                tail = torch.from_numpy(np.array(TRAILING_WORDS, dtype=np.uint32).view(np.int32)).to(bitmaps[0].device)
                bitmaps = [torch.cat([b, tail]) for b in bitmaps]
            gathered = _fence(torch.cat(bitmaps))
            res = [e.bottom_up(gathered, words + (2 if trailing else 0)) for e in engines]
            yield "bottom_up", res
        total = sum(r[0] for r in res)
        levels += 1
        yield "level", mode
    full = np.empty(n, dtype=np.int32)
    for r, e in enumerate(engines):
        full[r::parts] = e.labels()
    return full, levels


def run(engines, src, schedule, trailing, check=None):
    """One search of the P engines (one per rank) under `schedule` ("td" / "bu" per level, the last entry repeats).
    check(step, results) is called after every step.  Returns (assembled global labels, levels)."""
    it = _steps(engines, src, schedule, trailing)
    while True:
        try:
            step, res = next(it)
        except StopIteration as end:
            return end.value
        if check is not None:
            check(step, res)


# ------------------------------------------------------------------------------------------------------------------
# side by side: the model and the engines under test, every step compared
# ------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _compare_bitmaps(model, hip, where):
    for r, (m, h) in enumerate(zip(model, hip)):
        words = mg.mask_words((m.n_global + m.parts - 1) // m.parts)
        mb, hb = _np(m.frontier_bitmap()), _np(h.frontier_bitmap())
        assert mb.shape[0] == words and hb.shape[0] == words, "%s: rank %d: %d bitmap words, %d expected" % (where, r, hb.shape[0], words)
        bits = np.unpackbits(hb.view(np.uint8), bitorder="little")
        assert not bits[m.n_local:].any(), "%s: rank %d: frontier bits at positions >= n_local = %d: %s" % (
            where, r, m.n_local, (np.nonzero(bits[m.n_local:])[0] + m.n_local).tolist()[:8])
        assert np.array_equal(mb, hb), "%s: rank %d: frontier bitmap differs in words %s" % (where, r, np.nonzero(mb != hb)[0].tolist()[:8])


def run_side_by_side(model, hip, src, schedule, trailing):
    """Advances both engine lists through the same search and asserts after every step that they agree.  Returns
    (labels, levels, found_bottom_up): the last is, per rank, the local ids that a bottom-up level discovered."""
    parts = len(model)
    assert len(hip) == parts
    a, b = _steps(model, src, schedule, trailing), _steps(hip, src, schedule, trailing)
    found_bu = [np.zeros(m.n_local, dtype=bool) for m in model]
    count = 0
    while True:
        try:
            step, ra = next(a)
        except StopIteration as end:
            la, levels = end.value
            try:
                next(b)
            except StopIteration as end_b:
                lb, levels_b = end_b.value
            else:
                raise AssertionError("the model's search ended after %d steps, the other went on" % count)
            assert levels == levels_b and np.array_equal(la, lb)
            return lb, levels, found_bu
        try:
            step_b, rb = next(b)
        except StopIteration:
            raise AssertionError("the search under test ended after %d steps, the model went on with %s" % (count, step))
        count += 1
        where = "step %d (%s)" % (count, step)
        assert step == step_b, "%s: the search under test is at %s" % (where, step_b)
        if step in ("reset", "filter_received", "bitmap_to_queue"):
            for r in range(parts):
                assert tuple(ra[r]) == tuple(rb[r]), "%s: rank %d returns (len, edges) = %s, model %s" % (where, r, tuple(rb[r]), tuple(ra[r]))
        elif step == "advance_local":
            for r in range(parts):
                (ca, sa), (cb, sb) = ra[r], rb[r]
                assert [int(x) for x in ca] == [int(x) for x in cb], "%s: rank %d send_counts %s, model %s" % (where, r, list(cb), list(ca))
                sa, sb = _np(sa), _np(sb)
                offs = np.concatenate(([0], np.cumsum(ca))).astype(np.int64)
                for q in range(parts):
                    seg_a, seg_b = np.sort(sa[offs[q]:offs[q + 1]]), np.sort(sb[offs[q]:offs[q + 1]])
                    assert np.unique(seg_b).shape[0] == seg_b.shape[0], "%s: rank %d sends owner %d an id twice" % (where, r, q)
                    assert np.array_equal(seg_a, seg_b), "%s: rank %d -> owner %d: ids %s, model %s" % (where, r, q, seg_b[:16].tolist(), seg_a[:16].tolist())
        elif step == "bottom_up":
            for r in range(parts):
                assert int(ra[r][0]) == int(rb[r][0]), "%s: rank %d found %d, model %d" % (where, r, int(rb[r][0]), int(ra[r][0]))
        if step in ("queue_to_bitmap", "bottom_up"):
            _compare_bitmaps(model, hip, where)
        if step in ("filter_received", "bottom_up", "level"):  # (the labels right after the step that wrote them, and after the level)
            for r in range(parts):
                lm, lh = _np(model[r].labels()), _np(hip[r].labels())
                assert np.array_equal(lm, lh), "%s: rank %d: labels differ at local ids %s" % (where, r, np.nonzero(lm != lh)[0].tolist()[:8])
        if step == "bottom_up":
            for r in range(parts):
                bits = np.unpackbits(_np(model[r].frontier_bitmap()).view(np.uint8), bitorder="little").astype(bool)
                found_bu[r] |= bits[:model[r].n_local]


def check_stepwise_preds(name, src, labels, preds_per_rank, found_bu):
    """Parents of the step-wise path: -1 at the source; a vertex that a bottom-up level found names a global neighbour one
    level up; everything else -- top-down finds (no parents travel with the ids) and unreached vertices -- keeps -2."""
    n, ro, ci = GRAPHS[name]
    parts = len(preds_per_rank)
    preds = np.empty(n, dtype=np.int32)
    by_bu = np.zeros(n, dtype=bool)
    for r in range(parts):
        preds[r::parts] = preds_per_rank[r]
        by_bu[r::parts] = found_bu[r]
    assert preds[src] == -1, "the source's pred is %d" % preds[src]
    for v in range(n):
        if v == src:
            continue
        p = int(preds[v])
        if by_bu[v]:
            assert 0 <= p < n and p in ci[ro[v]:ro[v + 1]] and labels[p] == labels[v] - 1, \
                "vertex %d (label %d, found bottom-up) has pred %d" % (v, labels[v], p)
        else:
            assert p == -2, "vertex %d (label %d, not found bottom-up) has pred %d, not -2" % (v, labels[v], p)
