"""Subgraph matching: the binding of grx_sm_* (gunrock_mi355x.h).

The CSR is read as the simple undirected graph G, as TC and the clique family read it, with an optional int32 label per vertex.  A
pattern H has q vertices (2 .. 6), a list of pairs, an optional int32 label per vertex (-1: a wildcard) and the flag `induced`.  The
results are integers with one value each: the occurrences of H in G (embeddings modulo Aut(H)), the embeddings, and per vertex the
occurrences whose image contains it."""
import ctypes as C

import numpy as np

from .capi import _TunedProblem, _check, _cut, _i32, _one_shot, _opt, _out, _p, lib

SM_AUTO, SM_GROUP8, SM_WAVE = 0, 1, 2  # enum GRX_SM_* (gunrock_mi355x.h): option "strategy"
SM_TOO_LARGE, SM_NOT_CERTIFIED = -4, -5  # grx_sm_enact, next to -1 / -2 / -3
SM_MAX_Q, SM_MAX_CONSTRAINTS = 6, 15

# named patterns: (q, pairs).  The paw has its triangle on 0, 1, 2 and its pendant on 2; the diamond its chord on 0 - 1; the house
# its roof on 0 and its square on 1, 2, 3, 4; the bull its triangle on 0, 1, 2 and its horns on 1 and 2.
SM_PATTERNS = {
    "edge": (2, [(0, 1)]),
    "wedge": (3, [(0, 1), (1, 2)]),
    "triangle": (3, [(0, 1), (1, 2), (0, 2)]),
    "p4": (4, [(0, 1), (1, 2), (2, 3)]),
    "claw": (4, [(0, 1), (0, 2), (0, 3)]),
    "c4": (4, [(0, 1), (1, 2), (2, 3), (3, 0)]),
    "paw": (4, [(0, 1), (1, 2), (0, 2), (2, 3)]),
    "diamond": (4, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)]),
    "k4": (4, [(a, b) for a in range(4) for b in range(a + 1, 4)]),
    "c5": (5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]),
    "house": (5, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 4), (3, 4)]),
    "bull": (5, [(0, 1), (1, 2), (0, 2), (1, 3), (2, 4)]),
    "k5": (5, [(a, b) for a in range(5) for b in range(a + 1, 5)]),
    "c6": (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)]),
    "k6": (6, [(a, b) for a in range(6) for b in range(a + 1, 6)]),
}
SM_GRAPHLETS = {3: ("wedge", "triangle"), 4: ("p4", "claw", "c4", "paw", "diamond", "k4")}  # the connected k-vertex graphs


class SmTooLarge(ArithmeticError):
    """SmProblem.enact: the work bound (q - 1) * hom(T, G) exceeds "work_limit" (GRX_SM_TOO_LARGE): nothing ran, the handle holds no
    result and takes the next pattern or option"""


class SmNotCertified(RuntimeError):
    """SmProblem.enact under "symmetry" 0: a count was no multiple of |Aut(H)| (GRX_SM_NOT_CERTIFIED): there is no result"""


class SmProblem(_TunedProblem):
    """SmProblem + SmEnactor behind the handle C ABI: the occurrences of a pattern in the CSR read as an undirected simple graph,
    per vertex (int64) and in total.  One graph per handle, any number of patterns, one at a time.  A device CSR and device labels
    stay the caller's; the labels are read by every enact.

    Options: "symmetry", "per_vertex", "strategy" (SM_AUTO / SM_GROUP8 / SM_WAVE), "group_max_row", "work_limit", "order".
    device_results: (device pointer of the int64 counts, device pointer of the int32 degrees)."""

    _family, _problem, _enactor = "sm", "SmProblem", "SmEnactor"
    _results = 2
    q = 0  # of the pattern in force
    _stats = (("items", ("group8_items", "wave_items"), "candidates", "bisections", "occurrences", "embeddings", "pairs", "longest_row",
               "kernel_launches"), ("bound", "kernel_ms", "bin_ms", "group8_ms", "wave_ms", "finish_ms", "build_ms"))

    def init(self, nodes, row_offsets, col_indices, labels=None):
        return self._init_host(nodes, row_offsets, col_indices, per_node=(labels, "labels", "nodes"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_labels=None):
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_labels))

    def set_pattern(self, q, pairs, labels=None, induced=False):
        """the pattern of the next enact: q vertices, pairs as a sequence of (a, b) or a name of SM_PATTERNS (then q may be None).
        ValueError for what is no pattern; the one in force stays"""
        if isinstance(pairs, str):
            q, pairs = SM_PATTERNS[pairs] if q is None else (q, SM_PATTERNS[pairs][1])
        ab = _i32(np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2))
        a, b = np.ascontiguousarray(ab[:, 0]), np.ascontiguousarray(ab[:, 1])
        plabels = None if labels is None else _i32(labels)
        if plabels is not None and plabels.shape[0] != int(q):
            raise ValueError("gunrockinst_amd: %d pattern labels for %d pattern vertices" % (plabels.shape[0], int(q)))
        rc = lib().grx_sm_set_pattern(self._h, int(q), int(a.shape[0]), _p(a), _p(b), _opt(plabels), int(bool(induced)))
        if rc == -1:
            raise ValueError("gunrockinst_amd: SmProblem::SetPattern: not a connected simple pattern of 2 .. %d vertices (code %d)" % (SM_MAX_Q, rc))
        _check(rc, "SmProblem::SetPattern")
        self.q = int(q)
        return self

    def pattern_info(self):
        """{"q", "aut", "order", "constraints"}: |Aut(H)|, the matching order and the pairs (lo, hi) with f(lo) < f(hi), of the
        pattern and the options in force"""
        q, aut, count = C.c_int(), C.c_int(), C.c_int()
        order, lo, hi = _out(SM_MAX_Q), _out(SM_MAX_CONSTRAINTS), _out(SM_MAX_CONSTRAINTS)
        _check(lib().grx_sm_pattern_info(self._h, C.byref(q), C.byref(aut), _p(order), C.byref(count), _p(lo), _p(hi)), "grx_sm_pattern_info")
        return {"q": q.value, "aut": aut.value, "order": order[:q.value].tolist(),
                "constraints": list(zip(lo[:count.value].tolist(), hi[:count.value].tolist()))}

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds.  SmTooLarge, SmNotCertified: there is no result"""
        ms = C.c_float()
        rc = lib().grx_sm_enact(self._h, int(max_grid_size), C.byref(ms))
        if rc == SM_TOO_LARGE:
            raise SmTooLarge("gunrockinst_amd: SmEnactor::Enact refused: hom(T, G) = %.17g puts the work beyond work_limit (code %d)"
                             % (self.stats()["bound"], rc))
        if rc == SM_NOT_CERTIFIED:
            raise SmNotCertified("gunrockinst_amd: SmEnactor::Enact: a count is no multiple of |Aut(H)| (code %d)" % rc)
        _check(rc, "SmEnactor::Enact")
        return float(ms.value)

    def extract(self, count=True):
        """(count as int64 per vertex, or None; occurrences; embeddings)"""
        out, occ, emb = _out(self.nodes, np.int64, count), C.c_longlong(), C.c_longlong()
        _check(lib().grx_sm_extract(self._h, _opt(out), C.byref(occ), C.byref(emb)), "SmProblem::Extract")
        return _cut(out, self.nodes), int(occ.value), int(emb.value)


def gunrock_subgraph_matching(nodes, row_offsets, col_indices, pattern_pairs, q=None, labels=None, pattern_labels=None, induced=False, device=0):
    """One-shot subgraph matching: (count int64 per vertex, occurrences, aut).  pattern_pairs: (a, b) pairs, or a name of SM_PATTERNS"""
    def result(p):
        count, occurrences, _ = p.extract()
        return count, occurrences, p.pattern_info()["aut"]
    return _one_shot(SmProblem(device=device).init(nodes, row_offsets, col_indices, labels), lambda p: p.set_pattern(q, pattern_pairs, pattern_labels, induced),
                     SmProblem.enact, result)


def gunrock_graphlets(nodes, row_offsets, col_indices, k, device=0):
    """The induced occurrences of every connected k-vertex graphlet, k = 3 or 4, on one handle: {name: (count int64 per vertex,
    occurrences)} over SM_GRAPHLETS[k]"""
    if k not in SM_GRAPHLETS:
        raise ValueError("gunrockinst_amd: graphlets of 3 or 4 vertices, not %r" % (k,))

    def census(p):
        out = {}
        for name in SM_GRAPHLETS[k]:
            p.set_pattern(None, name, induced=True)
            p.enact()
            count, occurrences, _ = p.extract()
            out[name] = (count, occurrences)
        return out
    return _one_shot(SmProblem(device=device).init(nodes, row_offsets, col_indices), census)
