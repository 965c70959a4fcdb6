"""Maximum bipartite matching and the Dulmage-Mendelsohn decomposition: the binding of grx_bipartite_* (gunrock_mi355x.h).

A matrix is a CSR pattern of shape (rows, cols), read as given: duplicates and unsorted rows mean nothing, empty rows and columns
and a dimension of 0 are allowed.  The size of a maximum matching (the structural rank), the horizontal / square / vertical part
of every row and column, König's minimum vertex cover and the irreducible blocks of the square part have one value each; the
matching itself is one of many and is certified on the device before anything is reported as maximum."""
import ctypes as C

import numpy as np

from .capi import SccProblem, _TRACE, _TunedProblem, _check, _count_then_fill, _i32_of, _matrix, _one_shot, _opt, _out, _p, _u8p, lib

BIPARTITE_AUTO, BIPARTITE_LANE, BIPARTITE_WAVE, BIPARTITE_BLOCK = 0, 1, 2, 3  # enum GRX_BIPARTITE_* (gunrock_mi355x.h): option "strategy"
BIPARTITE_HORIZONTAL, BIPARTITE_SQUARE, BIPARTITE_VERTICAL = 0, 1, 2  # row_part / col_part
BIPARTITE_MAXIMUM, BIPARTITE_CAPPED = 0, 1  # stats()["state"]: how the last enact ended
BIPARTITE_NOT_CERTIFIED, BIPARTITE_BAD_MATCHING, BIPARTITE_NOT_MAXIMUM = -4, -5, -6  # the family's codes next to -1 / -2 / -3
BIPARTITE_SCHEDULE_AUTO, BIPARTITE_ROUNDS, BIPARTITE_DEVICE_LOOP = 0, 1, 2  # option "schedule"


class BipartiteNotCertified(RuntimeError):
    """the certificate of a bipartite matching failed: there is no result"""


class BipartiteNotMaximum(RuntimeError):
    """the parts, the cover or the blocks were asked of a run that "max_phases" ended: its matching is not known to be maximum"""


class BipartiteProblem(_TunedProblem):
    """BipartiteProblem + BipartiteEnactor behind the handle C ABI: a maximum matching of the bipartite graph rows -- columns of a
    CSR pattern, its Dulmage-Mendelsohn decomposition and König's minimum vertex cover.  Its operand is a matrix with a shape, so
    init, init_device and the attributes (rows, cols, entries) are its own.  A device CSR stays the caller's and is read by every
    enact: it has to outlive the handle.

    Options: "greedy", "max_phases", "strategy" (BIPARTITE_AUTO / BIPARTITE_LANE / BIPARTITE_WAVE / BIPARTITE_BLOCK),
    "wave_min_row", "block_min_row", "schedule" (BIPARTITE_SCHEDULE_AUTO / BIPARTITE_ROUNDS / BIPARTITE_DEVICE_LOOP),
    "loop_max_list", "loop_max_entries".
    device_results: "mate_row", "mate_col", "row_part", "col_part": int32; "row_cover", "col_cover": uint8."""

    _family, _problem, _enactor = "bipartite", "BipartiteProblem", "BipartiteEnactor"
    _results = ("mate_row", "mate_col", "row_part", "col_part", "row_cover", "col_cover")
    _KERNEL_MS = ("kernel_ms", "roots_ms", "level_ms", "loop_ms", "augment_ms", "rest_ms")

    def __init__(self, instrument=False, device=0):
        self._create("grx_bipartite_create", int(instrument), device)
        self._device = device
        self.rows = self.cols = self.entries = 0

    def init(self, shape, offsets, cols):
        """the pattern of shape (rows, cols) from the host"""
        (self.rows, self.cols), ro, ci, _ = _matrix((shape, offsets, cols, None))
        self.entries = int(ci.shape[0])
        _check(lib().grx_bipartite_init(self._h, self.rows, self.cols, self.entries, _p(ro), _p(ci)), "BipartiteProblem::Init")
        return self

    def init_device(self, shape, entries, d_offsets, d_cols):
        """d_* are integer device addresses (e.g. torch.Tensor.data_ptr()), borrowed"""
        self.rows, self.cols, self.entries = int(shape[0]), int(shape[1]), int(entries)
        _check(lib().grx_bipartite_init_device(self._h, self.rows, self.cols, self.entries, C.c_void_p(d_offsets), C.c_void_p(d_cols)),
               "BipartiteProblem::Init(device)")
        return self

    def reset(self, mate_row=None):
        """the matching the next enact starts from: a column or -1 per row, or None for the empty one.  ValueError when it is
        none: a mate out of range, a pair that is no entry, a column used twice (the start is then the empty matching)"""
        rc = lib().grx_bipartite_reset(self._h, _opt(_i32_of(mate_row, self.rows, "mates", "rows")))
        if rc == BIPARTITE_BAD_MATCHING:
            raise ValueError("gunrockinst_amd: BipartiteProblem::Reset: mate_row is no matching of the matrix (code %d)" % rc)
        _check(rc, "BipartiteProblem::Reset")

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds; stats()["state"] tells how it ended.  BipartiteNotCertified: there is no result"""
        ms = C.c_float()
        rc = lib().grx_bipartite_enact(self._h, int(max_grid_size), C.byref(ms))
        if rc == BIPARTITE_NOT_CERTIFIED:
            raise BipartiteNotCertified("gunrockinst_amd: BipartiteEnactor::Enact: the certificate failed: %r" % (self.stats()["certificate"],))
        _check(rc, "BipartiteEnactor::Enact")
        return float(ms.value)

    def stats(self):
        names = ("size", "phases", "levels", "vertical_levels", "augmentations", "greedy_pairs", "state")
        ints = [C.c_longlong() for _ in names]
        cert, regime = (C.c_longlong * 3)(), (C.c_longlong * 3)()
        loop, launches, readbacks = C.c_longlong(), C.c_longlong(), C.c_longlong()
        kernel_ms, build_ms = (C.c_double * 6)(), C.c_double()
        _check(lib().grx_bipartite_stats(self._h, *map(C.byref, ints), cert, regime, C.byref(loop), C.byref(launches), C.byref(readbacks), kernel_ms,
                                         C.byref(build_ms)), "grx_bipartite_stats")
        out = {name: x.value for name, x in zip(names, ints)}
        out.update(certificate=[int(x) for x in cert], regime_columns=[int(x) for x in regime], loop_levels=loop.value,
                   kernel_launches=launches.value, readbacks=readbacks.value, build_ms=build_ms.value)
        out.update(zip(self._KERNEL_MS, (float(x) for x in kernel_ms)))
        return out

    def phase_trace(self):
        """one row per phase of the last enact, then one for the search from the unmatched rows: (levels as int32, paths flipped
        as int64, milliseconds as float64)"""
        return _count_then_fill(lib().grx_bipartite_phase_trace, self._h, "grx_bipartite_phase_trace", _TRACE)

    def _refusing(self, rc, what):
        if rc == BIPARTITE_NOT_MAXIMUM:
            raise BipartiteNotMaximum("gunrockinst_amd: %s: the last enact ended BIPARTITE_CAPPED (code %d)" % (what, rc))
        _check(rc, what)

    def extract_matching(self):
        """{"size", "mate_row", "mate_col"}: int32 per row and per column, -1 for unmatched"""
        size, mr, mc = C.c_longlong(), _out(self.rows), _out(self.cols)
        _check(lib().grx_bipartite_extract_matching(self._h, _p(mr), _p(mc), C.byref(size)), "BipartiteProblem::ExtractMatching")
        return {"size": int(size.value), "mate_row": mr[:self.rows], "mate_col": mc[:self.cols]}

    def extract_parts(self):
        """(row_part, col_part, part_sizes): BIPARTITE_HORIZONTAL / _SQUARE / _VERTICAL as int32 per row and per column, and the
        six sizes: rows then columns in the three parts"""
        rp, cp, sizes = _out(self.rows), _out(self.cols), (C.c_longlong * 6)()
        self._refusing(lib().grx_bipartite_extract_parts(self._h, _p(rp), _p(cp), sizes), "BipartiteProblem::ExtractParts")
        return rp[:self.rows], cp[:self.cols], [int(x) for x in sizes]

    def extract_cover(self):
        """(row_cover, col_cover) as uint8: König's minimum vertex cover"""
        rc_, cc = _out(self.rows, np.uint8), _out(self.cols, np.uint8)
        self._refusing(lib().grx_bipartite_extract_cover(self._h, _u8p(rc_), _u8p(cc)), "BipartiteProblem::ExtractCover")
        return rc_[:self.rows], cc[:self.cols]

    def square_graph(self):
        """(k, arcs, d_row_offsets, d_col_indices, d_rows): the contracted square part in device memory, the handle's"""
        k, arcs, p = C.c_int(), C.c_int(), [C.c_void_p() for _ in range(3)]
        self._refusing(lib().grx_bipartite_square_graph(self._h, C.byref(k), C.byref(arcs), *map(C.byref, p)), "BipartiteProblem::SquareGraph")
        return (k.value, arcs.value) + tuple(x.value for x in p)

    def blocks(self):
        """(row_block, col_block, blocks): the fine decomposition.  The blocks are the strongly connected components of the
        contracted square part (SccProblem on the handle's device graph); a block's id is its smallest row, -1 outside the
        square part, and a column is in its mate row's block"""
        m = self.extract_matching()
        row_block, col_block = np.full(self.rows, -1, np.int32), np.full(self.cols, -1, np.int32)
        k, arcs, d_ro, d_ci, d_rows = self.square_graph()
        if k == 0:
            return row_block, col_block, 0
        scc = SccProblem(device=self._device).init_device(k, arcs, d_ro, d_ci)
        try:
            scc.reset()
            scc.enact()
            comp, count = scc.extract()
        finally:
            scc.close()
        rows = np.flatnonzero(self.extract_parts()[0] == BIPARTITE_SQUARE).astype(np.int32)  # local -> row: the square rows ascending
        row_block[rows] = rows[comp]
        col_block[m["mate_row"][rows]] = row_block[rows]
        return row_block, col_block, int(count)


def _problem(matrix, device):
    """an initialised problem over (shape, offsets, cols), or (offsets, cols) for a square matrix"""
    m = tuple(matrix)
    if len(m) not in (2, 3):
        raise ValueError("gunrockinst_amd: a matrix is (shape, offsets, cols) or (offsets, cols)")
    shape, ro, ci, _ = _matrix(m + (None,) if len(m) == 3 else m)
    return BipartiteProblem(device=device).init(shape, ro, ci)


def gunrock_bipartite_matching(matrix, device=0):
    """One-shot maximum matching of (shape, offsets, cols), or (offsets, cols) for a square one: {"size", "mate_row", "mate_col"}"""
    return _one_shot(_problem(matrix, device), BipartiteProblem.enact, BipartiteProblem.extract_matching)


def gunrock_structural_rank(matrix, device=0):
    """One-shot structural rank: the size of a maximum matching, an int"""
    return _one_shot(_problem(matrix, device), BipartiteProblem.enact, lambda p: int(p.stats()["size"]))


def gunrock_vertex_cover(matrix, device=0):
    """One-shot minimum vertex cover (König): (row_cover, col_cover) as uint8"""
    return _one_shot(_problem(matrix, device), BipartiteProblem.enact, BipartiteProblem.extract_cover)


def gunrock_dulmage_mendelsohn(matrix, fine=True, device=0):
    """One-shot Dulmage-Mendelsohn decomposition: {"size", "mate_row", "mate_col", "row_part", "col_part", "part_sizes",
    "row_cover", "col_cover"} and, with fine, {"row_block", "col_block", "blocks"}"""
    def result(p):
        out = p.extract_matching()
        out["row_part"], out["col_part"], out["part_sizes"] = p.extract_parts()
        out["row_cover"], out["col_cover"] = p.extract_cover()
        if fine:
            out["row_block"], out["col_block"], out["blocks"] = p.blocks()
        return out
    return _one_shot(_problem(matrix, device), BipartiteProblem.enact, result)
