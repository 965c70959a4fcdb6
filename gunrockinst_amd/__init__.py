"""gunrockinst_amd -- MI355X-native frontier engine (BFS / CC / SSSP / BC / PageRank / TopK / MST / MIS / TC / k-core / k-truss / SCC / MS-BFS / BCC / max-flow / matching / k-cliques / label propagation / 4-cycles) behind Gunrock's C ABI.

The product is the shared library ``gunrockinst_amd/lib/libgunrock.so`` (hand-written HIP for gfx950,
built by ``gunrockinst_amd/csrc/Makefile``).  This package is only the host-side binding: ctypes
mirrors of ``include/gunrock/gunrock.h`` and ``include/gunrock/gunrock_mi355x.h``.  There is no
CPU fallback: importing the binding without the built library raises.
"""
from .capi import (  # noqa: F401
    GunrockConfig, GunrockDataType, GunrockGraph, LIB_PATH, lib, build_library,
    VTXID_INT, SIZET_INT, VALUE_INT, VALUE_UINT, VALUE_FLOAT, SRC_MANUALLY, SRC_RANDOMIZE, SRC_LARGEST_DEGREE,
    HostGraph, BfsProblem, CcProblem, SsspProblem, BcProblem, PrProblem, gunrock_bfs, gunrock_cc, gunrock_sssp, gunrock_bc,
    gunrock_pr, gunrock_topk, version, filter_queue, MstProblem, gunrock_mst,
    MisProblem, gunrock_mis, gunrock_color, mis_priorities, MIS_SET, MIS_COLOR_ROUNDS, MIS_COLOR_FIRST_FIT,
    TcProblem, gunrock_tc, gunrock_clustering, TC_AUTO, TC_LANE, TC_LDS, TC_GLOBAL,
    KcoreProblem, gunrock_kcore, gunrock_kcore_members, KCORE_AUTO, KCORE_ROUNDS, KCORE_DEVICE_LOOP,
    TrussProblem, gunrock_truss, gunrock_edge_support, gunrock_ktruss, TRUSS_AUTO, TRUSS_ROUNDS,
    SccProblem, gunrock_scc, gunrock_condensation, SCC_AUTO, SCC_ROUNDS, SCC_DEVICE_LOOP, SCC_TRIM, SCC_PIVOT, SCC_COLOUR,
    MsbfsProblem, gunrock_msbfs, gunrock_closeness, gunrock_eccentricity, closeness_from_sums, MSBFS_AUTO, MSBFS_PUSH, MSBFS_PULL, MSBFS_ALTERNATE,
    MSBFS_INVERSE_AUTO, MSBFS_INVERSE_NONE, MSBFS_INVERSE_SELF, MSBFS_INVERSE_BUILD, MSBFS_LEVEL_PUSH, MSBFS_LEVEL_PULL,
    MSBFS_DEPTHS_NOT_STORED, MSBFS_INVERSE_NOT_SYMMETRIC,
    BccProblem, gunrock_bcc, gunrock_bridges, gunrock_articulation_points, BCC_AUTO, BCC_ROUNDS, BCC_DEVICE_LOOP,
    BCC_FOREST, BCC_SIZES, BCC_NUMBER, BCC_LOWHIGH, BCC_LINK, BCC_LABEL,
    MaxflowProblem, MaxflowGaveUp, gunrock_maxflow, gunrock_mincut, MAXFLOW_AUTO, MAXFLOW_ROUNDS, MAXFLOW_DEVICE_LOOP,
    MAXFLOW_PREFLOW, MAXFLOW_RETURN, MAXFLOW_CUT, MAXFLOW_GAVE_UP,
    MatchingProblem, MatchingGaveUp, MatchingOverflow, gunrock_matching, gunrock_coarsen, matching_keys, MATCHING_AUTO, MATCHING_ROUNDS,
    MATCHING_DEVICE_LOOP, MATCHING_STEP_WIDE, MATCHING_STEP_LOOP, MATCHING_GAVE_UP, MATCHING_OVERFLOW,
    BcOverflow, BC_OVERFLOW,
    CliqueProblem, CliqueOverflow, gunrock_cliques, CLIQUE_AUTO, CLIQUE_BITMAP, CLIQUE_LIST, CLIQUE_OVERFLOW,
    LpProblem, gunrock_label_propagation, modularity_from_sums, LP_SYNC, LP_CLASSES, LP_AUTO, LP_LANE, LP_WAVE, LP_BLOCK,
    LP_CONVERGED, LP_PERIOD2, LP_CAPPED, LP_BAD_CLASSES,
    C4Problem, C4Overflow, gunrock_four_cycles, gunrock_edge_four_cycles, C4_AUTO, C4_LANE, C4_WAVE, C4_BLOCK, C4_GLOBAL, C4_OVERFLOW,
    advance_frontier, advance_queue, advance_reduce,
)

__all__ = [
    "GunrockConfig", "GunrockDataType", "GunrockGraph", "LIB_PATH", "lib", "build_library",
    "HostGraph", "BfsProblem", "CcProblem", "SsspProblem", "BcProblem", "gunrock_bfs", "gunrock_cc", "gunrock_sssp",
    "gunrock_bc", "PrProblem", "gunrock_pr", "gunrock_topk", "version", "filter_queue", "MstProblem", "gunrock_mst",
    "MisProblem", "gunrock_mis", "gunrock_color", "mis_priorities", "MIS_SET", "MIS_COLOR_ROUNDS", "MIS_COLOR_FIRST_FIT",
    "TcProblem", "gunrock_tc", "gunrock_clustering", "TC_AUTO", "TC_LANE", "TC_LDS", "TC_GLOBAL",
    "KcoreProblem", "gunrock_kcore", "gunrock_kcore_members", "KCORE_AUTO", "KCORE_ROUNDS", "KCORE_DEVICE_LOOP",
    "TrussProblem", "gunrock_truss", "gunrock_edge_support", "gunrock_ktruss", "TRUSS_AUTO", "TRUSS_ROUNDS",
    "SccProblem", "gunrock_scc", "gunrock_condensation", "SCC_AUTO", "SCC_ROUNDS", "SCC_DEVICE_LOOP", "SCC_TRIM", "SCC_PIVOT", "SCC_COLOUR",
    "MsbfsProblem", "gunrock_msbfs", "gunrock_closeness", "gunrock_eccentricity", "closeness_from_sums", "MSBFS_AUTO", "MSBFS_PUSH", "MSBFS_PULL",
    "MSBFS_ALTERNATE", "MSBFS_INVERSE_AUTO", "MSBFS_INVERSE_NONE", "MSBFS_INVERSE_SELF", "MSBFS_INVERSE_BUILD", "MSBFS_LEVEL_PUSH", "MSBFS_LEVEL_PULL",
    "MSBFS_DEPTHS_NOT_STORED", "MSBFS_INVERSE_NOT_SYMMETRIC",
    "BccProblem", "gunrock_bcc", "gunrock_bridges", "gunrock_articulation_points", "BCC_AUTO", "BCC_ROUNDS", "BCC_DEVICE_LOOP", "BCC_FOREST", "BCC_SIZES", "BCC_NUMBER", "BCC_LOWHIGH", "BCC_LINK", "BCC_LABEL",
    "MaxflowProblem", "MaxflowGaveUp", "gunrock_maxflow", "gunrock_mincut", "MAXFLOW_AUTO", "MAXFLOW_ROUNDS", "MAXFLOW_DEVICE_LOOP", "MAXFLOW_PREFLOW",
    "MAXFLOW_RETURN", "MAXFLOW_CUT", "MAXFLOW_GAVE_UP",
    "MatchingProblem", "MatchingGaveUp", "MatchingOverflow", "gunrock_matching", "gunrock_coarsen", "matching_keys", "MATCHING_AUTO",
    "MATCHING_ROUNDS", "MATCHING_DEVICE_LOOP", "MATCHING_STEP_WIDE", "MATCHING_STEP_LOOP", "MATCHING_GAVE_UP", "MATCHING_OVERFLOW",
    "BcOverflow", "BC_OVERFLOW",
    "CliqueProblem", "CliqueOverflow", "gunrock_cliques", "CLIQUE_AUTO", "CLIQUE_BITMAP", "CLIQUE_LIST", "CLIQUE_OVERFLOW",
    "LpProblem", "gunrock_label_propagation", "modularity_from_sums", "LP_SYNC", "LP_CLASSES", "LP_AUTO", "LP_LANE", "LP_WAVE", "LP_BLOCK",
    "LP_CONVERGED", "LP_PERIOD2", "LP_CAPPED", "LP_BAD_CLASSES",
    "C4Problem", "C4Overflow", "gunrock_four_cycles", "gunrock_edge_four_cycles", "C4_AUTO", "C4_LANE", "C4_WAVE", "C4_BLOCK", "C4_GLOBAL",
    "C4_OVERFLOW",
    "advance_frontier", "advance_queue", "advance_reduce",
]
