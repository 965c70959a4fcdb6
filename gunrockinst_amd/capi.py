"""ctypes binding of libgunrock.so.

Struct layouts mirror include/gunrock/gunrock.h (reference gunrock/gunrock.h:51-99) field by field.
No compute happens in Python and nothing here falls back to a CPU implementation: if the HIP
library is missing, :func:`lib` raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# GUNROCK_LIB_PATH: another build of the same library (tuning variants from tools/build_variant.sh); still no fallback.
LIB_PATH = os.environ.get("GUNROCK_LIB_PATH") or os.path.join(_PKG, "lib", "libgunrock.so")
_LIB = None

# enum VertexIdType / SizeTType / ValueType / SrcMode (gunrock.h)
VTXID_INT = 0
SIZET_INT = 0
VALUE_INT, VALUE_UINT, VALUE_FLOAT = 0, 1, 2
SRC_MANUALLY, SRC_RANDOMIZE, SRC_LARGEST_DEGREE = 0, 1, 2

i32p = C.POINTER(C.c_int32)


class GunrockDataType(C.Structure):
    _fields_ = [("VTXID_TYPE", C.c_int), ("SIZET_TYPE", C.c_int), ("VALUE_TYPE", C.c_int)]


class GunrockGraph(C.Structure):
    _fields_ = [("num_nodes", C.c_size_t), ("num_edges", C.c_size_t),
                ("row_offsets", C.c_void_p), ("col_indices", C.c_void_p),
                ("col_offsets", C.c_void_p), ("row_indices", C.c_void_p),
                ("node_values", C.c_void_p), ("edge_values", C.c_void_p)]


class GunrockConfig(C.Structure):
    _fields_ = [("mark_pred", C.c_bool), ("idempotence", C.c_bool),
                ("src_node", C.c_int), ("device", C.c_int), ("max_iter", C.c_int),
                ("top_nodes", C.c_int), ("delta_factor", C.c_int),
                ("delta", C.c_float), ("error", C.c_float), ("queue_size", C.c_float),
                ("src_mode", C.c_int)]


def build_library(force=False):
    """Compile libgunrock.so for gfx950 (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_PKG, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src_dir, "clean"])
    subprocess.check_call(["make", "-C", src_dir, "-j8", "-s"])
    return LIB_PATH


# every symbol declared in include/gunrock/*.h (tests/test_capi_symbols.py checks the list against the headers)
_SIGNATURES = {
    "gunrock_bfs_func": (None, [C.POINTER(GunrockGraph), C.POINTER(GunrockGraph), GunrockConfig, GunrockDataType]),
    "gunrock_bc_func": (None, [C.POINTER(GunrockGraph), C.POINTER(GunrockGraph), GunrockConfig, GunrockDataType]),
    "gunrock_cc_func": (None, [C.POINTER(GunrockGraph), C.POINTER(GunrockGraph), GunrockConfig, GunrockDataType]),
    "gunrock_sssp_func": (None, [C.POINTER(GunrockGraph), C.c_void_p, C.POINTER(GunrockGraph), GunrockConfig,
                                 GunrockDataType]),
    "gunrock_pr_func": (None, [C.POINTER(GunrockGraph), C.c_void_p, C.c_void_p, C.POINTER(GunrockGraph),
                               GunrockConfig, GunrockDataType]),
    "gunrock_topk_func": (None, [C.POINTER(GunrockGraph), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(GunrockGraph), GunrockConfig, GunrockDataType]),
    "grx_graph_from_market": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "grx_graph_from_market_cached": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p)]),
    "grx_graph_rmat_libc": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.c_double] * 4 + [C.POINTER(C.c_void_p)]),
    "grx_graph_rmat_seeded": (C.c_int, [C.c_int, C.c_longlong, C.c_uint64, C.c_int] + [C.c_double] * 4 +
                              [C.POINTER(C.c_void_p)]),
    "grx_graph_from_coo": (C.c_int, [C.c_int, C.c_longlong, i32p, i32p, i32p, C.POINTER(C.c_void_p)]),
    "grx_graph_from_csr": (C.c_int, [C.c_int, C.c_int, i32p, i32p, i32p, C.POINTER(C.c_void_p)]),
    "grx_graph_nodes": (C.c_int, [C.c_void_p]),
    "grx_graph_edges": (C.c_int, [C.c_void_p]),
    "grx_graph_row_offsets": (i32p, [C.c_void_p]),
    "grx_graph_col_indices": (i32p, [C.c_void_p]),
    "grx_graph_edge_values": (i32p, [C.c_void_p]),
    "grx_graph_highest_degree_node": (C.c_int, [C.c_void_p, i32p]),
    "grx_graph_average_degree": (C.c_int, [C.c_void_p]),
    "grx_random_node": (C.c_int, [C.c_int]),
    "grx_graph_free": (None, [C.c_void_p]),
    "grx_rmat_seeded_device": (C.c_int, [C.c_int, C.c_longlong, C.c_longlong, C.c_uint64] + [C.c_double] * 4 +
                               [C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_coo_to_csr_sort": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_void_p]),
    "grx_coo_to_csr_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_coo_to_csr_free": (None, [C.c_void_p]),
    "grx_bc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "grx_bc_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_bc_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_bc_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_float)]),
    "grx_bc_extract": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_bc_destroy": (None, [C.c_void_p]),
    "grx_bfs_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "grx_bfs_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_bfs_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_bfs_set_inverse_graph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float]),
    "grx_bfs_auto_inverse": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "grx_bfs_set_tuning": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int]),
    "grx_bfs_set_persistent_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "grx_bfs_set_twc_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "grx_bfs_set_binned_min_edges": (C.c_int, [C.c_void_p, C.c_longlong]),
    "grx_bfs_set_label_deferral": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "grx_bfs_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_bfs_set_cooperative_launch": (C.c_int, [C.c_void_p, C.c_int]),
    "grx_bfs_set_head_pass": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "grx_bfs_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "grx_bfs_enact": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_bfs_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_bfs_level_trace": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                      C.POINTER(C.c_double), i32p]),
    "grx_bfs_extract": (C.c_int, [C.c_void_p, i32p, i32p]),
    "grx_bfs_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "grx_bfs_mask_flushes": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "grx_bfs_stream_idle": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "grx_bfs_fused_publications": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "grx_bfs_relabel_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int),
                                       C.POINTER(C.c_float), C.POINTER(C.c_longlong)]),
    "grx_bfs_destroy": (None, [C.c_void_p]),
    "grx_cc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_cc_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_cc_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_cc_reset": (C.c_int, [C.c_void_p]),
    "grx_cc_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_cc_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                               C.POINTER(C.c_double)]),
    "grx_cc_mirrored": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "grx_cc_sweep_edges": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "grx_cc_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_uint)]),
    "grx_cc_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "grx_cc_destroy": (None, [C.c_void_p]),
    "grx_mst_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_mst_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_mst_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_mst_reset": (C.c_int, [C.c_void_p]),
    "grx_mst_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_mst_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                C.POINTER(C.c_double)]),
    "grx_mst_round_trace": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_mst_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "grx_mst_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "grx_mst_destroy": (None, [C.c_void_p]),
    "grx_mis_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_mis_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p, C.c_uint]),
    "grx_mis_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]),
    "grx_mis_set_tail": (C.c_int, [C.c_void_p, C.c_int]),
    "grx_mis_reset": (C.c_int, [C.c_void_p]),
    "grx_mis_enact": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_mis_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_mis_round_trace": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_mis_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_longlong)]),
    "grx_mis_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "grx_mis_destroy": (None, [C.c_void_p]),
    "grx_tc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_tc_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_tc_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_tc_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_tc_reset": (C.c_int, [C.c_void_p]),
    "grx_tc_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_tc_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                               C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "grx_tc_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_tc_clustering": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "grx_tc_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "grx_tc_destroy": (None, [C.c_void_p]),
    "grx_kcore_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_kcore_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_kcore_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_kcore_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_kcore_reset": (C.c_int, [C.c_void_p]),
    "grx_kcore_enact": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_kcore_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 8 + [C.POINTER(C.c_double)] * 2),
    "grx_kcore_level_trace": (C.c_int, [C.c_void_p, C.c_int, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_kcore_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_int)]),
    "grx_kcore_shells": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]),
    "grx_kcore_members": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_kcore_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "grx_kcore_destroy": (None, [C.c_void_p]),
    "grx_truss_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_truss_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_truss_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_truss_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_truss_reset": (C.c_int, [C.c_void_p]),
    "grx_truss_enact": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_truss_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 10 + [C.POINTER(C.c_double)] * 3),
    "grx_truss_level_trace": (C.c_int, [C.c_void_p, C.c_int, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_truss_edges": (C.c_int, [C.c_void_p, i32p, i32p]),
    "grx_truss_support": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_longlong)]),
    "grx_truss_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_int)]),
    "grx_truss_classes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]),
    "grx_truss_members": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_truss_vertex_truss": (C.c_int, [C.c_void_p, i32p]),
    "grx_truss_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4),
    "grx_truss_destroy": (None, [C.c_void_p]),
    "grx_scc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_scc_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_scc_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_scc_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_scc_reset": (C.c_int, [C.c_void_p]),
    "grx_scc_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_scc_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 8 + [C.POINTER(C.c_double)] * 2),
    "grx_scc_phase_trace": (C.c_int, [C.c_void_p, C.c_int, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_scc_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_longlong)]),
    "grx_scc_summary": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 3 + [C.POINTER(C.c_int)]),
    "grx_scc_sizes": (C.c_int, [C.c_void_p, i32p]),
    "grx_scc_condensation": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p]),
    "grx_scc_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3),
    "grx_scc_destroy": (None, [C.c_void_p]),
    "grx_msbfs_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_msbfs_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_msbfs_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_msbfs_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_msbfs_reset": (C.c_int, [C.c_void_p, i32p, C.c_int, C.c_int]),
    "grx_msbfs_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_msbfs_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 6 + [C.POINTER(C.c_double)] * 2),
    "grx_msbfs_level_trace": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                        C.POINTER(C.c_double)]),
    "grx_msbfs_extract_depths": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p]),
    "grx_msbfs_source_summary": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), i32p]),
    "grx_msbfs_vertex_summary": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_longlong)]),
    "grx_msbfs_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 6),
    "grx_msbfs_destroy": (None, [C.c_void_p]),
    "grx_bcc_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_bcc_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_bcc_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_bcc_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_bcc_reset": (C.c_int, [C.c_void_p]),
    "grx_bcc_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_bcc_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 6 + [C.POINTER(C.c_double)] * 2),
    "grx_bcc_phase_trace": (C.c_int, [C.c_void_p, C.c_int, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_bcc_edges": (C.c_int, [C.c_void_p, i32p, i32p]),
    "grx_bcc_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), i32p, i32p]),
    "grx_bcc_summary": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 4 + [C.POINTER(C.c_int)] + [C.POINTER(C.c_longlong)] * 2 +
                        [C.POINTER(C.c_int)]),
    "grx_bcc_block_cut": (C.c_int, [C.c_void_p, C.c_int, i32p, i32p]),
    "grx_bcc_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 8),
    "grx_bcc_destroy": (None, [C.c_void_p]),
    "grx_maxflow_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_maxflow_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_maxflow_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_maxflow_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_maxflow_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "grx_maxflow_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_maxflow_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 8 + [C.POINTER(C.c_double)] * 2),
    "grx_maxflow_phase_trace": (C.c_int, [C.c_void_p, C.c_int, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_maxflow_pairs": (C.c_longlong, [C.c_void_p, i32p, i32p, i32p, i32p]),
    "grx_maxflow_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), i32p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "grx_maxflow_arc_flow": (C.c_int, [C.c_void_p, i32p]),
    "grx_maxflow_summary": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "grx_maxflow_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 7),
    "grx_maxflow_destroy": (None, [C.c_void_p]),
    "grx_matching_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_matching_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p, C.c_uint]),
    "grx_matching_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint]),
    "grx_matching_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_matching_reset": (C.c_int, [C.c_void_p]),
    "grx_matching_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_matching_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 6 + [C.POINTER(C.c_double)] * 2),
    "grx_matching_round_trace": (C.c_int, [C.c_void_p, C.c_int, i32p] + [C.POINTER(C.c_longlong)] * 3),
    "grx_matching_pairs": (C.c_longlong, [C.c_void_p, i32p, i32p, i32p]),
    "grx_matching_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte), i32p, i32p]),
    "grx_matching_summary": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "grx_matching_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 6),
    "grx_matching_contract": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_matching_coarse_extract": (C.c_int, [C.c_void_p, i32p, i32p, i32p, i32p, i32p]),
    "grx_matching_coarse_device": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 5),
    "grx_matching_destroy": (None, [C.c_void_p]),
    "grx_clique_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_clique_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_clique_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_clique_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_clique_reset": (C.c_int, [C.c_void_p]),
    "grx_clique_enact": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_clique_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 6 + [C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
                         + [C.POINTER(C.c_double)] * 2),
    "grx_clique_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_clique_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "grx_clique_destroy": (None, [C.c_void_p]),
    "grx_c4_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_c4_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_c4_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_c4_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_c4_reset": (C.c_int, [C.c_void_p]),
    "grx_c4_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_c4_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 5 + [C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
                     + [C.POINTER(C.c_double)] * 2),
    "grx_c4_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_c4_edges": (C.c_int, [C.c_void_p, i32p, i32p]),
    "grx_c4_extract_edges": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "grx_c4_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4),
    "grx_c4_destroy": (None, [C.c_void_p]),
    "grx_rw_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_rw_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_rw_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_rw_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_rw_reset": (C.c_int, [C.c_void_p, C.c_int, i32p]),
    "grx_rw_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_rw_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 6 + [C.POINTER(C.c_double)] * 2),
    "grx_rw_extract": (C.c_int, [C.c_void_p, i32p, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_rw_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_longlong)]),
    "grx_rw_destroy": (None, [C.c_void_p]),
    "grx_sample_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_sample_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_sample_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_sample_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_sample_set_fanouts": (C.c_int, [C.c_void_p, C.c_int, i32p]),
    "grx_sample_reset": (C.c_int, [C.c_void_p, C.c_int, i32p]),
    "grx_sample_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_sample_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)] + [C.POINTER(C.c_longlong)] * 6 + [C.POINTER(C.c_double)] * 3),
    "grx_sample_sizes": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 4),
    "grx_sample_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_longlong), i32p, i32p]),
    "grx_sample_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4),
    "grx_sample_destroy": (None, [C.c_void_p]),
    "grx_sim_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_sim_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_sim_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_sim_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_sim_reset": (C.c_int, [C.c_void_p]),
    "grx_sim_pairs": (C.c_int, [C.c_void_p, C.c_longlong, i32p, i32p, C.c_int, C.POINTER(C.c_float)]),
    "grx_sim_pairs_device": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_sim_topk": (C.c_int, [C.c_void_p, C.c_longlong, i32p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_sim_topk_device": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_sim_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 9 + [C.POINTER(C.c_double)] * 2),
    "grx_sim_extract_pairs": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_sim_extract_topk": (C.c_int, [C.c_void_p, i32p, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_double), i32p,
                                       i32p]),
    "grx_sim_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 9),
    "grx_sim_destroy": (None, [C.c_void_p]),
    "grx_spgemm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_spgemm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_spgemm_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_spgemm_set_right": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_spgemm_set_right_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_spgemm_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_spgemm_reset": (C.c_int, [C.c_void_p]),
    "grx_spgemm_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_spgemm_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 7 + [C.POINTER(C.c_double)] * 3),
    "grx_spgemm_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "grx_spgemm_extract": (C.c_int, [C.c_void_p, i32p, i32p, C.POINTER(C.c_longlong)]),
    "grx_spgemm_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3),
    "grx_spgemm_destroy": (None, [C.c_void_p]),
    "grx_bipartite_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_bipartite_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, i32p]),
    "grx_bipartite_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_bipartite_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_bipartite_reset": (C.c_int, [C.c_void_p, i32p]),
    "grx_bipartite_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_bipartite_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 12 + [C.POINTER(C.c_double)] * 2),
    "grx_bipartite_phase_trace": (C.c_int, [C.c_void_p, C.c_int, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "grx_bipartite_extract_matching": (C.c_int, [C.c_void_p, i32p, i32p, C.POINTER(C.c_longlong)]),
    "grx_bipartite_extract_parts": (C.c_int, [C.c_void_p, i32p, i32p, C.POINTER(C.c_longlong)]),
    "grx_bipartite_extract_cover": (C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]),
    "grx_bipartite_square_graph": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.POINTER(C.c_void_p)] * 3),
    "grx_bipartite_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 6),
    "grx_bipartite_destroy": (None, [C.c_void_p]),
    "grx_sm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_sm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_sm_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_sm_set_pattern": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p, C.c_int]),
    "grx_sm_pattern_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), i32p, C.POINTER(C.c_int), i32p, i32p]),
    "grx_sm_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_sm_reset": (C.c_int, [C.c_void_p]),
    "grx_sm_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_sm_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 9 + [C.POINTER(C.c_double)] * 7),
    "grx_sm_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_sm_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "grx_sm_destroy": (None, [C.c_void_p]),
    "grx_lp_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_lp_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, i32p]),
    "grx_lp_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_lp_set_classes": (C.c_int, [C.c_void_p, i32p, C.c_int]),
    "grx_lp_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_lp_reset": (C.c_int, [C.c_void_p, i32p]),
    "grx_lp_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_lp_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 9 + [C.POINTER(C.c_double)] * 2),
    "grx_lp_round_trace": (C.c_int, [C.c_void_p, C.c_int] + [C.POINTER(C.c_longlong)] * 2),
    "grx_lp_extract": (C.c_int, [C.c_void_p, i32p, i32p, C.POINTER(C.c_longlong)]),
    "grx_lp_summary": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 4),
    "grx_lp_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "grx_lp_destroy": (None, [C.c_void_p]),
    "grx_wl_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int]),
    "grx_wl_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_wl_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_wl_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_wl_reset": (C.c_int, [C.c_void_p, i32p]),
    "grx_wl_enact": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "grx_wl_stats": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_longlong)] * 10 + [C.POINTER(C.c_double)]),
    "grx_wl_round_trace": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]),
    "grx_wl_extract": (C.c_int, [C.c_void_p, i32p, C.POINTER(C.c_longlong), i32p, C.POINTER(C.c_longlong)]),
    "grx_wl_history": (C.c_int, [C.c_void_p, C.c_int, i32p, C.POINTER(C.c_longlong)]),
    "grx_wl_device_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3),
    "grx_wl_destroy": (None, [C.c_void_p]),
    "grx_sssp_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]),
    "grx_sssp_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p, C.POINTER(C.c_uint32), C.c_int]),
    "grx_sssp_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]),
    "grx_sssp_set_inverse_graph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]),
    "grx_sssp_pull_levels": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)]),
    "grx_filter_queue": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                   C.POINTER(C.c_longlong), C.c_int]),
    "grx_advance_queue": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.c_int]),
    "grx_advance_reduce": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 7 + [C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int]),
    "grx_device_scan": (C.c_int, [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "grx_device_key_sort": (C.c_int, [C.c_int, C.POINTER(C.c_longlong), i32p, C.c_void_p, C.c_void_p]),
    "grx_device_transpose": (C.c_int, [C.c_int, C.c_longlong] + [C.c_void_p] * 6),
    "grx_wave_ops": (C.c_int, [C.c_int] * 4 + [C.c_longlong] + [C.c_void_p] * 4),
    "grx_bisect_queue": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.c_int]),
    "grx_sssp_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "grx_sssp_enact": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_sssp_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                 C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.POINTER(C.c_float)]),
    "grx_sssp_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), i32p]),
    "grx_sssp_destroy": (None, [C.c_void_p]),
    "grx_pr_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "grx_pr_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, i32p, i32p]),
    "grx_pr_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_pr_set_inverse_graph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "grx_pr_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "grx_pr_enact": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "grx_pr_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_pr_extract": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), i32p, C.c_int]),
    "grx_pr_device_results": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "grx_pr_destroy": (None, [C.c_void_p]),
    "grx_pbfs_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "grx_pbfs_init_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grx_pbfs_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "grx_pbfs_frontier": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "grx_pbfs_advance_local": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]),
    "grx_pbfs_filter_received": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "grx_pbfs_queue_to_bitmap": (C.c_int, [C.c_void_p]),
    "grx_pbfs_frontier_bitmap": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "grx_pbfs_bottom_up": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "grx_pbfs_bitmap_to_queue": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "grx_pbfs_labels": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "grx_pbfs_preds": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "grx_pbfs_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double]),
    "grx_pbfs_stat": (C.c_longlong, [C.c_void_p, C.c_char_p]),
    "grx_rccl_load": (C.c_int, []),
    "grx_rccl_unique_id": (C.c_int, [C.c_char_p]),
    "grx_pbfs_comm_init_rccl": (C.c_int, [C.c_void_p, C.c_char_p]),
    "grx_pbfs_set_transport": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grx_pbfs_set_options": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "grx_pbfs_search": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "grx_pbfs_destroy": (None, [C.c_void_p]),
    "grx_bfs_count_visited": (None, [C.c_int, i32p, i32p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "grx_version": (C.c_char_p, []),
}


def lib():
    """Load libgunrock.so (once).  Raises if the HIP library has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "gunrockinst_amd: %s is missing -- build it with `make -C gunrockinst_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def exported_symbols():
    return sorted(_SIGNATURES)


def version():
    return lib().grx_version().decode()


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("gunrockinst_amd: %s failed (code %d)" % (what, rc))


def _p(a):
    return a.ctypes.data_as(i32p)


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_ubyte))


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


_POINTER_OF = {"int32": _p, "int64": _i64p, "uint8": _u8p, "float64": _f64p, "float32": _f32p}


def _opt(a):
    """None, or the pointer of a's element type"""
    return None if a is None else _POINTER_OF[a.dtype.name](a)


def _out(n, dtype=np.int32, wanted=True):
    """An output array for n entries (never of size 0: the library gets a valid pointer), or None when it is not wanted"""
    return np.empty(max(n, 1), dtype=dtype) if wanted else None


def _cut(a, n):
    """An output array cut back to its n entries; None stays None"""
    return None if a is None else a[:n]


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _i32_of(values, count, what, of):
    """None, or `values` as contiguous int32 once there are `count` of them: one per entry, per node, ..."""
    if values is None:
        return None
    a = _i32(values)
    if a.shape[0] != count:
        raise ValueError("gunrockinst_amd: %d %s for %d %s" % (a.shape[0], what, count, of))
    return a


def _count_then_fill(fn, h, what, dtypes, negated=False):
    """The columns of a trace or a list behind `fn(h, capacity, *columns)`: asks for the count with no columns, allocates one
    column per dtype, has them filled and returns them cut to the count.  A negative count raises.  The library has two
    conventions and `negated` picks the family's: the traces return a code, reported as it is, and their fill cannot fail; the
    lists (negated) return minus the code -- the message shows the positive number -- and their fill is checked the same way."""
    count = fn(h, 0, *[None] * len(dtypes))
    if count < 0:
        _check(-count if negated else count, what)
    columns = [_out(count, dtype) for dtype in dtypes]
    rc = fn(h, count, *[_opt(c) for c in columns])
    if negated and rc < 0:
        _check(-rc, what)
    return tuple(c[:count] for c in columns)


_TRACE = (np.int32, np.int64, np.float64)  # the columns of a level or phase trace: (k or kind, items, milliseconds)


def _pair_list(fn, h, what, max_edges):
    """(first, second, count) of a sorted int32 pair list behind `fn(h, capacity, first, second)`; max_edges caps what is copied
    (None: all, 0: the count only).  Codes come negated, as in the lists of _count_then_fill."""
    count = fn(h, 0, None, None)
    if count < 0:
        _check(-count, what)
    take = count if max_edges is None else min(count, int(max_edges))
    a, b = _out(take), _out(take)
    if take > 0:
        rc = fn(h, take, _p(a), _p(b))
        if rc < 0:
            _check(-rc, what)
    return a[:take], b[:take], count


def _check_offsets(row_offsets, nodes):
    if row_offsets.shape[0] != int(nodes) + 1:
        raise ValueError("gunrockinst_amd: %d row offsets for %d nodes" % (row_offsets.shape[0], int(nodes)))


def _csr_arrays(row_offsets, col_indices, nodes=None):
    """The two CSR arrays as contiguous int32; with `nodes`, the offsets must have nodes + 1 entries."""
    ro, ci = _i32(row_offsets), _i32(col_indices)
    if nodes is not None:
        _check_offsets(ro, nodes)
    return ro, ci


class _Handle:
    """Owner of one library handle `_h`; a subclass names the symbol that destroys it."""

    _destroy = None

    def _create(self, symbol, *args):
        self._h = C.c_void_p()
        _check(getattr(lib(), symbol)(C.byref(self._h), *args), symbol)

    def _timed(self, fn, what, *args):
        """a library call whose last argument receives the elapsed milliseconds"""
        ms = C.c_float()
        _check(fn(self._h, *args, C.byref(ms)), what)
        return float(ms.value)

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Problem(_Handle):
    """One family of the handle C ABI, grx_<family>_*: the Python counterpart of handle_runner.hpp.  A subclass declares

      _family              "tc" for grx_tc_*
      _problem, _enactor   the names in messages: "TCProblem", "TCEnactor"
      _count               the attribute that holds the number of CSR entries: "edges" or "entries" (None: not kept)
      _stats               (int64 fields, double fields) in the order of grx_<family>_stats.  An int64 field is a name, a
                           (name, n) pair for an array of n kept as a list, or a tuple of names for an array spread over keys
      _results             the names of grx_<family>_device_results' pointers (device_results returns a dict), or their
                           number (a tuple)

    and writes: init / init_device where Init has trailing arguments, as one call of _init_host / _init_device; _ready() for
    what has to be read back behind either; its extract methods; and any phase whose signature or return codes are its own.
    reset, enact and run of the five benchmarked classes sit in the benchmark's timing loops and name their symbols directly,
    lib().grx_bfs_enact: nothing is looked up by name there."""

    _family = _problem = _enactor = None
    _count = "edges"
    _check_rows = True  # False: the classes that mirror the reference's Init, which takes the offsets as they come
    _stats = ((), ())
    _results = 0

    def __init__(self, instrument=False, device=0):
        self._create("grx_%s_create" % self._family, int(instrument), device)
        self._sized(0, 0)

    def _fn(self, phase):
        return getattr(lib(), "grx_%s_%s" % (self._family, phase))

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def _sized(self, nodes, entries):
        self.nodes = int(nodes)
        if self._count:
            setattr(self, self._count, int(entries))
        return self.nodes, int(entries)

    def _ready(self):
        """called behind a successful Init: what a family reads back once (the number of its canonical edges, ...)"""

    def _init_host(self, nodes, row_offsets, col_indices, *extra, per_entry=None, per_node=None):
        """Init from host arrays.  per_entry = (values or None, "weights", "entries"): the family's optional int32 array with
        one value per CSR entry and the words of its length check; it follows the column indices.  per_node = (values or None,
        "ranks", "nodes"): the same with one value per vertex; it comes next.  `extra` are the trailing arguments.  The checks
        run in this order: row offsets, per_entry, per_node."""
        ro, ci = _csr_arrays(row_offsets, col_indices, nodes if self._check_rows else None)
        args = [_p(ro), _p(ci)]
        if per_entry is not None:
            args.append(_opt(_i32_of(per_entry[0], ci.shape[0], *per_entry[1:])))
        if per_node is not None:
            args.append(_opt(_i32_of(per_node[0], int(nodes), *per_node[1:])))
        _check(self._fn("init")(self._h, *self._sized(nodes, ci.shape[0]), *args, *extra), self._problem + "::Init")
        self._ready()
        return self

    def _init_device(self, nodes, edges, d_row_offsets, d_col_indices, *extra):
        """Init from a CSR in device memory: integer addresses (torch.Tensor.data_ptr()), borrowed.  An address among `extra`
        goes through C.c_void_p, for which None and 0 are the null pointer."""
        _check(self._fn("init_device")(self._h, *self._sized(nodes, edges), C.c_void_p(d_row_offsets), C.c_void_p(d_col_indices), *extra),
               self._problem + "::Init(device)")
        self._ready()
        return self

    def init(self, nodes, row_offsets, col_indices):
        return self._init_host(nodes, row_offsets, col_indices)

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices):
        """d_* are integer device addresses (e.g. torch.Tensor.data_ptr()); borrowed: see the class for how long they are read"""
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices)

    def reset(self):
        _check(self._fn("reset")(self._h), self._problem + "::Reset")

    def _reset_labels(self, labels):
        """Reset of the families that start from optional int32 labels, one per vertex"""
        _check(self._fn("reset")(self._h, _opt(_i32_of(labels, self.nodes, "labels", "nodes"))), self._problem + "::Reset")

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds"""
        return self._timed(self._fn("enact"), self._enactor + "::Enact", int(max_grid_size))

    def stats(self):
        ints, doubles = self._stats
        slots = [C.c_longlong() if isinstance(f, str) else (C.c_longlong * (f[1] if isinstance(f[1], int) else len(f)))() for f in ints]
        ms = [C.c_double() for _ in doubles]
        _check(self._fn("stats")(self._h, *[C.byref(s) if isinstance(f, str) else s for f, s in zip(ints, slots)], *map(C.byref, ms)),
               "grx_%s_stats" % self._family)
        out = {}
        for f, s in zip(ints, slots):
            if isinstance(f, str):
                out[f] = s.value
            elif isinstance(f[1], int):
                out[f[0]] = [int(x) for x in s]
            else:
                out.update(zip(f, (int(x) for x in s)))
        out.update((name, x.value) for name, x in zip(doubles, ms))
        return out

    def _device_pointers(self, count, phase="device_results"):
        p = [C.c_void_p() for _ in range(count)]
        _check(self._fn(phase)(self._h, *map(C.byref, p)), "grx_%s_%s" % (self._family, phase))
        return [x.value for x in p]

    def device_results(self):
        """the device pointers of the results, which live as long as the handle: see the class for their names or order"""
        if isinstance(self._results, int):
            return tuple(self._device_pointers(self._results))
        return dict(zip(self._results, self._device_pointers(len(self._results))))


class _TunedProblem(_Problem):
    """A family with grx_<family>_set_option; its class docstring lists the names."""

    def set_option(self, name, value):
        """returns the library's code: 0 = set, 1 = unknown name (a value out of range raises)"""
        rc = self._fn("set_option")(self._h, name.encode(), float(value))
        if rc not in (0, 1):
            _check(rc, "grx_%s_set_option(%s)" % (self._family, name))
        return rc


def _one_shot(problem, *steps):
    """Runs the steps on an initialised problem, closes it whatever happens and returns what the last step returned."""
    try:
        for step in steps[:-1]:
            step(problem)
        return steps[-1](problem)
    finally:
        problem.close()


class HostGraph(_Handle):
    """gunrock::Csr<int,int,int> built by the library's own host graph code."""

    _destroy = "grx_graph_free"

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        L = lib()
        self.nodes = L.grx_graph_nodes(self._h)
        self.edges = L.grx_graph_edges(self._h)

    @classmethod
    def from_market(cls, path, undirected=False, reversed_=False, cache=False):
        """cache=True: the reference's CSR cache rule with a binary, stamped cache file next to the input; the instance's
        `cache_hit` tells whether the graph came from it."""
        h = C.c_void_p()
        if cache:
            hit = C.c_int()
            _check(lib().grx_graph_from_market_cached(os.fsencode(path), int(undirected), int(reversed_), C.byref(hit), C.byref(h)),
                   "BuildMarketGraphCached(%s)" % path)
            g = cls(h.value)
            g.cache_hit = bool(hit.value)
            return g
        _check(lib().grx_graph_from_market(os.fsencode(path), int(undirected), int(reversed_), C.byref(h)),
               "BuildMarketGraph(%s)" % path)
        return cls(h.value)

    @classmethod
    def rmat_libc(cls, nodes, edges, undirected=False, a=0.55, b=0.2, c=0.2, d=0.05):
        h = C.c_void_p()
        _check(lib().grx_graph_rmat_libc(nodes, edges, int(undirected), a, b, c, d, C.byref(h)), "BuildRmatGraph")
        return cls(h.value)

    @classmethod
    def rmat_seeded(cls, scale, pairs, seed=0x6772, undirected=True, a=0.55, b=0.2, c=0.2, d=0.05):
        h = C.c_void_p()
        _check(lib().grx_graph_rmat_seeded(scale, pairs, seed, int(undirected), a, b, c, d, C.byref(h)),
               "BuildSeededRmatGraph")
        return cls(h.value)

    @classmethod
    def from_coo(cls, nodes, rows, cols, vals=None):
        rows = _i32(rows)
        cols = _i32(cols)
        v = None if vals is None else _i32(vals)
        h = C.c_void_p()
        _check(lib().grx_graph_from_coo(nodes, rows.shape[0], _p(rows), _p(cols), None if v is None else _p(v),
                                        C.byref(h)), "Csr::FromCoo")
        return cls(h.value)

    @classmethod
    def from_csr(cls, nodes, row_offsets, col_indices, edge_values=None):
        ro, ci = _csr_arrays(row_offsets, col_indices)
        ev = None if edge_values is None else _i32(edge_values)
        h = C.c_void_p()
        _check(lib().grx_graph_from_csr(nodes, ci.shape[0], _p(ro), _p(ci), None if ev is None else _p(ev),
                                        C.byref(h)), "grx_graph_from_csr")
        return cls(h.value)

    @property
    def row_offsets(self):
        return np.ctypeslib.as_array(lib().grx_graph_row_offsets(self._h), shape=(self.nodes + 1,))

    @property
    def col_indices(self):
        if self.edges == 0:
            return np.empty(0, dtype=np.int32)
        return np.ctypeslib.as_array(lib().grx_graph_col_indices(self._h), shape=(self.edges,))

    @property
    def edge_values(self):
        p = lib().grx_graph_edge_values(self._h)
        if not p or self.edges == 0:
            return None
        return np.ctypeslib.as_array(p, shape=(self.edges,))

    def highest_degree_node(self):
        md = C.c_int32()
        v = lib().grx_graph_highest_degree_node(self._h, C.byref(md))
        return int(v), int(md.value)

    def average_degree(self):
        return int(lib().grx_graph_average_degree(self._h))


class BfsProblem(_Problem):
    """BFSProblem + BFSEnactor behind the handle C ABI (Init once, Reset + Enact per run, Extract).  reset and enact are timed
    by the benchmark and name their symbols directly; device_results: (labels, predecessors).  The arrays given to init_device
    are borrowed for every search and must outlive the problem."""

    _family, _problem, _enactor = "bfs", "BFSProblem", "BFSEnactor"
    _count, _check_rows = None, False
    _results = 2

    def __init__(self, mark_pred=False, idempotence=False, instrument=False, device=0):
        self.mark_pred = bool(mark_pred)
        self._create("grx_bfs_create", int(mark_pred), int(idempotence), int(instrument), device)
        self.nodes = 0

    def set_inverse_graph(self, d_inv_row_offsets=None, d_inv_col_indices=None, alpha=0.0, beta=0.0):
        """Enable traversal_mode=2 (direction-optimizing).  No arguments = the graph is symmetric."""
        _check(lib().grx_bfs_set_inverse_graph(self._h, C.c_void_p(d_inv_row_offsets), C.c_void_p(d_inv_col_indices),
                                               alpha, beta), "BFSProblem::SetInverseGraph")
        return self

    def auto_inverse(self, build_if_directed=True):
        """What gunrock_bfs_func does before its search: symmetric graph -> its own inverse; directed -> transpose built on the
        device (owned by the handle).  Returns (enabled, built, build_ms)."""
        on, made, ms = C.c_int(), C.c_int(), C.c_float()
        _check(lib().grx_bfs_auto_inverse(self._h, int(bool(build_if_directed)), C.byref(on), C.byref(made), C.byref(ms)),
               "grx_bfs_auto_inverse")
        return bool(on.value), bool(made.value), float(ms.value)

    def set_tuning(self, alpha=0.0, beta=0.0, lite_factor=-1.0, tail_edge_limit=-1):
        _check(lib().grx_bfs_set_tuning(self._h, alpha, beta, lite_factor, tail_edge_limit), "grx_bfs_set_tuning")
        return self

    def set_head_pass(self, min_edges=-1, max_edges=-1):
        _check(lib().grx_bfs_set_head_pass(self._h, int(min_edges), int(max_edges)), "grx_bfs_set_head_pass")
        return self

    def set_option(self, name, value):
        """Named enactor tuning knob (include/gunrock/gunrock_mi355x.h grx_bfs_set_option); results never depend on them."""
        _check(lib().grx_bfs_set_option(self._h, name.encode(), float(value)), "grx_bfs_set_option(%s)" % name)
        return self

    def set_label_deferral(self, enabled=-1, mask_limit=0):
        """Deferred labels of direction-optimizing searches (one emit pass at the end of Enact); effective at the next reset."""
        _check(lib().grx_bfs_set_label_deferral(self._h, int(enabled), int(mask_limit)), "grx_bfs_set_label_deferral")
        return self

    def set_binned_min_edges(self, min_edges):
        _check(lib().grx_bfs_set_binned_min_edges(self._h, int(min_edges)), "grx_bfs_set_binned_min_edges")
        return self

    def set_cooperative_launch(self, on=True):
        _check(lib().grx_bfs_set_cooperative_launch(self._h, int(bool(on))), "grx_bfs_set_cooperative_launch")
        return self

    def set_persistent_limit(self, edge_limit):
        _check(lib().grx_bfs_set_persistent_limit(self._h, int(edge_limit)), "grx_bfs_set_persistent_limit")
        return self

    def set_twc_limit(self, edge_limit):
        _check(lib().grx_bfs_set_twc_limit(self._h, int(edge_limit)), "grx_bfs_set_twc_limit")
        return self

    def reset(self, src, queue_sizing=1.0):
        _check(lib().grx_bfs_reset(self._h, int(src), float(queue_sizing)), "BFSProblem::Reset")

    def enact(self, src, max_grid_size=0, traversal_mode=0):
        return self._timed(lib().grx_bfs_enact, "BFSEnactor::Enact", int(src), max_grid_size, traversal_mode)

    def stats(self):
        q, d, l = C.c_longlong(), C.c_longlong(), C.c_longlong()
        duty, kms = C.c_double(), C.c_double()
        _check(lib().grx_bfs_stats(self._h, C.byref(q), C.byref(d), C.byref(duty), C.byref(l), C.byref(kms)),
               "BFSEnactor::GetStatistics")
        return {"total_queued": q.value, "search_depth": d.value, "avg_duty": duty.value,
                "kernel_launches": l.value, "kernel_ms": kms.value}

    def level_trace(self, max_levels=4096):
        fr = (C.c_longlong * max_levels)()
        ed = (C.c_longlong * max_levels)()
        ms = (C.c_double * max_levels)()
        kd = (C.c_int32 * max_levels)()
        n = lib().grx_bfs_level_trace(self._h, max_levels, fr, ed, ms, kd)
        n = min(max(n, 0), max_levels)
        return [{"frontier": fr[i], "edges": ed[i], "ms": ms[i], "kind": kd[i]} for i in range(n)]

    def extract(self):
        labels, preds = _out(self.nodes), _out(self.nodes, wanted=self.mark_pred)
        _check(lib().grx_bfs_extract(self._h, _p(labels), _opt(preds)), "BFSProblem::Extract")
        return labels[:self.nodes], _cut(preds, self.nodes)

    def mask_flushes(self):
        """kept level bitmaps flushed into the labels in the middle of a search, over the handle's life"""
        v = C.c_longlong()
        _check(lib().grx_bfs_mask_flushes(self._h, C.byref(v)), "grx_bfs_mask_flushes")
        return v.value

    def fused_publications(self):
        """read-backs a label pass published for the enactor (option fused_publish), over the handle's life"""
        v = C.c_longlong()
        _check(lib().grx_bfs_fused_publications(self._h, C.byref(v)), "grx_bfs_fused_publications")
        return v.value

    def stream_idle(self):
        """True when nothing is queued or running on the handle's stream (always so right after enact)"""
        v = C.c_int()
        _check(lib().grx_bfs_stream_idle(self._h, C.byref(v)), "grx_bfs_stream_idle")
        return bool(v.value)

    def relabel_info(self):
        """The relabelled copy of a symmetric problem: hub-tier size (-1 = no copy), vertices with edges, hub degree
        threshold, build milliseconds, device bytes."""
        h, we, t, ms, b = C.c_longlong(), C.c_longlong(), C.c_int(), C.c_float(), C.c_longlong()
        _check(lib().grx_bfs_relabel_info(self._h, C.byref(h), C.byref(we), C.byref(t), C.byref(ms), C.byref(b)),
               "grx_bfs_relabel_info")
        return {"hubs": h.value, "with_edges": we.value, "threshold": t.value, "build_ms": ms.value, "bytes": b.value}


def _graph_struct(nodes, row_offsets, col_indices, edge_values=None):
    g = GunrockGraph()
    g.num_nodes = nodes
    g.num_edges = col_indices.shape[0]
    g.row_offsets = row_offsets.ctypes.data
    g.col_indices = col_indices.ctypes.data
    g.edge_values = None if edge_values is None else edge_values.ctypes.data
    return g


def _take_node_values(gout, nodes, dtype):
    """graph_out->node_values is malloc()ed by the library and owned by the caller (bfs_app.cu:211)."""
    ptr = gout.node_values
    if not ptr:
        raise RuntimeError("gunrockinst_amd: the call produced no node_values")
    arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(max(nodes, 1),))[:nodes].copy()
    C.CDLL(None).free(C.c_void_p(ptr))
    return arr.view(dtype)


def gunrock_bfs(nodes, row_offsets, col_indices, src=0, mark_pred=False, idempotence=False, queue_size=1.0,
                src_mode=SRC_MANUALLY, device=0):
    """Call gunrock_bfs_func exactly as reference shared_lib_tests/test_bfs.c does; returns the labels."""
    ro, ci = _csr_arrays(row_offsets, col_indices)
    gin = _graph_struct(nodes, ro, ci)
    gout = GunrockGraph()
    cfg = GunrockConfig()
    cfg.mark_pred, cfg.idempotence = mark_pred, idempotence
    cfg.src_node, cfg.device, cfg.queue_size, cfg.src_mode = src, device, queue_size, src_mode
    dt = GunrockDataType(VTXID_INT, SIZET_INT, VALUE_INT)
    lib().gunrock_bfs_func(C.byref(gout), C.byref(gin), cfg, dt)
    return _take_node_values(gout, nodes, np.int32)


class CcProblem(_Problem):
    """CCProblem + CCEnactor behind the handle C ABI.  reset and enact are timed by the benchmark and name their symbols
    directly."""

    _family, _problem, _enactor = "cc", "CCProblem", "CCEnactor"
    _count, _check_rows = None, False
    _stats = (("edge_sweeps", "vertex_sweeps", "kernel_launches"), ("kernel_ms",))

    def reset(self):
        _check(lib().grx_cc_reset(self._h), "CCProblem::Reset")

    def enact(self, max_grid_size=0):
        return self._timed(lib().grx_cc_enact, "CCEnactor::Enact", max_grid_size)

    def stats(self):
        out = super().stats()
        mir, se = C.c_int(), C.c_longlong()
        _check(lib().grx_cc_mirrored(self._h, C.byref(mir)), "grx_cc_mirrored")
        _check(lib().grx_cc_sweep_edges(self._h, C.byref(se)), "grx_cc_sweep_edges")
        out["mirrored"], out["sweep_edges"] = bool(mir.value), se.value
        return out

    def extract(self):
        ids, nc = _out(self.nodes), C.c_uint()
        _check(lib().grx_cc_extract(self._h, _p(ids), C.byref(nc)), "CCProblem::Extract")
        return ids[:self.nodes], int(nc.value)

    def device_results(self):
        """the device pointer of the component ids"""
        return self._device_pointers(1)[0]


def gunrock_cc(nodes, row_offsets, col_indices, device=0):
    """Call gunrock_cc_func as reference shared_lib_tests/test_cc.c does; returns the component ids."""
    ro, ci = _csr_arrays(row_offsets, col_indices)
    gin = _graph_struct(nodes, ro, ci)
    gout = GunrockGraph()
    cfg = GunrockConfig()
    cfg.device = device
    dt = GunrockDataType(VTXID_INT, SIZET_INT, VALUE_INT)
    lib().gunrock_cc_func(C.byref(gout), C.byref(gin), cfg, dt)
    return _take_node_values(gout, nodes, np.int32)


class MstProblem(_Problem):
    """MSTProblem + MSTEnactor behind the handle C ABI: the minimum spanning forest of the CSR read as an undirected multigraph,
    unique under the order (weight as int32, then CSR index)."""

    _family, _problem, _enactor = "mst", "MSTProblem", "MSTEnactor"
    _stats = (("rounds", "edges_scanned", "kernel_launches"), ("kernel_ms",))

    def init(self, nodes, row_offsets, col_indices, edge_values):
        return self._init_host(nodes, row_offsets, col_indices, per_entry=(_i32(edge_values), "edge values", "edges"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_edge_values):
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_edge_values))

    def round_trace(self, max_rounds=1024):
        entries = (C.c_longlong * max_rounds)()
        ms = (C.c_double * max_rounds)()
        n = lib().grx_mst_round_trace(self._h, max_rounds, entries, ms)
        n = min(max(n, 0), max_rounds)
        return [{"entries": entries[i], "ms": ms[i]} for i in range(n)]

    def extract(self, selected=True):
        """(selected 0/1 per CSR entry as int32, or None; total_weight; forest_edges)"""
        sel = _out(self.edges, wanted=selected)
        tw, fe = C.c_longlong(), C.c_int()
        _check(lib().grx_mst_extract(self._h, _opt(sel), C.byref(tw), C.byref(fe)), "MSTProblem::Extract")
        return _cut(sel, self.edges), int(tw.value), int(fe.value)

    def device_results(self):
        """the device pointer of the selected flags"""
        return self._device_pointers(1)[0]


def gunrock_mst(nodes, row_offsets, col_indices, edge_values, device=0):
    """One-shot minimum spanning forest: returns (selected, total_weight, forest_edges); components = nodes - forest_edges."""
    return _one_shot(MstProblem(device=device).init(nodes, row_offsets, col_indices, edge_values),
                     MstProblem.reset, MstProblem.enact, MstProblem.extract)


MIS_SET, MIS_COLOR_ROUNDS, MIS_COLOR_FIRST_FIT = 0, 1, 2  # enum GRX_MIS_* (gunrock_mi355x.h)


def mis_priorities(nodes, seed=0):
    """The hashed priorities grx_mis_* uses when none are passed: fmix32((uint32)v + seed * 0x9E3779B9) as uint32 (host helper:
    the order is key(v) = (prio(v), v), prio compared as UNSIGNED here, as signed int32 for a caller's array)."""
    h = (np.arange(int(nodes), dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


class MisProblem(_Problem):
    """MISProblem + MISEnactor behind the handle C ABI: the lexicographically first maximal independent set and the two greedy
    colourings of the CSR read as an undirected simple graph, unique under the order key(v) = (prio(v), v)."""

    _family, _problem, _enactor = "mis", "MISProblem", "MISEnactor"
    _stats = (("rounds", "tail_sweeps", "entries_read", "polls", "kernel_launches"), ("kernel_ms",))

    def init(self, nodes, row_offsets, col_indices, priorities=None, seed=0):
        return self._init_host(nodes, row_offsets, col_indices, int(seed) & 0xFFFFFFFF, per_node=(priorities, "priorities", "nodes"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_priorities=None, seed=0):
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_priorities), int(seed) & 0xFFFFFFFF)

    def set_tail(self, enable=True):
        """False: one launch and one read-back per round to the end instead of the device-side tail loop (same result)"""
        _check(lib().grx_mis_set_tail(self._h, int(bool(enable))), "grx_mis_set_tail")
        return self

    def enact(self, mode=MIS_SET, max_grid_size=0):
        return self._timed(lib().grx_mis_enact, "MISEnactor::Enact", int(mode), int(max_grid_size))

    def round_trace(self, max_rounds=4096):
        vertices = (C.c_longlong * max_rounds)()
        ms = (C.c_double * max_rounds)()
        n = lib().grx_mis_round_trace(self._h, max_rounds, vertices, ms)
        n = min(max(n, 0), max_rounds)
        return [{"vertices": vertices[i], "ms": ms[i]} for i in range(n)]

    def extract(self, ids=True):
        """(ids as int32 per vertex, or None; summary = the size of the set or the number of colours)"""
        out, summary = _out(self.nodes, wanted=ids), C.c_longlong()
        _check(lib().grx_mis_extract(self._h, _opt(out), C.byref(summary)), "MISProblem::Extract")
        return _cut(out, self.nodes), int(summary.value)

    def device_results(self):
        """the device pointer of the ids"""
        return self._device_pointers(1)[0]


def _mis_one_shot(mode, nodes, row_offsets, col_indices, priorities, seed, device):
    return _one_shot(MisProblem(device=device).init(nodes, row_offsets, col_indices, priorities, seed),
                     MisProblem.reset, lambda p: p.enact(mode), MisProblem.extract)


def gunrock_mis(nodes, row_offsets, col_indices, priorities=None, seed=0, device=0):
    """One-shot maximal independent set: returns (ids 0/1 per vertex, size of the set)."""
    return _mis_one_shot(MIS_SET, nodes, row_offsets, col_indices, priorities, seed, device)


def gunrock_color(nodes, row_offsets, col_indices, priorities=None, seed=0, first_fit=True, device=0):
    """One-shot greedy colouring: returns (colour >= 1 per vertex, number of colours).  first_fit: Jones-Plassmann; else the
    reference's independent-set rounds run to the end (colour = 1 + the largest colour among the larger-keyed neighbours)."""
    return _mis_one_shot(MIS_COLOR_FIRST_FIT if first_fit else MIS_COLOR_ROUNDS, nodes, row_offsets, col_indices, priorities, seed,
                         device)


TC_AUTO, TC_LANE, TC_LDS, TC_GLOBAL = 0, 1, 2, 3  # enum GRX_TC_* (gunrock_mi355x.h)


class TcProblem(_TunedProblem):
    """TCProblem + TCEnactor behind the handle C ABI: per-vertex triangle counts (int64), their total, clustering coefficients and
    the transitivity of the CSR read as an undirected simple graph.

    Options: "strategy" (TC_AUTO / TC_LANE / TC_LDS / TC_GLOBAL), "lds_entries", "lane_max_row".
    device_results: (device pointer of the int64 counts, device pointer of the int32 degrees)."""

    _family, _problem, _enactor = "tc", "TCProblem", "TCEnactor"
    _stats = (("oriented_edges", "max_out_row", "entries_probed", "kernel_launches", ("lane_rows", "lds_rows", "global_rows")),
              ("kernel_ms", "build_ms"))
    _results = 2

    def extract(self, triangles=True):
        """(triangles as int64 per vertex, or None; the number of triangles of the graph)"""
        out, total = _out(self.nodes, np.int64, triangles), C.c_longlong()
        _check(lib().grx_tc_extract(self._h, _opt(out), C.byref(total)), "TCProblem::Extract")
        return _cut(out, self.nodes), int(total.value)

    def clustering(self, coefficients=True):
        """(clustering coefficient as float64 per vertex, or None; the transitivity of the graph)"""
        out, t = _out(self.nodes, np.float64, coefficients), C.c_double()
        _check(lib().grx_tc_clustering(self._h, _opt(out), C.byref(t)), "TCProblem::Clustering")
        return _cut(out, self.nodes), float(t.value)


def gunrock_tc(nodes, row_offsets, col_indices, device=0):
    """One-shot triangle counting: returns (triangles int64 per vertex, the number of triangles)."""
    return _one_shot(TcProblem(device=device).init(nodes, row_offsets, col_indices), TcProblem.reset, TcProblem.enact, TcProblem.extract)


def gunrock_clustering(nodes, row_offsets, col_indices, device=0):
    """One-shot clustering coefficients: returns (coefficient float64 per vertex, transitivity)."""
    return _one_shot(TcProblem(device=device).init(nodes, row_offsets, col_indices), TcProblem.reset, TcProblem.enact, TcProblem.clustering)


KCORE_AUTO, KCORE_ROUNDS, KCORE_DEVICE_LOOP = 0, 1, 2  # enum GRX_KCORE_* (gunrock_mi355x.h)


class KcoreProblem(_TunedProblem):
    """KcoreProblem + KcoreEnactor behind the handle C ABI: the core number of every vertex (int32), the degeneracy, the shell
    sizes and the k-cores of the CSR read as an undirected simple graph.

    Options: "schedule" (KCORE_AUTO / KCORE_ROUNDS / KCORE_DEVICE_LOOP), "compact_below", "wave_min_row", "loop_max_list",
    "loop_max_entries".
    device_results: (device pointer of the int32 core numbers, device pointer of the int32 degrees)."""

    _family, _problem, _enactor = "kcore", "KcoreProblem", "KcoreEnactor"
    _stats = (("simple_edges", "max_degree", "levels", "rounds", "vertices_peeled", "entries_read", "compactions", "kernel_launches"),
              ("kernel_ms", "build_ms"))
    _results = 2

    def enact(self, k_limit=-1, max_grid_size=0):
        return self._timed(lib().grx_kcore_enact, "KcoreEnactor::Enact", int(k_limit), int(max_grid_size))

    def level_trace(self):
        """the non-empty levels of the last enact: (k as int32, vertices peeled at it as int64, milliseconds as float64)"""
        return _count_then_fill(lib().grx_kcore_level_trace, self._h, "grx_kcore_level_trace", _TRACE)

    def extract(self, core=True):
        """(core numbers as int32 per vertex, or None; the degeneracy)"""
        out, d = _out(self.nodes, wanted=core), C.c_int()
        _check(lib().grx_kcore_extract(self._h, _opt(out), C.byref(d)), "KcoreProblem::Extract")
        return _cut(out, self.nodes), int(d.value)

    def shells(self):
        """shell sizes as int64: entry k is the number of vertices with core number k, k = 0 .. degeneracy"""
        return _count_then_fill(lib().grx_kcore_shells, self._h, "KcoreProblem::Shells", (np.int64,), negated=True)[0]

    def members(self, k, mask=True):
        """the k-core: (mask core >= k as uint8 per vertex, or None; its vertices; the edges of the graph inside it)"""
        out, v, e = _out(self.nodes, np.uint8, mask), C.c_longlong(), C.c_longlong()
        _check(lib().grx_kcore_members(self._h, int(k), _opt(out), C.byref(v), C.byref(e)), "KcoreProblem::Members")
        return _cut(out, self.nodes), int(v.value), int(e.value)


def gunrock_kcore(nodes, row_offsets, col_indices, device=0):
    """One-shot k-core decomposition: returns (core numbers int32 per vertex, the degeneracy)."""
    return _one_shot(KcoreProblem(device=device).init(nodes, row_offsets, col_indices),
                     KcoreProblem.reset, KcoreProblem.enact, KcoreProblem.extract)


def gunrock_kcore_members(nodes, row_offsets, col_indices, k, device=0):
    """One-shot k-core extraction (peels the levels below k only): returns (mask uint8 per vertex, vertices, edges inside)."""
    return _one_shot(KcoreProblem(device=device).init(nodes, row_offsets, col_indices),
                     KcoreProblem.reset, lambda p: p.enact(k_limit=k), lambda p: p.members(k))


TRUSS_AUTO, TRUSS_ROUNDS = 0, 1  # enum GRX_TRUSS_* (gunrock_mi355x.h)


class _EdgeListProblem(_TunedProblem):
    """A family over the canonical edges of the simple graph, (a, b) with a < b, sorted: their number, simple_edges, is read back
    behind Init and edges() returns them."""

    _count = "entries"

    def __init__(self, instrument=False, device=0):
        super().__init__(instrument, device)
        self.simple_edges = 0

    def _edge_list(self, src, dst):
        m = self._fn("edges")(self._h, _opt(src), _opt(dst))
        if m < 0:
            _check(-m, self._problem + "::Edges")
        return int(m)

    def _ready(self):
        self.simple_edges = self._edge_list(None, None)

    def edges(self):
        """the canonical edges (src, dst) as int32, src < dst, sorted by (src, dst)"""
        src, dst = _out(self.simple_edges), _out(self.simple_edges)
        m = self._edge_list(src, dst)
        return src[:m], dst[:m]


class TrussProblem(_EdgeListProblem):
    """TrussProblem + TrussEnactor behind the handle C ABI: the triangle support and the truss number of every edge (int32, in
    the canonical edge order: (a, b) with a < b, sorted), the truss classes, the k-trusses and the per-vertex maximum, of the CSR
    read as an undirected simple graph.

    Options: "schedule" (TRUSS_AUTO / TRUSS_ROUNDS), "wave_min_row", "loop_max_list", "loop_max_entries".
    device_results: device pointers of the int32 arrays (truss, support, src, dst), simple_edges entries each."""

    _family, _problem, _enactor = "truss", "TrussProblem", "TrussEnactor"
    _stats = (("simple_edges", "triangles", "max_support", "levels", "rounds", "edges_peeled", "support_entries", "peel_entries",
               "kernel_launches", "readbacks"), ("kernel_ms", "build_ms", "support_ms"))
    _results = 4

    def enact(self, k_limit=-1, max_grid_size=0):
        return self._timed(lib().grx_truss_enact, "TrussEnactor::Enact", int(k_limit), int(max_grid_size))

    def level_trace(self):
        """the non-empty levels of the last enact: (k as int32, edges peeled at it as int64, milliseconds as float64)"""
        return _count_then_fill(lib().grx_truss_level_trace, self._h, "grx_truss_level_trace", _TRACE)

    def support(self):
        """(triangles per edge as int32, the triangles of the graph); valid after init"""
        out, total = _out(self.simple_edges), C.c_longlong()
        _check(lib().grx_truss_support(self._h, _p(out), C.byref(total)), "TrussProblem::Support")
        return out[:self.simple_edges], int(total.value)

    def extract(self, truss=True):
        """(truss numbers as int32 per edge, or None; the largest)"""
        out, top = _out(self.simple_edges, wanted=truss), C.c_int()
        _check(lib().grx_truss_extract(self._h, _opt(out), C.byref(top)), "TrussProblem::Extract")
        return _cut(out, self.simple_edges), int(top.value)

    def classes(self):
        """class sizes as int64: entry k is the number of edges with truss number k, k = 0 .. max_truss"""
        return _count_then_fill(lib().grx_truss_classes, self._h, "TrussProblem::Classes", (np.int64,), negated=True)[0]

    def members(self, k, mask=True):
        """the k-truss: (mask truss >= k as uint8 per edge, or None; its edges; the vertices at one of them)"""
        out, e, v = _out(self.simple_edges, np.uint8, mask), C.c_longlong(), C.c_longlong()
        _check(lib().grx_truss_members(self._h, int(k), _opt(out), C.byref(e), C.byref(v)), "TrussProblem::Members")
        return _cut(out, self.simple_edges), int(e.value), int(v.value)

    def vertex_truss(self):
        """the largest truss number over the edges at every vertex, int32; 0 without a neighbour"""
        out = _out(self.nodes)
        _check(lib().grx_truss_vertex_truss(self._h, _p(out)), "TrussProblem::VertexTruss")
        return out[:self.nodes]


def gunrock_truss(nodes, row_offsets, col_indices, device=0):
    """One-shot k-truss decomposition: returns (src, dst, truss numbers, the largest), int32 per canonical edge."""
    return _one_shot(TrussProblem(device=device).init(nodes, row_offsets, col_indices),
                     TrussProblem.reset, TrussProblem.enact, lambda p: p.edges() + p.extract())


def gunrock_edge_support(nodes, row_offsets, col_indices, device=0):
    """One-shot per-edge triangle support: returns (src, dst, support as int32 per canonical edge, the triangles of the graph)."""
    return _one_shot(TrussProblem(device=device).init(nodes, row_offsets, col_indices), lambda p: p.edges() + p.support())


def gunrock_ktruss(nodes, row_offsets, col_indices, k, device=0):
    """One-shot k-truss extraction (peels the levels below k only): returns (src, dst, mask uint8 per edge, edges, vertices)."""
    return _one_shot(TrussProblem(device=device).init(nodes, row_offsets, col_indices),
                     TrussProblem.reset, lambda p: p.enact(k_limit=k), lambda p: p.edges() + p.members(k))


SCC_AUTO, SCC_ROUNDS, SCC_DEVICE_LOOP = 0, 1, 2  # enum GRX_SCC_* (gunrock_mi355x.h)
SCC_TRIM, SCC_PIVOT, SCC_COLOUR = 0, 1, 2  # enum GRX_SCC_PHASE_* (gunrock_mi355x.h): the kinds of phase_trace()


class SccProblem(_TunedProblem):
    """SccProblem + SccEnactor behind the handle C ABI: the strongly connected components of the CSR read as a directed
    multigraph: comp[v] = the smallest vertex id of v's component (int32), the component sizes and the condensation.

    Options: "schedule" (SCC_AUTO / SCC_ROUNDS / SCC_DEVICE_LOOP), "pivot_phase", "trim", "pair_trim", "wave_min_row",
    "loop_max_list", "loop_max_entries".
    device_results: (device pointers of comp (int32 per vertex), of the transpose's row offsets and of its column indices)."""

    _family, _problem, _enactor = "scc", "SccProblem", "SccEnactor"
    _stats = (("trimmed", "trim_rounds", "pivot_component", "colour_rounds", "sweeps", "bfs_levels", "entries_read", "kernel_launches"),
              ("kernel_ms", "build_ms"))
    _results = 3

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_inv_row_offsets=None, d_inv_col_indices=None):
        """a CSR in HBM (borrowed); the transpose too when both inverse pointers are given, else it is built"""
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_inv_row_offsets), C.c_void_p(d_inv_col_indices))

    def phase_trace(self):
        """the phases of the last enact in order: (kind as int32: SCC_TRIM / SCC_PIVOT / SCC_COLOUR, vertices finished in it as
        int64, milliseconds as float64)"""
        return _count_then_fill(lib().grx_scc_phase_trace, self._h, "grx_scc_phase_trace", _TRACE)

    def extract(self, comp=True):
        """(comp as int32 per vertex, or None; the number of components)"""
        out, n = _out(self.nodes, wanted=comp), C.c_longlong()
        _check(lib().grx_scc_extract(self._h, _opt(out), C.byref(n)), "SccProblem::Extract")
        return _cut(out, self.nodes), int(n.value)

    def summary(self):
        """{"components", "trivial", "largest", "largest_root"}"""
        c, t, l, r = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_int()
        _check(lib().grx_scc_summary(self._h, C.byref(c), C.byref(t), C.byref(l), C.byref(r)), "SccProblem::Summary")
        return {"components": int(c.value), "trivial": int(t.value), "largest": int(l.value), "largest_root": int(r.value)}

    def sizes(self):
        """size[v] as int32: the vertex count of v's component"""
        out = _out(self.nodes)
        _check(lib().grx_scc_sizes(self._h, _p(out)), "SccProblem::Sizes")
        return out[:self.nodes]

    def condensation(self, max_edges=None):
        """the condensation sorted by (from, to): (from as int32, to as int32, the number of pairs); max_edges caps what is
        copied (0: the count only)"""
        return _pair_list(lib().grx_scc_condensation, self._h, "SccProblem::Condensation", max_edges)


def gunrock_scc(nodes, row_offsets, col_indices, device=0):
    """One-shot strongly connected components: returns (comp int32 per vertex: the smallest id of its component, components)."""
    return _one_shot(SccProblem(device=device).init(nodes, row_offsets, col_indices), SccProblem.reset, SccProblem.enact, SccProblem.extract)


def gunrock_condensation(nodes, row_offsets, col_indices, device=0):
    """One-shot condensation: returns (comp, from, to), the pairs sorted by (from, to)."""
    return _one_shot(SccProblem(device=device).init(nodes, row_offsets, col_indices), SccProblem.reset, SccProblem.enact,
                     lambda p: (p.extract()[0],) + p.condensation()[:2])


BCC_AUTO, BCC_ROUNDS, BCC_DEVICE_LOOP = 0, 1, 2  # enum GRX_BCC_* (gunrock_mi355x.h)
BCC_FOREST, BCC_SIZES, BCC_NUMBER, BCC_LOWHIGH, BCC_LINK, BCC_LABEL = range(6)  # enum GRX_BCC_PHASE_*: the kinds of phase_trace()


class BccProblem(_EdgeListProblem):
    """BccProblem + BccEnactor behind the handle C ABI: the biconnected components (bcc[e] = the smallest canonical edge index of
    e's block, int32), the bridges and the articulation points (uint8 masks), the 2-edge-connected components (tecc[v] = the
    smallest id, int32) and the block-cut tree, of the CSR read as an undirected simple graph; per-edge arrays in the canonical
    edge order ((a, b) with a < b, sorted).

    Options: "schedule" (BCC_AUTO / BCC_ROUNDS / BCC_DEVICE_LOOP), "wave_min_row", "loop_max_list", "loop_max_entries".
    device_results: int32 arrays but for the two uint8 masks; per edge: bcc, bridge, src, dst; per vertex: the rest.  parent /
    level are the spanning forest (not unique)."""

    _family, _problem, _enactor = "bcc", "BccProblem", "BccEnactor"
    _stats = (("simple_edges", "trees", "levels", "entries_read", "kernel_launches", "readbacks"), ("kernel_ms", "build_ms"))
    _results = ("bcc", "tecc", "bridge", "articulation", "src", "dst", "parent", "level")
    _SUMMARY = ("blocks", "bridges", "articulation_points", "largest_block", "largest_block_id", "tecc_components", "largest_tecc",
                "largest_tecc_root")

    def phase_trace(self):
        """the six phases of the last enact: (kind as int32: BCC_FOREST .. BCC_LABEL, vertices or edges touched as int64,
        milliseconds as float64)"""
        return _count_then_fill(lib().grx_bcc_phase_trace, self._h, "grx_bcc_phase_trace", _TRACE)

    def extract(self):
        """{"bcc": int32 per edge, "bridge": uint8 per edge, "articulation": uint8 per vertex, "tecc": int32 per vertex,
        "block_size": int32 per edge}"""
        M, N = self.simple_edges, self.nodes
        bcc, size, tecc, bridge, art = _out(M), _out(M), _out(N), _out(M, np.uint8), _out(N, np.uint8)
        _check(lib().grx_bcc_extract(self._h, _p(bcc), _u8p(bridge), _u8p(art), _p(tecc), _p(size)), "BccProblem::Extract")
        return {"bcc": bcc[:M], "bridge": bridge[:M], "articulation": art[:N], "tecc": tecc[:N], "block_size": size[:M]}

    def summary(self):
        """{"blocks", "bridges", "articulation_points", "largest_block", "largest_block_id", "tecc_components", "largest_tecc",
        "largest_tecc_root"}"""
        v = [C.c_int() if name in ("largest_block_id", "largest_tecc_root") else C.c_longlong() for name in self._SUMMARY]
        _check(lib().grx_bcc_summary(self._h, *[C.byref(x) for x in v]), "BccProblem::Summary")
        return {name: int(x.value) for name, x in zip(self._SUMMARY, v)}

    def block_cut(self, max_edges=None):
        """the block-cut tree sorted by (vertex, block): (articulation point as int32, bcc id as int32, the number of pairs);
        max_edges caps what is copied (0: the count only).  The library builds the pairs once per enact: the second call copies"""
        return _pair_list(lib().grx_bcc_block_cut, self._h, "BccProblem::BlockCut", max_edges)


def gunrock_bcc(nodes, row_offsets, col_indices, device=0):
    """One-shot biconnected components: returns (src, dst, bcc int32 per canonical edge: the smallest edge index of its block,
    blocks)."""
    return _one_shot(BccProblem(device=device).init(nodes, row_offsets, col_indices), BccProblem.reset, BccProblem.enact,
                     lambda p: p.edges() + (p.extract()["bcc"], p.summary()["blocks"]))


def gunrock_bridges(nodes, row_offsets, col_indices, device=0):
    """One-shot bridges: returns (src, dst, mask uint8 per canonical edge, bridges)."""
    return _one_shot(BccProblem(device=device).init(nodes, row_offsets, col_indices), BccProblem.reset, BccProblem.enact,
                     lambda p: p.edges() + (p.extract()["bridge"], p.summary()["bridges"]))


def gunrock_articulation_points(nodes, row_offsets, col_indices, device=0):
    """One-shot articulation points: returns (mask uint8 per vertex, articulation points)."""
    return _one_shot(BccProblem(device=device).init(nodes, row_offsets, col_indices), BccProblem.reset, BccProblem.enact,
                     lambda p: (p.extract()["articulation"], p.summary()["articulation_points"]))


MAXFLOW_AUTO, MAXFLOW_ROUNDS, MAXFLOW_DEVICE_LOOP = 0, 1, 2  # enum GRX_MAXFLOW_* (gunrock_mi355x.h)
MAXFLOW_PREFLOW, MAXFLOW_RETURN, MAXFLOW_CUT = range(3)  # enum GRX_MAXFLOW_PHASE_*: the kinds of phase_trace()
MAXFLOW_GAVE_UP = -4  # grx_maxflow_enact: more than "max_rounds" rounds


class MaxflowGaveUp(RuntimeError):
    """MaxflowProblem.enact passed "max_rounds" (GRX_MAXFLOW_GAVE_UP): the handle holds no result and takes the next reset"""


class _PairListProblem(_TunedProblem):
    """A family over the canonical pairs of the graph, (a, b) with a < b, sorted: their number, num_pairs, is read back behind
    Init and pairs() returns them with the family's values, _pair_columns int32 columns in all."""

    _count = "entries"
    _pair_columns = 0

    def __init__(self, instrument=False, device=0):
        super().__init__(instrument, device)
        self.num_pairs = 0

    def _pair_list(self, columns):
        m = self._fn("pairs")(self._h, *map(_opt, columns))
        if m < 0:
            _check(-m, self._problem + "::Pairs")
        return int(m)

    def _ready(self):
        self.num_pairs = self._pair_list([None] * self._pair_columns)

    def pairs(self):
        """the canonical pairs and their values as int32 columns, sorted by (a, b): see the class"""
        columns = [_out(self.num_pairs) for _ in range(self._pair_columns)]
        m = self._pair_list(columns)
        return tuple(c[:m] for c in columns)


class MaxflowProblem(_PairListProblem):
    """MaxflowProblem + MaxflowEnactor behind the handle C ABI: the maximum flow from src to sink and the minimum cuts of the CSR read
    as a directed multigraph with int32 capacities (None: 1 each; parallel arcs add up, self-loops are ignored).  Per-pair arrays in
    the canonical pair order ((a, b) with a < b and an arc either way, sorted).  value, side and cut have one value each; flow and
    arc_flow are a valid maximum flow that depends on the run.  pairs(): (a, b, cap_ab, cap_ba).

    Options: "schedule" (MAXFLOW_AUTO / MAXFLOW_ROUNDS / MAXFLOW_DEVICE_LOOP), "wave_min_row", "discharge_steps",
    "relabel_interval", "max_rounds", "loop_max_list", "loop_max_entries".
    device_results: per pair flow (int32), cut (uint8), a, b (int32); per vertex side (uint8), excess (int64) and height (int32,
    not unique)."""

    _family, _problem, _enactor = "maxflow", "MaxflowProblem", "MaxflowEnactor"
    _pair_columns = 4  # (a, b, cap_ab, cap_ba)
    _stats = (("pairs", "rounds", "global_relabels", "pushes", "relabels", "entries_read", "kernel_launches", "readbacks"),
              ("kernel_ms", "build_ms"))
    _results = ("flow", "side", "cut", "a", "b", "excess", "height")
    _SUMMARY = ("value", "side0", "side1", "side2", "cut0", "cut1")

    def init(self, nodes, row_offsets, col_indices, capacities=None):
        return self._init_host(nodes, row_offsets, col_indices, per_entry=(capacities, "capacities", "arcs"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_capacities=None):
        """the CSR (and the capacities) stay the caller's and must outlive the handle"""
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_capacities))

    def reset(self, src, sink):
        _check(lib().grx_maxflow_reset(self._h, int(src), int(sink)), "MaxflowProblem::Reset")

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds; MaxflowGaveUp when the rounds passed the option max_rounds"""
        ms = C.c_float()
        rc = lib().grx_maxflow_enact(self._h, int(max_grid_size), C.byref(ms))
        if rc == MAXFLOW_GAVE_UP:
            raise MaxflowGaveUp("gunrockinst_amd: MaxflowEnactor::Enact gave up (code %d)" % rc)
        _check(rc, "MaxflowEnactor::Enact")
        return ms.value

    def phase_trace(self):
        """the three phases of the last enact: (kind as int32: MAXFLOW_PREFLOW / MAXFLOW_RETURN / MAXFLOW_CUT, rounds as int64,
        milliseconds as float64)"""
        return _count_then_fill(lib().grx_maxflow_phase_trace, self._h, "grx_maxflow_phase_trace", _TRACE)

    def extract(self):
        """{"value": int, "flow": int32 per pair, "side": uint8 per vertex, "cut": uint8 per pair}"""
        M, N, value = self.num_pairs, self.nodes, C.c_longlong()
        flow, side, cut = _out(M), _out(N, np.uint8), _out(M, np.uint8)
        _check(lib().grx_maxflow_extract(self._h, C.byref(value), _p(flow), _u8p(side), _u8p(cut)), "MaxflowProblem::Extract")
        return {"value": int(value.value), "flow": flow[:M], "side": side[:N], "cut": cut[:M]}

    def arc_flow(self):
        """int32 per CSR entry of the input"""
        out = _out(self.entries)
        _check(lib().grx_maxflow_arc_flow(self._h, _p(out)), "MaxflowProblem::ArcFlow")
        return out[:self.entries]

    def summary(self):
        """{"value", "side0", "side1", "side2", "cut0", "cut1"}"""
        v = (C.c_longlong * 6)()
        _check(lib().grx_maxflow_summary(self._h, v), "MaxflowProblem::Summary")
        return {name: int(x) for name, x in zip(self._SUMMARY, v)}


def gunrock_maxflow(nodes, row_offsets, col_indices, capacities, src, sink, device=0):
    """One-shot maximum flow: returns (value, arc_flow int32 per CSR entry)."""
    return _one_shot(MaxflowProblem(device=device).init(nodes, row_offsets, col_indices, capacities), lambda p: p.reset(src, sink),
                     MaxflowProblem.enact, lambda p: (p.extract()["value"], p.arc_flow()))


def gunrock_mincut(nodes, row_offsets, col_indices, capacities, src, sink, device=0):
    """One-shot minimum cut: returns (value, side uint8 per vertex, a, b, cut uint8 per canonical pair)."""
    def result(p):
        r = p.extract()
        a, b = p.pairs()[:2]
        return r["value"], r["side"], a, b, r["cut"]
    return _one_shot(MaxflowProblem(device=device).init(nodes, row_offsets, col_indices, capacities), lambda p: p.reset(src, sink),
                     MaxflowProblem.enact, result)


MATCHING_AUTO, MATCHING_ROUNDS, MATCHING_DEVICE_LOOP = 0, 1, 2  # enum GRX_MATCHING_* (gunrock_mi355x.h)
MATCHING_STEP_WIDE, MATCHING_STEP_LOOP = 0, 1  # enum GRX_MATCHING_STEP_*: the kinds of round_trace()
MATCHING_GAVE_UP, MATCHING_OVERFLOW = -4, -5  # grx_matching_enact: more than "max_rounds" rounds; grx_matching_contract: a sum outside int32


class MatchingGaveUp(RuntimeError):
    """MatchingProblem.enact passed "max_rounds" (GRX_MATCHING_GAVE_UP): the handle holds no result and takes the next reset"""


class MatchingOverflow(ArithmeticError):
    """MatchingProblem.contract: a coarse pair weight or vertex weight is outside int32 (GRX_MATCHING_OVERFLOW); nothing is kept"""


def matching_keys(pair_weights, seed=0):
    """The keys grx_matching_* orders the pairs by, as uint64 (host helper): ((uint32)w(i) ^ 0x80000000) << 32 | fmix32((uint32)i +
    seed * 0x9E3779B9) for the pair weights in canonical pair order; heavier is larger, ties go by mis_priorities' hash."""
    w = np.asarray(pair_weights, dtype=np.int64)
    high = ((w & 0xFFFFFFFF) ^ 0x80000000).astype(np.uint64)
    return (high << np.uint64(32)) | mis_priorities(w.shape[0], seed).astype(np.uint64)


class MatchingProblem(_PairListProblem):
    """MatchingProblem + MatchingEnactor behind the handle C ABI: the locally dominant (heavy-edge) matching of the CSR read as an
    undirected simple graph with int32 weights (None: 1 each; a pair's weight is the largest of its entries), unique under the order
    matching_keys(); and its contraction into the coarse graph.  Per-pair arrays in the canonical pair order ((a, b) with a < b,
    sorted); pairs(): (src, dst, weight).

    Options: "schedule" (MATCHING_AUTO / MATCHING_ROUNDS / MATCHING_DEVICE_LOOP), "wave_min_row", "max_rounds", "loop_max_list",
    "loop_max_entries".
    device_results: per pair in_matching (uint8), src, dst, weight (int32); per vertex mate and medge (int32)."""

    _family, _problem, _enactor = "matching", "MatchingProblem", "MatchingEnactor"
    _pair_columns = 3
    _stats = (("pairs", "rounds", "loop_rounds", "entries_read", "polls", "kernel_launches"), ("kernel_ms", "build_ms"))
    _results = ("in_matching", "mate", "medge", "src", "dst", "weight")
    _SUMMARY = ("pairs", "matched", "weight", "unmatched", "unmatched_with_neighbours")

    def __init__(self, instrument=False, device=0):
        super().__init__(instrument, device)
        self.coarse_nodes = self.coarse_entries = 0

    def init(self, nodes, row_offsets, col_indices, weights=None, seed=0):
        return self._init_host(nodes, row_offsets, col_indices, int(seed) & 0xFFFFFFFF, per_entry=(weights, "weights", "entries"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_weights=None, seed=0):
        """the CSR (and the weights) stay the caller's; the build reads them, nothing later does"""
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_weights), int(seed) & 0xFFFFFFFF)

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds; MatchingGaveUp when the rounds passed the option max_rounds"""
        ms = C.c_float()
        rc = lib().grx_matching_enact(self._h, int(max_grid_size), C.byref(ms))
        if rc == MATCHING_GAVE_UP:
            raise MatchingGaveUp("gunrockinst_amd: MatchingEnactor::Enact gave up (code %d)" % rc)
        _check(rc, "MatchingEnactor::Enact")
        return ms.value

    def round_trace(self):
        """the host's steps of the last enact: (kind as int32: MATCHING_STEP_WIDE / MATCHING_STEP_LOOP, rounds, live list, matched
        pairs as int64)"""
        return _count_then_fill(lib().grx_matching_round_trace, self._h, "grx_matching_round_trace", (np.int32,) + (np.int64,) * 3)

    def extract(self):
        """{"in_matching": uint8 per pair, "mate": int32 per vertex (-1: unmatched), "medge": int32 per vertex (-1: unmatched)}"""
        M, N = self.num_pairs, self.nodes
        in_matching, mate, medge = _out(M, np.uint8), _out(N), _out(N)
        _check(lib().grx_matching_extract(self._h, _u8p(in_matching), _p(mate), _p(medge)), "MatchingProblem::Extract")
        return {"in_matching": in_matching[:M], "mate": mate[:N], "medge": medge[:N]}

    def summary(self):
        """{"pairs", "matched", "weight", "unmatched", "unmatched_with_neighbours"}"""
        v = (C.c_longlong * 5)()
        _check(lib().grx_matching_summary(self._h, v), "MatchingProblem::Summary")
        return {name: int(x) for name, x in zip(self._SUMMARY, v)}

    def contract(self, vertex_weights=None):
        """builds the coarse graph of the last enact on the device; returns (coarse_nodes, coarse_entries).  vertex_weights: None (1
        each), an int32 array, or a device pointer as int (the "vweight" of a level before).  MatchingOverflow when a sum leaves
        int32."""
        nc, ne = C.c_longlong(), C.c_longlong()
        if vertex_weights is None or isinstance(vertex_weights, int):
            vw, ptr = None, C.c_void_p(vertex_weights) if vertex_weights else None
        else:
            vw = _i32_of(vertex_weights, self.nodes, "vertex weights", "nodes")
            ptr = C.c_void_p(vw.ctypes.data)
        rc = lib().grx_matching_contract(self._h, ptr, C.byref(nc), C.byref(ne))
        if rc == MATCHING_OVERFLOW:
            raise MatchingOverflow("gunrockinst_amd: MatchingProblem::Contract: a sum outside int32 (code %d)" % rc)
        _check(rc, "MatchingProblem::Contract")
        self.coarse_nodes, self.coarse_entries = int(nc.value), int(ne.value)
        return self.coarse_nodes, self.coarse_entries

    def coarse_extract(self):
        """(map, coarse_nodes, row_offsets, col_indices, weights, vweight) of the last contract, int32 arrays"""
        nc, ne = self.coarse_nodes, self.coarse_entries
        cmap, ro, ci, w, vw = _out(self.nodes), _out(nc + 1), _out(ne), _out(ne), _out(nc)
        _check(lib().grx_matching_coarse_extract(self._h, _p(cmap), _p(ro), _p(ci), _p(w), _p(vw)), "MatchingProblem::CoarseExtract")
        return cmap[:self.nodes], nc, ro, ci[:ne], w[:ne], vw[:nc]

    def coarse_device(self):
        """device pointers {"map", "row_offsets", "col_indices", "weights", "vweight"} of the last contract: they live until this
        handle's next reset, contract or close"""
        names = ("map", "row_offsets", "col_indices", "weights", "vweight")
        return dict(zip(names, self._device_pointers(len(names), "coarse_device")))


def gunrock_matching(nodes, row_offsets, col_indices, weights=None, seed=0, device=0):
    """One-shot heavy-edge matching: returns (src, dst, in_matching uint8 per canonical pair, mate int32 per vertex, matched pairs,
    total matched weight)."""
    def result(p):
        r, s = p.extract(), p.summary()
        return p.pairs()[:2] + (r["in_matching"], r["mate"], s["matched"], s["weight"])
    return _one_shot(MatchingProblem(device=device).init(nodes, row_offsets, col_indices, weights, seed), MatchingProblem.reset,
                     MatchingProblem.enact, result)


def gunrock_coarsen(nodes, row_offsets, col_indices, weights=None, vertex_weights=None, seed=0, levels=1, device=0):
    """One-shot multilevel coarsening: a list with (map, coarse_nodes, row_offsets, col_indices, weights, vweight) per level, each
    level matched and contracted on the device from the level before's device arrays; stops early behind a level that matched
    nothing."""
    out, handles, p = [], [], None
    try:
        p = MatchingProblem(device=device).init(nodes, row_offsets, col_indices, weights, seed)
        vw = vertex_weights
        for _ in range(int(levels)):
            handles.append(p)
            p.reset()
            p.enact()
            matched = p.summary()["matched"]
            nc, ne = p.contract(vw)
            out.append(p.coarse_extract())
            if matched == 0:
                break
            d = p.coarse_device()
            vw = d["vweight"]
            if len(out) < int(levels):
                p = MatchingProblem(device=device).init_device(nc, ne, d["row_offsets"], d["col_indices"], d["weights"] if ne else None, seed)
    finally:
        for h in reversed(handles):
            h.close()
        if p is not None and p not in handles:
            p.close()
    return out


CLIQUE_AUTO, CLIQUE_BITMAP, CLIQUE_LIST = 0, 1, 2  # enum GRX_CLIQUE_* (gunrock_mi355x.h)
CLIQUE_OVERFLOW = -7  # grx_clique_enact: the bound on the counts reached "count_limit"


class CliqueOverflow(ArithmeticError):
    """CliqueProblem.enact: sum over u of C(d+(u), k - 1) reached "count_limit" (GRX_CLIQUE_OVERFLOW): nothing ran, the handle holds
    no result and takes the next enact"""


class CliqueProblem(_TunedProblem):
    """CliqueProblem + CliqueEnactor behind the handle C ABI: for k = 3 .. 6 the number of k-cliques through every vertex (int64)
    and their total, of the CSR read as an undirected simple graph.  `rank` (int32 per vertex, or None) orients the build; no rank
    changes a result.

    Options: "strategy" (CLIQUE_AUTO / CLIQUE_BITMAP / CLIQUE_LIST), "bitmap_rows", "count_limit".
    device_results: (device pointer of the int64 counts, device pointer of the int32 degrees)."""

    _family, _problem, _enactor = "clique", "CliqueProblem", "CliqueEnactor"
    _results = 2

    def init(self, nodes, row_offsets, col_indices, rank=None):
        return self._init_host(nodes, row_offsets, col_indices, per_node=(rank, "ranks", "nodes"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_rank=None):
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_rank))

    def enact(self, k, max_grid_size=0):
        """the elapsed milliseconds; CliqueOverflow when the bound on the counts reached the option count_limit"""
        ms = C.c_float()
        rc = lib().grx_clique_enact(self._h, int(k), int(max_grid_size), C.byref(ms))
        if rc == CLIQUE_OVERFLOW:
            raise CliqueOverflow("gunrockinst_amd: CliqueEnactor::Enact refused: the bound %.17g reached count_limit (code %d)"
                                 % (self.stats()["bound"], rc))
        _check(rc, "CliqueEnactor::Enact")
        return float(ms.value)

    def stats(self):
        o, r, a, l, n = (C.c_longlong() for _ in range(5))
        rows, edges = (C.c_longlong * 2)(), (C.c_longlong * 2)()
        bound, k, b = C.c_double(), C.c_double(), C.c_double()
        _check(lib().grx_clique_stats(self._h, C.byref(o), C.byref(r), rows, edges, C.byref(a), C.byref(l), C.byref(bound), C.byref(n),
                                      C.byref(k), C.byref(b)), "grx_clique_stats")
        return {"oriented_edges": o.value, "max_out_row": r.value, "bitmap_rows": rows[0], "list_rows": rows[1],
                "bitmap_edges": edges[0], "list_edges": edges[1], "bit_ands": a.value, "list_lookups": l.value, "bound": bound.value,
                "kernel_launches": n.value, "kernel_ms": k.value, "build_ms": b.value}

    def extract(self, cliques=True):
        """(cliques as int64 per vertex, or None; the number of k-cliques of the graph)"""
        out, total = _out(self.nodes, np.int64, cliques), C.c_longlong()
        _check(lib().grx_clique_extract(self._h, _opt(out), C.byref(total)), "CliqueProblem::Extract")
        return _cut(out, self.nodes), int(total.value)


def gunrock_cliques(nodes, row_offsets, col_indices, k, rank=None, device=0):
    """One-shot k-clique counting, k = 3 .. 6: returns (cliques int64 per vertex, the number of k-cliques)."""
    return _one_shot(CliqueProblem(device=device).init(nodes, row_offsets, col_indices, rank), CliqueProblem.reset,
                     lambda p: p.enact(k), CliqueProblem.extract)


C4_AUTO, C4_LANE, C4_WAVE, C4_BLOCK, C4_GLOBAL = 0, 1, 2, 3, 4  # enum GRX_C4_* (gunrock_mi355x.h): option "strategy"
C4_OVERFLOW = -7  # grx_c4_enact: the bound on the counts reached "count_limit"


class C4Overflow(ArithmeticError):
    """C4Problem.enact: sum over u of W(u) (dlow(u) - 1) / 2 reached "count_limit" (GRX_C4_OVERFLOW): nothing ran, the handle holds no
    result and takes the next enact"""


class C4Problem(_EdgeListProblem):
    """C4Problem + C4Enactor behind the handle C ABI: the 4-cycles (butterflies) through every vertex and every edge (int64, the edges
    in the canonical order: (a, b) with a < b, sorted) and their total, of the CSR read as an undirected simple graph.  The build
    reads a device CSR and nothing later does.

    Options: "strategy" (C4_AUTO / C4_LANE / C4_WAVE / C4_BLOCK / C4_GLOBAL), "lane_max_wedges", "table_slots", "block_slots",
    "scratch_mib", "edges", "count_limit".
    device_results: "cycles", "edge_cycles": int64 per vertex and per canonical edge; "src", "dst": int32 per edge."""

    _family, _problem, _enactor = "c4", "C4Problem", "C4Enactor"
    _results = ("cycles", "edge_cycles", "src", "dst")
    _REGIMES = ("lane", "wave", "block", "global")

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds; C4Overflow when the bound on the counts reached the option count_limit"""
        ms = C.c_float()
        rc = lib().grx_c4_enact(self._h, int(max_grid_size), C.byref(ms))
        if rc == C4_OVERFLOW:
            raise C4Overflow("gunrockinst_amd: C4Enactor::Enact refused: the bound %.17g reached count_limit (code %d)"
                             % (self.stats()["bound"], rc))
        _check(rc, "C4Enactor::Enact")
        return float(ms.value)

    def stats(self):
        m, w, probes, n = (C.c_longlong() for _ in range(4))
        vertices, wedges = (C.c_longlong * 4)(), (C.c_longlong * 4)()
        bound, k, b = C.c_double(), C.c_double(), C.c_double()
        _check(lib().grx_c4_stats(self._h, C.byref(m), C.byref(w), vertices, wedges, C.byref(probes), C.byref(bound), C.byref(n), C.byref(k),
                                  C.byref(b)), "grx_c4_stats")
        out = {"simple_edges": m.value, "wedges": w.value, "table_probes": probes.value, "bound": bound.value, "kernel_launches": n.value,
               "kernel_ms": k.value, "build_ms": b.value}
        for i, name in enumerate(self._REGIMES):
            out[name + "_vertices"], out[name + "_wedges"] = int(vertices[i]), int(wedges[i])
        return out

    def extract(self, cycles=True):
        """(4-cycles as int64 per vertex, or None; the 4-cycles of the graph)"""
        out, total = _out(self.nodes, np.int64, cycles), C.c_longlong()
        _check(lib().grx_c4_extract(self._h, _opt(out), C.byref(total)), "C4Problem::Extract")
        return _cut(out, self.nodes), int(total.value)

    def extract_edges(self):
        """4-cycles as int64 per canonical edge; refused (code -1) when the last enact ran with the option edges = 0"""
        out = _out(self.simple_edges, np.int64)
        _check(lib().grx_c4_extract_edges(self._h, _i64p(out)), "C4Problem::ExtractEdges")
        return out[:self.simple_edges]


def gunrock_four_cycles(nodes, row_offsets, col_indices, device=0):
    """One-shot 4-cycle (butterfly) counting per vertex: returns (cycles int64 per vertex, the 4-cycles of the graph)."""
    def prepare(p):
        p.set_option("edges", 0)
        p.reset()
    return _one_shot(C4Problem(device=device).init(nodes, row_offsets, col_indices), prepare, C4Problem.enact, C4Problem.extract)


def gunrock_edge_four_cycles(nodes, row_offsets, col_indices, device=0):
    """One-shot 4-cycle (butterfly) counting per edge: returns (src, dst, edge_cycles int64 per canonical edge, the 4-cycles of the
    graph)."""
    return _one_shot(C4Problem(device=device).init(nodes, row_offsets, col_indices), C4Problem.reset, C4Problem.enact,
                     lambda p: p.edges() + (p.extract_edges(), p.extract(cycles=False)[1]))


RW_AUTO, RW_LANE, RW_TILE = 0, 1, 2  # enum GRX_RW_* (gunrock_mi355x.h): option "strategy"


def rw_draw(seed, walk, step, t):
    """The draws of grx_rw_*: Mix(seed ^ Mix((walk << 32) | (step << 8) | t)) as uint64, Mix the splitmix64 finaliser
    (devgraph._splitmix64).  Host helper; the arguments may be arrays (walk < 2^31, step < 2^24, t < 2^8)."""
    def mix(x):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))
    seed, walk, step, t = (np.asarray(a).astype(np.uint64) for a in (seed, walk, step, t))
    with np.errstate(over="ignore"):
        out = mix(seed ^ mix((walk << np.uint64(32)) | (step << np.uint64(8)) | t))
    return out if out.ndim else np.uint64(out)


class RwProblem(_TunedProblem):
    """RwProblem + RwEnactor behind the handle C ABI: uniform, weighted and node2vec-biased random walks on the CSR as given (directed,
    self-loops and duplicates kept).  Every draw is rw_draw(seed, walk, step, try) and every choice exact integer arithmetic on it
    (gunrock_mi355x.h has the definition), so the walks are integers with one value: no option but "length", "seed", "weighted",
    the biases and "tries" changes them.  The build reads a device CSR (and the weights) and nothing later does.

    Options: "strategy" (RW_AUTO / RW_LANE / RW_TILE), "length", "seed", "weighted", "bias_return", "bias_in", "bias_out", "tries",
    "visits"."""

    _family, _problem, _enactor = "rw", "RwProblem", "RwEnactor"
    _count = "entries"
    _stats = (("walks", "steps", "ended_early", "biased_tries", "forced_fallbacks", "kernel_launches"), ("kernel_ms", "build_ms"))
    _results = ("walks", "lengths", "visits")

    def __init__(self, instrument=False, device=0):
        super().__init__(instrument, device)
        self.num_walks = 0
        self.length = 0  # of the last enact
        self._length = 0  # the option

    def init(self, nodes, row_offsets, col_indices, weights=None):
        return self._init_host(nodes, row_offsets, col_indices, per_entry=(weights, "weights", "entries"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_weights=None):
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_weights))

    def set_option(self, name, value):
        rc = super().set_option(name, value)
        if rc == 0 and name == "length":
            self._length = int(value)
        return rc

    def reset(self, starts):
        """the start vertices, one walk each"""
        s = _i32(starts).reshape(-1)
        _check(lib().grx_rw_reset(self._h, int(s.shape[0]), _p(s)), "RwProblem::Reset")
        self.num_walks = int(s.shape[0])

    def enact(self, max_grid_size=0):
        ms = super().enact(max_grid_size)
        self.length = self._length
        return ms

    def extract(self, walks=True, lengths=True, visits=False):
        """(walks int32 num_walks x (length + 1), lengths int32, visits int64 per vertex, steps); None for what was not asked for"""
        out_w = np.empty((max(self.num_walks, 1), self.length + 1), dtype=np.int32) if walks else None
        out_l, out_v, steps = _out(self.num_walks, wanted=lengths), _out(self.nodes, np.int64, visits), C.c_longlong()
        _check(lib().grx_rw_extract(self._h, _opt(out_w), _opt(out_l), _opt(out_v), C.byref(steps)), "RwProblem::Extract")
        return _cut(out_w, self.num_walks), _cut(out_l, self.num_walks), _cut(out_v, self.nodes), int(steps.value)

    def device_results(self):
        """device pointers {"walks": int32, rows "pitch" entries apart; "lengths": int32 per walk; "visits": int64 per vertex or None}
        and "pitch" """
        p, pitch = [C.c_void_p() for _ in self._results], C.c_longlong()
        _check(lib().grx_rw_device_results(self._h, *map(C.byref, p), C.byref(pitch)), "grx_rw_device_results")
        return dict(zip(self._results, (x.value for x in p)), pitch=int(pitch.value))


def gunrock_random_walks(nodes, row_offsets, col_indices, starts, length, weights=None, seed=0, bias=None, tries=32, visits=False, device=0):
    """One-shot random walks, one from every vertex of `starts`: returns (walks int32 len(starts) x (length + 1), -1 behind the end of
    a walk; lengths int32), and the visits (int64 per vertex) when asked for.  With `weights` (int32 >= 0 per entry) the steps are
    weighted; `bias` is a (return, in, out) triple of integers in 0 .. 65535, node2vec's 1/p, 1 and 1/q scaled to integers."""
    def prepare(p):
        p.set_option("length", length)
        p.set_option("seed", seed)
        p.set_option("weighted", 0 if weights is None else 1)
        for name, b in zip(("bias_return", "bias_in", "bias_out"), (1, 1, 1) if bias is None else bias):
            p.set_option(name, b)
        p.set_option("tries", tries)
        p.set_option("visits", 1 if visits else 0)
        p.reset(starts)

    def result(p):
        w, l, v, _ = p.extract(visits=bool(visits))
        return (w, l, v) if visits else (w, l)
    return _one_shot(RwProblem(device=device).init(nodes, row_offsets, col_indices, weights), prepare, RwProblem.enact, result)


SAMPLE_AUTO, SAMPLE_LANE, SAMPLE_GROUP = 0, 1, 2  # enum GRX_SAMPLE_* (gunrock_mi355x.h): option "strategy"
SAMPLE_TOO_LARGE = -4  # grx_sample_enact: a hop would have passed "edge_limit"


class SampleTooLarge(ArithmeticError):
    """SampleProblem.enact: the sampled edges would have passed the option "edge_limit" (GRX_SAMPLE_TOO_LARGE): the sampler of that hop
    did not run, the handle holds no result and takes the next reset / enact."""


class SampleProblem(_TunedProblem):
    """SampleProblem + SampleEnactor behind the handle C ABI: multi-hop fanout neighbourhood samples of the CSR as given (directed,
    self-loops and duplicates kept), renumbered to dense local ids.  Every draw is rw_draw(seed, vertex, hop, slot); without
    replacement the picks of a row are Robert Floyd's subset over those draws (gunrock_mi355x.h has the definition), so the sample is
    integers with one value: no option but "seed", "replace" and "weighted", the fanouts and the seeds changes it.  The build reads
    a device CSR (and the weights) and nothing later does.

    Options: "strategy" (SAMPLE_AUTO / SAMPLE_LANE / SAMPLE_GROUP), "seed", "replace", "weighted", "edge_limit", "long_row", "eids".
    device_results: "vertices": int32[V], "offsets": int64[V + 1], "cols": int32[E], "eids": int32[E] or None."""

    _family, _problem, _enactor = "sample", "SampleProblem", "SampleEnactor"
    _count = "entries"
    _results = ("vertices", "offsets", "cols", "eids")

    def __init__(self, instrument=False, device=0):
        super().__init__(instrument, device)
        self.hops = 0

    def init(self, nodes, row_offsets, col_indices, weights=None):
        return self._init_host(nodes, row_offsets, col_indices, per_entry=(weights, "weights", "entries"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_weights=None):
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_weights))

    def set_fanouts(self, fanouts):
        """the fanout of every hop: -1 (the whole row) or 1 .. 64, for 1 .. 16 hops"""
        f = _i32(fanouts).reshape(-1)
        _check(lib().grx_sample_set_fanouts(self._h, int(f.shape[0]), _p(f)), "grx_sample_set_fanouts")
        self.hops = int(f.shape[0])

    def reset(self, seeds):
        """the seeds: distinct vertices, the local ids 0 .. len(seeds) - 1"""
        s = _i32(seeds).reshape(-1)
        _check(lib().grx_sample_reset(self._h, int(s.shape[0]), _p(s)), "SampleProblem::Reset")

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds; SampleTooLarge when a hop would have passed the option edge_limit"""
        ms = C.c_float()
        rc = lib().grx_sample_enact(self._h, int(max_grid_size), C.byref(ms))
        if rc == SAMPLE_TOO_LARGE:
            raise SampleTooLarge("gunrockinst_amd: SampleEnactor::Enact refused: the sampled edges would pass edge_limit (code %d)" % rc)
        _check(rc, "SampleEnactor::Enact")
        return float(ms.value)

    def stats(self):
        hops = C.c_int()
        expanded, sampled, copied = ((C.c_longlong * 16)() for _ in range(3))
        long_rows, n, r = (C.c_longlong() for _ in range(3))
        k, b = C.c_double(), C.c_double()
        phases = (C.c_double * 4)()
        _check(lib().grx_sample_stats(self._h, C.byref(hops), expanded, sampled, copied, C.byref(long_rows), C.byref(n), C.byref(r), C.byref(k),
                                      phases, C.byref(b)), "grx_sample_stats")
        h = hops.value
        out = {"rows_expanded": [int(x) for x in expanded[:h]], "rows_sampled": [int(x) for x in sampled[:h]],
               "rows_copied": [int(x) for x in copied[:h]], "long_rows": long_rows.value, "kernel_launches": n.value, "readbacks": r.value,
               "kernel_ms": k.value, "build_ms": b.value}
        for name, ms in zip(("count_ms", "sample_ms", "renumber_ms", "relabel_ms"), phases):
            out[name] = float(ms)
        return out

    def sizes(self):
        """(V, E, vertex_ptr int64[H + 2], edge_ptr int64[H + 1]) of the last enact"""
        v, e = C.c_longlong(), C.c_longlong()
        vp, ep = np.zeros(self.hops + 2, dtype=np.int64), np.zeros(self.hops + 1, dtype=np.int64)
        _check(lib().grx_sample_sizes(self._h, C.byref(v), C.byref(e), _i64p(vp), _i64p(ep)), "grx_sample_sizes")
        return int(v.value), int(e.value), vp, ep

    def extract(self, eids=True):
        """{"vertices", "vertex_ptr", "offsets", "cols", "eids" (None when not asked for), "edge_ptr"}"""
        v, e, vp, ep = self.sizes()
        vertices, offsets, cols, ids = _out(v), _out(v + 1, np.int64), _out(e), _out(e, wanted=eids)
        _check(lib().grx_sample_extract(self._h, _p(vertices), _i64p(offsets), _p(cols), _opt(ids)), "SampleProblem::Extract")
        return {"vertices": vertices[:v], "vertex_ptr": vp, "offsets": offsets, "cols": cols[:e], "eids": _cut(ids, e), "edge_ptr": ep}


def gunrock_sample_neighbors(nodes, row_offsets, col_indices, seeds, fanouts, weights=None, replace=False, seed=0, device=0):
    """One-shot neighbourhood sample: the multi-hop subgraph of the distinct `seeds` under one fanout per hop (-1: whole rows), as a
    dict of the six arrays "vertices", "vertex_ptr", "offsets", "cols", "eids", "edge_ptr".  With `weights` (int32 >= 0 per entry)
    the picks are weighted, which needs `replace`."""
    def prepare(p):
        p.set_option("seed", seed)
        p.set_option("replace", 1 if replace else 0)
        p.set_option("weighted", 0 if weights is None else 1)
        p.set_fanouts(fanouts)
        p.reset(seeds)
    return _one_shot(SampleProblem(device=device).init(nodes, row_offsets, col_indices, weights), prepare, SampleProblem.enact,
                     SampleProblem.extract)


SIM_AUTO, SIM_LANE, SIM_WAVE, SIM_BLOCK, SIM_GLOBAL = 0, 1, 2, 3, 4  # enum GRX_SIM_* (gunrock_mi355x.h): option "strategy"
SIM_COMMON, SIM_JACCARD, SIM_OVERLAP, SIM_SORENSEN = 0, 1, 2, 3  # option "metric"
SIM_MAX_K = 64
SIM_TOO_LARGE = -4  # grx_sim_pairs / grx_sim_topk: the query is beyond what int32 offsets address


class SimTooLarge(ArithmeticError):
    """SimProblem.pairs / topk: more than INT_MAX pairs, or sources x k beyond INT_MAX (GRX_SIM_TOO_LARGE): nothing ran, the handle
    takes the next call"""


class SimProblem(_TunedProblem):
    """SimProblem + SimEnactor behind the handle C ABI: vertex similarity of the CSR read as an undirected simple graph -- common
    neighbours, Jaccard, overlap and Sorensen as exact fractions num / den (int64) with the float64 score num / den, for given pairs
    and as the k most similar vertices of given sources (score descending by exact comparison, then id ascending).  pairs / topk and
    their _device forms take the place of enact.  The build reads a device CSR and nothing later does.

    Options: "metric" (SIM_COMMON / SIM_JACCARD / SIM_OVERLAP / SIM_SORENSEN), "skip_neighbors", "strategy" (SIM_AUTO / SIM_LANE /
    SIM_WAVE / SIM_BLOCK / SIM_GLOBAL), "lane_max", "table_slots", "block_slots", "scratch_mib".
    device_results: the integer results (None without a result of that mode)."""

    _family, _problem, _enactor = "sim", "SimProblem", "SimEnactor"
    _count = "entries"
    _stats = (("simple_edges", "wedges", "wedges_walked", ("lane_pairs", "wave_pairs"), ("wave_sources", "block_sources", "global_sources"),
               ("wave_wedges", "block_wedges", "global_wedges"), "candidates", "table_probes", "kernel_launches"), ("kernel_ms", "build_ms"))
    _results = ("pair_common", "pair_num", "pair_den", "ids", "common", "num", "den", "count", "candidates")

    @property
    def enact(self):
        raise AttributeError("SimProblem has no enact: pairs() and topk() take its place")

    def __init__(self, instrument=False, device=0):
        super().__init__(instrument, device)
        self._pairs = 0
        self._rows = 0
        self._k = 1

    @staticmethod
    def _enacted(rc, what):
        if rc == SIM_TOO_LARGE:
            raise SimTooLarge("gunrockinst_amd: %s refused: the query is beyond int32 offsets (code %d)" % (what, rc))
        _check(rc, what)

    def pairs(self, u, v, max_grid_size=0):
        """scores the pairs (u[i], v[i]) given on the host; the elapsed milliseconds.  An id outside [0, nodes) raises (code -1)"""
        u, v = _i32(u).ravel(), _i32(v).ravel()
        if u.shape != v.shape:
            raise ValueError("gunrockinst_amd: %d and %d pair ends" % (u.shape[0], v.shape[0]))
        ms = C.c_float()
        self._pairs = 0
        self._enacted(lib().grx_sim_pairs(self._h, int(u.shape[0]), _p(u), _p(v), int(max_grid_size), C.byref(ms)), "SimEnactor::EnactPairs")
        self._pairs = int(u.shape[0])
        return float(ms.value)

    def pairs_device(self, num_pairs, d_u, d_v, max_grid_size=0):
        """the same for int32 arrays in device memory, which stay the caller's"""
        ms = C.c_float()
        self._pairs = 0
        self._enacted(lib().grx_sim_pairs_device(self._h, int(num_pairs), C.c_void_p(d_u), C.c_void_p(d_v), int(max_grid_size), C.byref(ms)),
                      "SimEnactor::EnactPairs(device)")
        self._pairs = int(num_pairs)
        return float(ms.value)

    def topk(self, sources, k, max_grid_size=0):
        """the k most similar vertices of every source given on the host; the elapsed milliseconds"""
        s = _i32(sources).ravel()
        ms = C.c_float()
        self._rows = 0
        self._enacted(lib().grx_sim_topk(self._h, int(s.shape[0]), _p(s), int(k), int(max_grid_size), C.byref(ms)), "SimEnactor::EnactTopk")
        self._rows, self._k = int(s.shape[0]), int(k)
        return float(ms.value)

    def topk_device(self, num_sources, d_sources, k, max_grid_size=0):
        ms = C.c_float()
        self._rows = 0
        self._enacted(lib().grx_sim_topk_device(self._h, int(num_sources), C.c_void_p(d_sources), int(k), int(max_grid_size), C.byref(ms)),
                      "SimEnactor::EnactTopk(device)")
        self._rows, self._k = int(num_sources), int(k)
        return float(ms.value)

    def extract_pairs(self):
        """{"common": int32, "num", "den": int64, "score": float64}, one entry per pair of the last pairs()"""
        count = self._pairs
        common, num, den, score = _out(count), _out(count, np.int64), _out(count, np.int64), _out(count, np.float64)
        _check(lib().grx_sim_extract_pairs(self._h, _p(common), _i64p(num), _i64p(den), _f64p(score)), "SimProblem::ExtractPairs")
        return {"common": common[:count], "num": num[:count], "den": den[:count], "score": score[:count]}

    def extract_topk(self):
        """{"ids", "common": int32 (S, k); "num", "den": int64 (S, k); "score": float64 (S, k); "count", "candidates": int32 (S)} of the
        last topk(); ids are -1 and the rest 0 beyond count[s]"""
        rows, k = self._rows, self._k
        count = rows * k
        ids, common, num, den, score = _out(count), _out(count), _out(count, np.int64), _out(count, np.int64), _out(count, np.float64)
        kept, candidates = _out(rows), _out(rows)
        _check(lib().grx_sim_extract_topk(self._h, _p(ids), _p(common), _i64p(num), _i64p(den), _f64p(score), _p(kept), _p(candidates)),
               "SimProblem::ExtractTopk")
        out = {name: a[:count].reshape(rows, k) for name, a in (("ids", ids), ("common", common), ("num", num), ("den", den), ("score", score))}
        out["count"], out["candidates"] = kept[:rows], candidates[:rows]
        return out


def gunrock_similarity(offsets, cols, u, v, metric=SIM_JACCARD, device=0):
    """One-shot pair similarity on the CSR (offsets, cols): returns {"common", "num", "den", "score"}, one entry per pair (u[i], v[i])."""
    offsets = _i32(offsets)
    return _one_shot(SimProblem(device=device).init(offsets.shape[0] - 1, offsets, cols), lambda p: p.set_option("metric", metric),
                     lambda p: p.pairs(u, v), SimProblem.extract_pairs)


def gunrock_similar_vertices(offsets, cols, sources, k, metric=SIM_JACCARD, skip_neighbors=False, device=0):
    """One-shot top-k similarity on the CSR (offsets, cols): the k most similar vertices of every source, as {"ids", "common", "num",
    "den", "score"} of shape (S, k) and {"count", "candidates"} of shape (S); with skip_neighbors the neighbours of a source are no
    candidates."""
    offsets = _i32(offsets)

    def prepare(p):
        p.set_option("metric", metric)
        p.set_option("skip_neighbors", 1 if skip_neighbors else 0)
    return _one_shot(SimProblem(device=device).init(offsets.shape[0] - 1, offsets, cols), prepare, lambda p: p.topk(sources, k),
                     SimProblem.extract_topk)


SPGEMM_AUTO, SPGEMM_LANE, SPGEMM_WAVE, SPGEMM_BLOCK, SPGEMM_GLOBAL = 0, 1, 2, 3, 4  # enum GRX_SPGEMM_* (gunrock_mi355x.h): option "strategy"
SPGEMM_SELF, SPGEMM_TRANSPOSE, SPGEMM_GIVEN = 0, 1, 2  # option "right"
SPGEMM_TOO_LARGE = -4  # grx_spgemm_enact: nnz(C) or the products of one row are beyond what int32 addresses
SPGEMM_OVERFLOW = -7  # grx_spgemm_enact: the bound on the values reached "count_limit"


class SpgemmTooLarge(ArithmeticError):
    """SpgemmProblem.enact: nnz(C) or the products of one row beyond INT_MAX (GRX_SPGEMM_TOO_LARGE): no result was written, the
    handle takes the next call"""


class SpgemmOverflow(ArithmeticError):
    """SpgemmProblem.enact: max over i of sum over k in A[i] of |a_ik| sum over j of |b_kj| reached "count_limit"
    (GRX_SPGEMM_OVERFLOW): no result was written, the handle takes the next call"""


def _matrix(m):
    """((rows, cols), offsets, cols, vals or None) as contiguous int32 from (offsets, cols[, vals]) -- square, of len(offsets) - 1
    rows -- or (shape, offsets, cols[, vals])"""
    m = tuple(m)
    shape = None
    # three parts whose first has two numbers: a shape when the second is the offsets of that many rows over the third (the one-row
    # matrix (offsets, cols, vals) is not: its column would have to be 1 of 1)
    if len(m) == 4 or (len(m) == 3 and m[2] is not None and len(m[0]) == 2 and len(m[1]) == int(m[0][0]) + 1
                       and int(np.asarray(m[1])[-1]) == len(m[2])):
        shape, m = (int(m[0][0]), int(m[0][1])), m[1:]
    if len(m) not in (2, 3):
        raise ValueError("gunrockinst_amd: a matrix is (offsets, cols[, vals]) or (shape, offsets, cols[, vals])")
    ro, ci = _i32(m[0]).ravel(), _i32(m[1]).ravel()
    vals = None if len(m) == 2 or m[2] is None else _i32(m[2]).ravel()
    if shape is None:
        shape = (ro.shape[0] - 1,) * 2
    _check_offsets(ro, shape[0])
    if vals is not None and vals.shape != ci.shape:
        raise ValueError("gunrockinst_amd: %d values for %d entries" % (vals.shape[0], ci.shape[0]))
    return shape, ro, ci, vals


class SpgemmProblem(_TunedProblem):
    """SpgemmProblem + SpgemmEnactor behind the handle C ABI: the sparse product C = A B of CSR matrices with int32 values (absent: 1
    each) read as given -- duplicates add, rows in any order -- as a CSR with strictly ascending rows and exact int64 values.  C is
    structural: an entry whose products cancel is stored with the value 0.  Its operands are matrices with a shape, so init,
    init_device and the constructor's attributes (rows, inner, entries) are its own.

    Options: "right" (SPGEMM_SELF / SPGEMM_TRANSPOSE / SPGEMM_GIVEN), "pattern_only", "strategy" (SPGEMM_AUTO / SPGEMM_LANE /
    SPGEMM_WAVE / SPGEMM_BLOCK / SPGEMM_GLOBAL), "lane_max", "table_slots", "block_slots", "scratch_mib", "count_limit".
    device_results: "offsets", "cols": int32; "vals": int64 (None without a result, or without entries or values)."""

    _family, _problem, _enactor = "spgemm", "SpgemmProblem", "SpgemmEnactor"
    _results = ("offsets", "cols", "vals")
    _REGIMES = ("lane", "wave", "block", "global")

    def __init__(self, instrument=False, device=0):
        self._create("grx_spgemm_create", int(instrument), device)
        self.rows = 0
        self.inner = 0
        self.entries = 0

    def init(self, shape, offsets, cols, vals=None):
        """A of shape (rows, inner) from the host"""
        (self.rows, self.inner), ro, ci, v = _matrix((shape, offsets, cols, vals))
        self.entries = int(ci.shape[0])
        _check(lib().grx_spgemm_init(self._h, self.rows, self.inner, self.entries, _p(ro), _p(ci), _opt(v)), "SpgemmProblem::Init")
        return self

    def init_device(self, shape, nnz, d_offsets, d_cols, d_vals=None):
        """the CSR stays the caller's and must outlive the handle's enacts"""
        self.rows, self.inner, self.entries = int(shape[0]), int(shape[1]), int(nnz)
        _check(lib().grx_spgemm_init_device(self._h, self.rows, self.inner, self.entries, C.c_void_p(d_offsets), C.c_void_p(d_cols),
                                            C.c_void_p(d_vals)), "SpgemmProblem::Init(device)")
        return self

    def set_right(self, shape, offsets, cols, vals=None):
        """B of shape (inner, cols) from the host; selects SPGEMM_GIVEN.  Returns the library's code: 0, -1 (B's rows are not A's
        inner) or -2 (not a CSR); anything else raises"""
        (rows, ncols), ro, ci, v = _matrix((shape, offsets, cols, vals))
        rc = lib().grx_spgemm_set_right(self._h, rows, ncols, int(ci.shape[0]), _p(ro), _p(ci), _opt(v))
        if rc not in (0, -1, -2):
            _check(rc, "SpgemmProblem::SetRight")
        return rc

    def set_right_device(self, shape, nnz, d_offsets, d_cols, d_vals=None):
        rc = lib().grx_spgemm_set_right_device(self._h, int(shape[0]), int(shape[1]), int(nnz), C.c_void_p(d_offsets), C.c_void_p(d_cols),
                                               C.c_void_p(d_vals))
        if rc not in (0, -1, -2):
            _check(rc, "SpgemmProblem::SetRight(device)")
        return rc

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds; SpgemmTooLarge / SpgemmOverflow when the product was refused.  A shape the right operand does
        not fit raises (code -1)"""
        ms = C.c_float()
        rc = lib().grx_spgemm_enact(self._h, int(max_grid_size), C.byref(ms))
        if rc == SPGEMM_TOO_LARGE:
            raise SpgemmTooLarge("gunrockinst_amd: SpgemmEnactor::Enact refused: the product is beyond int32 offsets (code %d)" % rc)
        if rc == SPGEMM_OVERFLOW:
            raise SpgemmOverflow("gunrockinst_amd: SpgemmEnactor::Enact refused: the bound %.17g reached count_limit (code %d)"
                                 % (self.stats()["bound"], rc))
        _check(rc, "SpgemmEnactor::Enact")
        return float(ms.value)

    def stats(self):
        rows, products = (C.c_longlong * 4)(), (C.c_longlong * 4)()
        total, nnz, probes, n, r = (C.c_longlong() for _ in range(5))
        bound, k, regime_ms = C.c_double(), C.c_double(), (C.c_double * 4)()
        _check(lib().grx_spgemm_stats(self._h, rows, products, C.byref(total), C.byref(nnz), C.byref(probes), C.byref(n), C.byref(r),
                                      C.byref(bound), C.byref(k), regime_ms), "grx_spgemm_stats")
        out = {"products": total.value, "nnz": nnz.value, "table_probes": probes.value, "kernel_launches": n.value, "readbacks": r.value,
               "bound": bound.value, "kernel_ms": k.value}
        for i, name in enumerate(self._REGIMES):
            out[name + "_rows"], out[name + "_products"], out[name + "_ms"] = int(rows[i]), int(products[i]), float(regime_ms[i])
        return out

    def sizes(self):
        """(rows, cols, nnz) of the result"""
        rows, cols, nnz = C.c_int(), C.c_int(), C.c_longlong()
        _check(lib().grx_spgemm_sizes(self._h, C.byref(rows), C.byref(cols), C.byref(nnz)), "grx_spgemm_sizes")
        return rows.value, cols.value, nnz.value

    def extract(self, values=True):
        """{"offsets": int32[rows + 1], "cols": int32[nnz], "vals": int64[nnz] or None, "shape": (rows, cols)} of the last enact"""
        rows, cols, nnz = self.sizes()
        offsets, ci, vals = _out(rows + 1), _out(nnz), _out(nnz, np.int64, values)
        _check(lib().grx_spgemm_extract(self._h, _p(offsets), _p(ci), _opt(vals)), "SpgemmProblem::Extract")
        return {"offsets": offsets, "cols": ci[:nnz], "vals": _cut(vals, nnz), "shape": (rows, cols)}


def gunrock_spgemm(a, b=None, transpose_right=False, pattern_only=False, device=0):
    """One-shot sparse product: A A (b None), A A^T (transpose_right) or A B.  A matrix is (offsets, cols[, vals]) -- square -- or
    (shape, offsets, cols[, vals]), CSR with int32 values (absent: 1 each).  Returns {"offsets", "cols", "vals", "shape"}: rows
    strictly ascending, vals int64 (None with pattern_only); an entry whose products cancel is stored as 0."""
    if b is not None and transpose_right:
        raise ValueError("gunrockinst_amd: a right operand and transpose_right exclude each other")
    shape, ro, ci, vals = _matrix(a)

    def prepare(p):
        p.set_option("pattern_only", 1 if pattern_only else 0)
        if transpose_right:
            p.set_option("right", SPGEMM_TRANSPOSE)
        if b is not None:
            _check(p.set_right(*_matrix(b)), "SpgemmProblem::SetRight")
    return _one_shot(SpgemmProblem(device=device).init(shape, ro, ci, vals), prepare, SpgemmProblem.enact,
                     lambda p: p.extract(values=not pattern_only))


def gunrock_quotient_graph(offsets, cols, weights, labels, device=0):
    """The contraction P^T A P of the square CSR (offsets, cols) with int32 weights (None: 1 each) by any label map onto 0 .. c - 1
    (int32 per vertex; LpProblem's dense community ids fit as they are): entry (x, y) is the sum of the weights of the entries that
    lead from label x to label y, self-loops included.  Two products: T = A P, then P^T T.  Returns {"offsets", "cols", "vals",
    "shape"}; SpgemmOverflow when a value of T leaves int32."""
    labels = _i32(labels).ravel()
    n = _i32(offsets).shape[0] - 1
    if labels.shape[0] != n:
        raise ValueError("gunrockinst_amd: %d labels for %d vertices" % (labels.shape[0], n))
    if n and int(labels.min()) < 0:
        raise ValueError("gunrockinst_amd: a negative label")
    c = int(labels.max()) + 1 if n else 0
    p = ((n, c), np.arange(n + 1, dtype=np.int32), labels)  # row v holds the one entry (v, labels[v])
    order = np.argsort(labels, kind="stable").astype(np.int32)
    pt = ((c, n), np.concatenate(([0], np.cumsum(np.bincount(labels, minlength=c)))).astype(np.int32), order)
    t = gunrock_spgemm(((n, n), offsets, cols, weights), p, device=device)
    if t["vals"].shape[0] and (int(t["vals"].max()) > 0x7FFFFFFF or int(t["vals"].min()) < -0x80000000):
        raise SpgemmOverflow("gunrockinst_amd: gunrock_quotient_graph: a weight sum of A P leaves int32")
    return gunrock_spgemm(pt, ((n, c), t["offsets"], t["cols"], t["vals"].astype(np.int32)), device=device)


LP_SYNC, LP_CLASSES = 0, 1  # enum GRX_LP_* (gunrock_mi355x.h): option "mode"
LP_AUTO, LP_LANE, LP_WAVE, LP_BLOCK = 0, 1, 2, 3  # option "strategy"
LP_CONVERGED, LP_PERIOD2, LP_CAPPED = 0, 1, 2  # stats()["state"]: how the last enact ended
LP_BAD_CLASSES = -8  # grx_lp_set_classes: a pair has both ends in one class


class LpProblem(_TunedProblem):
    """LpProblem + LpEnactor behind the handle C ABI: label-propagation communities of the CSR read as an undirected simple graph
    with int32 weights of at least 1 (None: 1 each; a pair's weight is the largest of its entries).  Integer scores and a total tie
    rule (keep the current label, else the smallest): every label has one value after any number of rounds.  The build reads a
    device CSR (and the weights) and nothing later does; stats()["state"] tells how the last enact ended.

    Options: "mode" (LP_CLASSES / LP_SYNC), "strategy" (LP_AUTO / LP_LANE / LP_WAVE / LP_BLOCK), "lane_max_row", "wave_max_row",
    "table_slots", "max_rounds".
    device_results: "labels", "community": int32 per vertex."""

    _family, _problem, _enactor = "lp", "LpProblem", "LpEnactor"
    _count = "entries"
    _stats = (("pairs", "rounds", "state", "visits", "entries_read", ("regime_rows", 3), "fallback_rows", "kernel_launches", "readbacks"),
              ("kernel_ms", "build_ms"))
    _results = ("labels", "community")

    def init(self, nodes, row_offsets, col_indices, weights=None):
        return self._init_host(nodes, row_offsets, col_indices, per_entry=(weights, "weights", "entries"))

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_weights=None):
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_weights))

    def set_classes(self, classes, num_classes=None):
        """a proper colouring for LP_CLASSES: int32 per vertex in [0, num_classes) (None: max + 1); returns the library's code:
        0 = installed, LP_BAD_CLASSES = a pair has both ends in one class and nothing is installed (anything else raises)"""
        cl = _i32_of(classes, self.nodes, "classes", "nodes")
        count = int(cl.max()) + 1 if num_classes is None else int(num_classes)
        rc = lib().grx_lp_set_classes(self._h, _p(cl), count)
        if rc not in (0, LP_BAD_CLASSES):
            _check(rc, "LpProblem::SetClasses")
        return rc

    def reset(self, labels=None):
        """L[v] = labels[v] (int32 in [0, nodes)), or v for None"""
        self._reset_labels(labels)

    def round_trace(self):
        """per round of the last enact, the closing one included: (vertices visited, labels changed) as int64"""
        return _count_then_fill(lib().grx_lp_round_trace, self._h, "grx_lp_round_trace", (np.int64, np.int64))

    def extract(self):
        """(labels int32 per vertex, community int32 per vertex: the rank of its label among the labels in use, communities)"""
        labels, community, count = _out(self.nodes), _out(self.nodes), C.c_longlong()
        _check(lib().grx_lp_extract(self._h, _p(labels), _p(community), C.byref(count)), "LpProblem::Extract")
        return labels[:self.nodes], community[:self.nodes], int(count.value)

    def summary(self):
        """{"size", "internal", "volume": int64 per community, "W": the sum of all pair weights}"""
        count, total = C.c_longlong(), C.c_longlong()
        _check(lib().grx_lp_extract(self._h, None, None, C.byref(count)), "LpProblem::Extract")
        k = int(count.value)
        size, internal, volume = (_out(k, np.int64) for _ in range(3))
        _check(lib().grx_lp_summary(self._h, _i64p(size), _i64p(internal), _i64p(volume), C.byref(total)), "LpProblem::Summary")
        return {"size": size[:k], "internal": internal[:k], "volume": volume[:k], "W": int(total.value)}


def modularity_from_sums(internal, volume, W):
    """Newman's modularity in float64 from LpProblem.summary()'s integers: sum(internal / W - (volume / (2 W))^2); 0.0 without a pair"""
    if int(W) == 0:
        return 0.0
    internal, volume = np.asarray(internal, np.float64), np.asarray(volume, np.float64)
    return float(np.sum(internal / float(W) - (volume / (2.0 * float(W))) ** 2))


def gunrock_label_propagation(nodes, row_offsets, col_indices, weights=None, mode=LP_CLASSES, labels=None, max_rounds=0, seed=0, device=0):
    """One-shot label propagation: returns (labels, community, communities, state, rounds).  In LP_CLASSES mode the classes are
    gunrock_color(seed=seed)'s colours."""
    colours = None
    if mode == LP_CLASSES:
        colours = gunrock_color(nodes, row_offsets, col_indices, seed=seed, device=device)[0]

    def prepare(p):
        p.set_option("mode", mode)
        p.set_option("max_rounds", max_rounds)
        if colours is not None:
            _check(p.set_classes(np.asarray(colours, np.int32) - 1), "LpProblem::SetClasses")
        p.reset(labels)

    def result(p):
        st = p.stats()
        return p.extract() + (st["state"], st["rounds"])
    return _one_shot(LpProblem(device=device).init(nodes, row_offsets, col_indices, weights), prepare, LpProblem.enact, result)


WL_AUTO, WL_LANE, WL_WAVE, WL_BLOCK = 0, 1, 2, 3  # enum GRX_WL_* (gunrock_mi355x.h): option "strategy"
WL_STABLE, WL_CAPPED = 0, 1  # stats()["state"]: how the last enact ended
WL_TOO_LARGE, WL_NOT_CERTIFIED = -4, -5  # grx_wl_enact's codes next to -1


class WlTooLarge(ArithmeticError):
    """the history of a colour refinement, (max_rounds + 1) * nodes colours, is beyond int32 offsets: nothing ran"""


class WlNotCertified(RuntimeError):
    """more than "max_repairs" certificates of a colour refinement failed: there is no result"""


def wl_mix(seed, attempt, colour):
    """The 128-bit mix of one entry of a row as (lo, hi): app/wl/wl_functor.hpp's Mix().  The signature of a row in signature pass
    `attempt` (1, 2, ...) is the wrapping 128-bit sum of the mixes of its entries' colours, a colour being the smallest member of a
    class, cut to its top "sig_bits" bits."""
    m = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & m
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        return x ^ (x >> 31)
    x = ((int(attempt) << 32) | (int(colour) & 0xFFFFFFFF)) & m
    return mix((int(seed) & m) ^ mix(x)), mix((int(seed) & m) ^ mix(x ^ m))


class WlProblem(_TunedProblem):
    """WlProblem + WlEnactor behind the handle C ABI: colour refinement (1-WL) of the CSR as given -- a row is the multiset of its
    entries -- from the classes of any int32 start labels down to the coarsest equitable partition, or for a fixed number of rounds.
    The classes are numbered by ascending smallest member; every result is certified by an exact comparison of rows.  A device CSR
    stays the caller's and is read by every enact: it has to outlive the handle.

    Options: "strategy" (WL_AUTO / WL_LANE / WL_WAVE / WL_BLOCK), "lane_max_row", "wave_max_row", "max_rounds", "history",
    "max_repairs", "sig_bits", "seed", "table_slots", "block_slots", "scratch_mib".
    device_results: "colour": int32 per vertex, "class_size": int64 per class, "representative": int32 per class."""

    _family, _problem, _enactor = "wl", "WlProblem", "WlEnactor"
    _count = "entries"
    _stats = (("entries", "rounds", "state", "classes", "repairs", "certificate_runs", ("regime_rows", 3), ("rung_rows", 3), "kernel_launches",
               "readbacks"), ("kernel_ms",))
    _results = ("colour", "class_size", "representative")

    def reset(self, labels=None):
        """the start labels: int32 of any value per vertex, or None for one class"""
        self._reset_labels(labels)

    def enact(self, max_grid_size=0):
        """the elapsed milliseconds; stats()["state"] tells how it ended.  WlNotCertified, WlTooLarge: there is no result"""
        ms = C.c_float()
        rc = lib().grx_wl_enact(self._h, int(max_grid_size), C.byref(ms))
        if rc == WL_NOT_CERTIFIED:
            raise WlNotCertified("gunrockinst_amd: WlEnactor::Enact: more certificates failed than max_repairs allows")
        if rc == WL_TOO_LARGE:
            raise WlTooLarge("gunrockinst_amd: WlEnactor::Enact: the history is beyond int32 offsets")
        _check(rc, "WlEnactor::Enact")
        return float(ms.value)

    def round_trace(self):
        """the classes behind the labels and behind each committed round of the last enact, int64 (rounds + 1 entries)"""
        return _count_then_fill(lib().grx_wl_round_trace, self._h, "grx_wl_round_trace", (np.int64,))[0]

    def extract(self):
        """(colour int32 per vertex, class_size int64 per class, representative int32 per class: its smallest member)"""
        count = C.c_longlong()
        _check(lib().grx_wl_extract(self._h, None, None, None, C.byref(count)), "WlProblem::Extract")
        k = int(count.value)
        colour, size, rep = _out(self.nodes), _out(k, np.int64), _out(k)
        _check(lib().grx_wl_extract(self._h, _p(colour), _i64p(size), _p(rep), None), "WlProblem::Extract")
        return colour[:self.nodes], size[:k], rep[:k]

    def history(self):
        """the dense colouring behind every round 0 .. rounds of the last enact with "history": int32, (rounds + 1) x nodes"""
        rounds = self.stats()["rounds"]
        out = np.empty((rounds + 1, max(self.nodes, 1)), np.int32)
        for h in range(rounds + 1):
            _check(lib().grx_wl_history(self._h, h, _p(out[h]), None), "WlProblem::History")
        return out[:, :self.nodes]


def gunrock_colour_refinement(nodes, row_offsets, col_indices, labels=None, max_rounds=-1, history=False, seed=0, device=0):
    """One-shot colour refinement: returns {"colour", "class_size", "representative", "classes", "state", "rounds"} and, with
    history (max_rounds in 1 .. 64), "history": the colouring behind every round, the WL-h features for h = 0 .. rounds."""
    def prepare(p):
        p.set_option("max_rounds", max_rounds)
        p.set_option("history", 1 if history else 0)
        p.set_option("seed", seed)
        p.reset(labels)

    def result(p):
        st = p.stats()
        colour, size, rep = p.extract()
        out = {"colour": colour, "class_size": size, "representative": rep, "classes": st["classes"], "state": st["state"],
               "rounds": st["rounds"]}
        if history:
            out["history"] = p.history()
        return out
    return _one_shot(WlProblem(device=device).init(nodes, row_offsets, col_indices), prepare, WlProblem.enact, result)


def gunrock_wl_test(graph_a, graph_b, labels_a=None, labels_b=None, device=0):
    """The 1-WL isomorphism screen of two graphs, each (row_offsets, col_indices): the disjoint union is refined and the class
    histograms of the two halves compared.  False: the graphs are certainly not isomorphic; True: 1-WL cannot tell them apart.
    Labels are given for both graphs or for neither."""
    if (labels_a is None) != (labels_b is None):
        raise ValueError("gunrockinst_amd: labels for one graph only")
    (ro_a, ci_a), (ro_b, ci_b) = _csr_arrays(*graph_a), _csr_arrays(*graph_b)
    na, nb = ro_a.shape[0] - 1, ro_b.shape[0] - 1
    if na != nb or ci_a.shape[0] != ci_b.shape[0]:
        return False
    if na == 0:
        return True
    ro = np.concatenate([ro_a, ro_b[1:] + ro_a[-1]]).astype(np.int32)
    ci = np.concatenate([ci_a, ci_b + na]).astype(np.int32)
    labels = None if labels_a is None else np.concatenate([_i32(labels_a).ravel(), _i32(labels_b).ravel()])
    got = gunrock_colour_refinement(na + nb, ro, ci, labels=labels, device=device)
    k = got["classes"]
    return bool(np.array_equal(np.bincount(got["colour"][:na], minlength=k), np.bincount(got["colour"][na:], minlength=k)))


MSBFS_AUTO, MSBFS_PUSH, MSBFS_PULL, MSBFS_ALTERNATE = 0, 1, 2, 3  # enum GRX_MSBFS_* (gunrock_mi355x.h): option "direction"
MSBFS_INVERSE_AUTO, MSBFS_INVERSE_NONE, MSBFS_INVERSE_SELF, MSBFS_INVERSE_BUILD = 0, 1, 2, 3  # enum GRX_MSBFS_INVERSE_*: option "inverse"
MSBFS_LEVEL_PUSH, MSBFS_LEVEL_PULL = 0, 1  # enum GRX_MSBFS_LEVEL_*: the kinds of level_trace()
MSBFS_DEPTHS_NOT_STORED, MSBFS_INVERSE_NOT_SYMMETRIC = -4, -5  # the family's codes next to -1 / -2 / -3


class MsbfsProblem(_TunedProblem):
    """MsbfsProblem + MsbfsEnactor behind the handle C ABI: breadth-first searches from k sources on the CSR read as a directed
    multigraph, 64 sources per pass over the edges.  All results are integers: depths(), source_summary(), vertex_summary().

    Options: "direction" (MSBFS_AUTO / MSBFS_PUSH / MSBFS_PULL / MSBFS_ALTERNATE), "inverse" (MSBFS_INVERSE_*, settled by the next
    reset), "alpha", "beta", "wave_min_row".
    device_results: device pointers of (depth or None, reached, dist_sum, ecc, sources_reaching, in_dist_sum)."""

    _family, _problem, _enactor = "msbfs", "MsbfsProblem", "MsbfsEnactor"
    _stats = (("batches", "levels", "push_levels", "pull_levels", "entries_read", "kernel_launches"), ("kernel_ms", "build_ms"))
    _results = 6

    def __init__(self, instrument=False, device=0):
        super().__init__(instrument, device)
        self.sources = 0

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_inv_row_offsets=None, d_inv_col_indices=None):
        """a CSR in HBM (borrowed); the in-neighbour lists too when both inverse pointers are given"""
        return self._init_device(nodes, edges, d_row_offsets, d_col_indices, C.c_void_p(d_inv_row_offsets), C.c_void_p(d_inv_col_indices))

    def reset(self, sources, store_depths=True):
        """the sources (vertex ids, repeats allowed, at least one) of the next enact.  Raises with code -1 for a source outside
        [0, nodes) and with code -5 when "inverse" is MSBFS_INVERSE_SELF and the graph is not symmetric; the handle stays usable"""
        src = _i32(sources).reshape(-1)
        _check(lib().grx_msbfs_reset(self._h, _p(src), int(src.shape[0]), int(bool(store_depths))), "MsbfsProblem::Reset")
        self.sources = int(src.shape[0])

    def level_trace(self):
        """the levels of the last enact in order: (batch, level, kind: MSBFS_LEVEL_PUSH / MSBFS_LEVEL_PULL) as int32, (frontier
        vertices, frontier out-row entries) as int64, milliseconds as float64 (0 unless instrumented)"""
        return _count_then_fill(lib().grx_msbfs_level_trace, self._h, "grx_msbfs_level_trace",
                                (np.int32,) * 3 + (np.int64,) * 2 + (np.float64,))

    def depths(self, first=0, count=None):
        """depth[first : first + count] as int32 [count, nodes]; raises with code -4 after a reset with store_depths off"""
        count = self.sources - int(first) if count is None else int(count)
        out = np.empty((max(count, 0), self.nodes), dtype=np.int32)
        _check(lib().grx_msbfs_extract_depths(self._h, int(first), count, _p(out)), "MsbfsProblem::ExtractDepths")
        return out

    def source_summary(self):
        """(reached int64, dist_sum int64, ecc int32), one entry per source"""
        k = self.sources
        reached, dist_sum, ecc = _out(k, np.int64), _out(k, np.int64), _out(k)
        _check(lib().grx_msbfs_source_summary(self._h, _i64p(reached), _i64p(dist_sum), _p(ecc)), "MsbfsProblem::SourceSummary")
        return reached[:k], dist_sum[:k], ecc[:k]

    def vertex_summary(self):
        """(sources_reaching int32, in_dist_sum int64), one entry per vertex"""
        reaching, in_dist_sum = _out(self.nodes), _out(self.nodes, np.int64)
        _check(lib().grx_msbfs_vertex_summary(self._h, _p(reaching), _i64p(in_dist_sum)), "MsbfsProblem::VertexSummary")
        return reaching[:self.nodes], in_dist_sum[:self.nodes]


def closeness_from_sums(nodes, sources, sources_reaching, in_dist_sum, wf_improved=True):
    """float64 closeness per vertex from MS-BFS's integers, in the formula of networkx.closeness_centrality on incoming distances:
    r = the sources other than v itself that reach v, c = r / in_dist_sum (0 where the sum is 0), times r / (nodes - 1) with
    wf_improved (Wasserman-Faust).  With every vertex as a source this is networkx's value."""
    own = np.bincount(np.asarray(sources, dtype=np.int64).reshape(-1), minlength=int(nodes))
    r = (np.asarray(sources_reaching, dtype=np.int64) - own).astype(np.float64)
    total = np.asarray(in_dist_sum, dtype=np.int64).astype(np.float64)
    c = np.zeros(int(nodes), dtype=np.float64)
    some = total > 0
    c[some] = r[some] / total[some]
    if wf_improved and nodes > 1:
        c *= r / (float(nodes) - 1.0)
    return c


def gunrock_msbfs(nodes, row_offsets, col_indices, sources, device=0):
    """One-shot multi-source BFS: returns (depth int32 [k, nodes], reached int64 [k], dist_sum int64 [k], ecc int32 [k])."""
    return _one_shot(MsbfsProblem(device=device).init(nodes, row_offsets, col_indices), lambda p: p.reset(sources), MsbfsProblem.enact,
                     lambda p: (p.depths(),) + p.source_summary())


def gunrock_closeness(nodes, row_offsets, col_indices, sources=None, wf_improved=True, device=0):
    """One-shot closeness centrality on incoming distances (float64 per vertex, closeness_from_sums' formula).  sources None: every
    vertex, which gives networkx.closeness_centrality(G, wf_improved=wf_improved) of the digraph; the depths are not stored."""
    src = np.arange(int(nodes), dtype=np.int32) if sources is None else _i32(sources).reshape(-1)
    reaching, in_dist_sum = _one_shot(MsbfsProblem(device=device).init(nodes, row_offsets, col_indices),
                                      lambda p: p.reset(src, store_depths=False), MsbfsProblem.enact, MsbfsProblem.vertex_summary)
    return closeness_from_sums(nodes, src, reaching, in_dist_sum, wf_improved)


def gunrock_eccentricity(nodes, row_offsets, col_indices, device=0):
    """One-shot eccentricities: returns (ecc int32 per vertex, diameter, radius).  ecc[v] is the largest FINITE distance from v, so
    on a graph that is not strongly connected it is taken inside what v reaches (0 for a vertex without out-edges); diameter and
    radius are the largest and the smallest ecc, i.e. the diameter is the largest finite distance between any two vertices and
    is not infinite for a disconnected graph."""
    src = np.arange(int(nodes), dtype=np.int32)
    ecc = _one_shot(MsbfsProblem(device=device).init(nodes, row_offsets, col_indices), lambda p: p.reset(src, store_depths=False),
                    MsbfsProblem.enact, lambda p: p.source_summary()[2].copy())
    return ecc, int(ecc.max()), int(ecc.min())


def gunrock_bc(nodes, row_offsets, col_indices, src=-1, queue_size=1.0, src_mode=SRC_MANUALLY, device=0):
    """Call gunrock_bc_func as reference shared_lib_tests/test_bc.c does (src -1 = every vertex in turn); returns
    (bc_values, ebc_values) as float32 arrays."""
    ro, ci = _csr_arrays(row_offsets, col_indices)
    gin = _graph_struct(nodes, ro, ci)
    gout = GunrockGraph()
    cfg = GunrockConfig()
    cfg.src_node, cfg.device, cfg.queue_size, cfg.src_mode = src, device, queue_size, src_mode
    dt = GunrockDataType(VTXID_INT, SIZET_INT, VALUE_FLOAT)
    lib().gunrock_bc_func(C.byref(gout), C.byref(gin), cfg, dt)
    edges = int(ci.shape[0])
    eptr = gout.edge_values
    bc = _take_node_values(gout, nodes, np.float32)
    if not eptr:
        raise RuntimeError("gunrockinst_amd: the call produced no edge_values")
    ebc = np.ctypeslib.as_array(C.cast(eptr, C.POINTER(C.c_float)), shape=(max(edges, 1),))[:edges].copy()
    C.CDLL(None).free(C.c_void_p(eptr))
    return bc, ebc


def gunrock_pr(nodes, row_offsets, col_indices, src=-1, delta=0.85, error=0.01, max_iter=20, top_nodes=0, src_mode=SRC_MANUALLY,
               device=0):
    """Call gunrock_pr_func as reference shared_lib_tests/test_pr.c does; returns (node_ids, page_rank) in descending rank order
    (top_nodes entries, all of them when top_nodes <= 0)."""
    ro, ci = _csr_arrays(row_offsets, col_indices)
    gin = _graph_struct(nodes, ro, ci)
    gout = GunrockGraph()
    cfg = GunrockConfig()
    cfg.src_node, cfg.device, cfg.src_mode = src, device, src_mode
    cfg.delta, cfg.error, cfg.max_iter, cfg.top_nodes = delta, error, max_iter, top_nodes
    count = nodes if top_nodes <= 0 else min(nodes, top_nodes)
    ids, ranks = _out(count), _out(count, np.float32)
    dt = GunrockDataType(VTXID_INT, SIZET_INT, VALUE_FLOAT)
    lib().gunrock_pr_func(C.byref(gout), ids.ctypes.data_as(C.c_void_p), ranks.ctypes.data_as(C.c_void_p), C.byref(gin), cfg, dt)
    return ids[:count], ranks[:count]


def gunrock_topk(nodes, row_offsets, col_indices, col_offsets, row_indices, top_nodes, device=0):
    """Call gunrock_topk_func as reference shared_lib_tests/test_topk.c does; returns (node_ids, in_degrees, out_degrees)."""
    ro, ci = _csr_arrays(row_offsets, col_indices)
    co = _i32(col_offsets)
    ri = _i32(row_indices)
    gin = _graph_struct(nodes, ro, ci)
    gin.col_offsets, gin.row_indices = co.ctypes.data, ri.ctypes.data
    gout = GunrockGraph()
    cfg = GunrockConfig()
    cfg.device, cfg.top_nodes = device, top_nodes
    k = max(min(nodes, top_nodes), 1)
    ids, ind, outd = (np.empty(k, dtype=np.int32) for _ in range(3))
    dt = GunrockDataType(VTXID_INT, SIZET_INT, VALUE_INT)
    lib().gunrock_topk_func(C.byref(gout), ids.ctypes.data_as(C.c_void_p), ind.ctypes.data_as(C.c_void_p), outd.ctypes.data_as(C.c_void_p),
                            C.byref(gin), cfg, dt)
    k = min(nodes, top_nodes)
    return ids[:k], ind[:k], outd[:k]


class PrProblem(_Problem):
    """PRProblem + PREnactor behind the handle ABI (grx_pr_*).  reset and enact are timed by the benchmark and name their symbols
    directly; device_results: (ranks, node ids)."""

    _family, _problem, _enactor = "pr", "PRProblem", "PREnactor"
    _check_rows = False
    _stats = (("iterations", "peeling_rounds", "surviving_nodes"), ())
    _results = 2

    def __init__(self, device=0):
        self._create("grx_pr_create", device)
        self.nodes = self.edges = 0

    def set_inverse_graph(self, d_inv_row_offsets=None, d_inv_col_indices=None, build=False):
        """No arguments: the graph is symmetric (its CSR is its own inverse); build=True: transpose on the device."""
        _check(lib().grx_pr_set_inverse_graph(self._h, C.c_void_p(d_inv_row_offsets), C.c_void_p(d_inv_col_indices), int(bool(build))),
               "PRProblem::SetInverseGraph")
        return self

    def reset(self, src=-1, delta=0.85, threshold=0.01):
        _check(lib().grx_pr_reset(self._h, int(src), float(delta), float(threshold)), "PRProblem::Reset")
        return self

    def enact(self, max_iter=20, max_grid_size=0):
        return self._timed(lib().grx_pr_enact, "PREnactor::Enact", int(max_iter), int(max_grid_size))

    def extract(self, count=-1):
        k = self.nodes if count < 0 else min(count, self.nodes)
        ranks, ids = _out(k, np.float32), _out(k)
        _check(lib().grx_pr_extract(self._h, _f32p(ranks), _p(ids), k), "PRProblem::Extract")
        return ids[:k], ranks[:k]


BC_OVERFLOW = -6  # enum GRX_BC_OVERFLOW (gunrock_mi355x.h)


class BcOverflow(ArithmeticError):
    """BcProblem.run: a source's shortest-path counts do not fit float32 (GRX_BC_OVERFLOW); bc_values are all 0 and the handle takes
    the next run"""


class BcProblem(_Handle):
    """BCProblem + BCEnactor behind the handle ABI (grx_bc_*): Init, one run() in place of Reset + Enact, Extract, with untyped
    array arguments -- none of the phases _Problem carries, so the class is written out."""

    _destroy = "grx_bc_destroy"

    def __init__(self, device=0):
        self._create("grx_bc_create", device)
        self.nodes = self.edges = 0
        self._keep = None

    def init(self, nodes, row_offsets, col_indices):
        ro, ci = _csr_arrays(row_offsets, col_indices)
        self.nodes, self.edges = int(nodes), int(ci.shape[0])
        _check(lib().grx_bc_init(self._h, self.nodes, self.edges, ro.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p)),
               "BCProblem::Init")
        return self

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices):
        self.nodes, self.edges = int(nodes), int(edges)
        _check(lib().grx_bc_init_device(self._h, self.nodes, self.edges, C.c_void_p(d_row_offsets), C.c_void_p(d_col_indices)),
               "BCProblem::Init(device)")
        return self

    def run(self, src=-1, max_grid_size=0, queue_sizing=1.0):
        """one source, or every vertex in turn (src = -1); returns the elapsed milliseconds.  BcOverflow when a path count leaves
        float32."""
        ms = C.c_float()
        rc = lib().grx_bc_run(self._h, int(src), max_grid_size, float(queue_sizing), C.byref(ms))
        if rc == BC_OVERFLOW:
            raise BcOverflow("gunrockinst_amd: BCEnactor::Enact: more than 2^126 shortest paths to a vertex (code %d)" % rc)
        _check(rc, "BCEnactor::Enact")
        return float(ms.value)

    def extract(self):
        sig, bc = _out(self.nodes, np.float32), _out(self.nodes, np.float32)
        _check(lib().grx_bc_extract(self._h, sig.ctypes.data_as(C.c_void_p), bc.ctypes.data_as(C.c_void_p), None), "BCProblem::Extract")
        return sig[:self.nodes], bc[:self.nodes]


def filter_queue(ids, row_offsets=None, capacity=None, max_grid_size=0):
    """oprtr::filter::Kernel with the BFS functor over a queue of vertex ids (-1 = culled entry), on the GPU.
    row_offsets given: returns (v, row_start, scan, edges) -- a complete vertex frontier, zero-degree vertices dropped;
    else (v,).  Output order is unspecified."""
    import numpy as np
    import torch
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    n = int(ids.shape[0])
    cap = int(capacity if capacity is not None else max(n, 1))
    d_in = torch.from_numpy(ids).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_v = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda")
    out_len, out_edges = C.c_int(), C.c_longlong()
    if row_offsets is None:
        _check(lib().grx_filter_queue(n, C.c_void_p(d_in.data_ptr()), None, cap, C.c_void_p(d_v.data_ptr()), None, None, C.byref(out_len),
                                      C.byref(out_edges), int(max_grid_size)), "filter::Kernel")
        return (d_v[:out_len.value].cpu().numpy(),)
    d_ro = torch.from_numpy(np.ascontiguousarray(row_offsets, dtype=np.int32)).cuda()
    d_rs = torch.empty_like(d_v)
    d_sc = torch.empty_like(d_v)
    _check(lib().grx_filter_queue(n, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_ro.data_ptr()), cap, C.c_void_p(d_v.data_ptr()),
                                  C.c_void_p(d_rs.data_ptr()), C.c_void_p(d_sc.data_ptr()), C.byref(out_len), C.byref(out_edges),
                                  int(max_grid_size)), "filter::Kernel")
    k = out_len.value
    return d_v[:k].cpu().numpy(), d_rs[:k].cpu().numpy(), d_sc[:k].cpu().numpy(), int(out_edges.value)


ADVANCE_MODES = {"ids": 0, "frontier": 1, "count": 2}
ADVANCE_RULES = {"mask": 0, "claim": 1}
ADVANCE_FUNCTORS = {"plain": 0, "hooked": 1}
REDUCE_TYPES = {"vertex": 1, "edge": 2}
REDUCE_OPS = {"plus": 1, "minus": 2, "multiplies": 3, "modulus": 4, "bit_or": 5, "bit_and": 6, "bit_xor": 7, "maximum": 8, "minimum": 9}
REDUCE_VALUE_TYPES = {"int32": 0, "uint32": 1, "float32": 2, "int64": 3, "uint64": 4}


def advance_frontier(row_offsets, vertices):
    """The input frontier of an advance as the operator consumes it: (v, row_start, scan, in_edges), scan = the exclusive
    prefix of the degrees in the given order.  A vertex without out-edges is outside the operator's contract: ValueError."""
    ro = np.asarray(row_offsets, dtype=np.int64)
    v = np.ascontiguousarray(vertices, dtype=np.int32).reshape(-1)
    if v.size and (v.min() < 0 or v.max() >= ro.size - 1):
        raise ValueError("advance_frontier: vertex id out of range")
    deg = ro[v.astype(np.int64) + 1] - ro[v]
    if (deg <= 0).any():
        raise ValueError("advance_frontier: vertex %d has no out-edges; an advance frontier never holds one" % int(v[np.argmax(deg <= 0)]))
    total = int(deg.sum())
    if total >= 2 ** 31:
        raise ValueError("advance_frontier: %d edge slots do not fit the operator's 32-bit SizeT" % total)
    scan = np.zeros(v.size, dtype=np.int64)
    np.cumsum(deg[:-1], out=scan[1:])
    return v, ro[v].astype(np.int32), scan.astype(np.int32), total


def _dev_i32(torch, a):
    a = np.array(a, dtype=np.int32, order="C")            # (a copy: the caller's array may be read-only)
    return torch.from_numpy(a).cuda() if a.size else torch.zeros(1, dtype=torch.int32, device="cuda")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def advance_queue(row_offsets, col_indices, vertices, mode="ids", rule="mask", functor="plain", mask=None, labels=None, depth=0,
                  record=True, capacity=None, max_grid_size=0):
    """advance::LaunchKernel over the frontier `vertices` (grx_advance_queue), on the GPU.  Returns a dict: `out_len`,
    `out_edges`, the output arrays `v` (+ `row_start`, `scan` in mode "frontier") cut to out_len, `buffers` = the whole output
    allocations (pre-filled with -7), `edge_hits` / `edge_src` (record=True; edge_src starts as -1) and `labels` (rule
    "claim").  Queue overflow raises RuntimeError."""
    import torch
    ro, ci = _csr_arrays(row_offsets, col_indices)
    v, rs, sc, in_edges = advance_frontier(ro, vertices)
    cap = int(capacity if capacity is not None else max(in_edges, 1))
    d_ro, d_ci, d_v, d_rs, d_sc = (_dev_i32(torch, a) for a in (ro, ci, v, rs, sc))
    d_mask = _dev_i32(torch, mask) if mask is not None else None
    d_labels = _dev_i32(torch, labels) if labels is not None else None
    d_hits = torch.zeros(max(ci.size, 1), dtype=torch.int32, device="cuda") if record else None
    d_src = torch.full((max(ci.size, 1),), -1, dtype=torch.int32, device="cuda") if record else None
    outs = [torch.full((max(cap, 1),), -7, dtype=torch.int32, device="cuda") for _ in range(3 if mode == "frontier" else 1)]
    out_len, out_edges = C.c_int(), C.c_longlong()
    torch.cuda.synchronize()
    _check(lib().grx_advance_queue(_ptr(d_ro), _ptr(d_ci), _ptr(d_v), _ptr(d_rs), _ptr(d_sc), int(v.size), in_edges, ADVANCE_MODES[mode],
                                   ADVANCE_RULES[rule], ADVANCE_FUNCTORS[functor], _ptr(d_mask), _ptr(d_labels), int(depth),
                                   _ptr(d_hits), _ptr(d_src), cap, _ptr(outs[0]), _ptr(outs[1]) if len(outs) > 1 else None,
                                   _ptr(outs[2]) if len(outs) > 1 else None, C.byref(out_len), C.byref(out_edges),
                                   int(max_grid_size)), "advance::LaunchKernel")
    k = out_len.value
    res = {"out_len": k, "out_edges": int(out_edges.value), "buffers": [t.cpu().numpy() for t in outs]}
    if mode != "count":
        for name, buf in zip(("v", "row_start", "scan"), res["buffers"]):
            res[name] = buf[:k]
    if record:
        res["edge_hits"] = d_hits[:ci.size].cpu().numpy()
        res["edge_src"] = d_src[:ci.size].cpu().numpy()
    if labels is not None:
        res["labels"] = d_labels.cpu().numpy()[:np.asarray(labels).size]
    return res


def advance_reduce(row_offsets, col_indices, vertices, values, r_type="vertex", op="plus", by_vertex=False, prefill=True, out=None,
                   out_len=None, mask=None, functor="plain", record=False, max_grid_size=0):
    """advance::LaunchReduce over the frontier `vertices` (grx_advance_reduce), on the GPU.  `values` (int32, uint32, float32,
    int64 or uint64; per vertex for r_type "vertex", per edge for "edge") picks the value type.  `out` = initial contents of
    the result array (default: zeros, one entry per vertex with by_vertex, else per frontier entry); `out_len` = entries the
    operator pre-sets to the identity when prefill (default: all of them).  Returns a dict: `reduced` (+ `edge_hits`,
    `edge_src` with record=True).  A combination the library does not instantiate raises RuntimeError."""
    import torch
    ro, ci = _csr_arrays(row_offsets, col_indices)
    v, rs, sc, in_edges = advance_frontier(ro, vertices)
    values = np.ascontiguousarray(values)
    vt = REDUCE_VALUE_TYPES[values.dtype.name]
    carrier = np.int32 if values.dtype.itemsize == 4 else np.int64        # bit patterns travel as signed words
    if values.size < (ci.size if r_type == "edge" else ro.size - 1):
        raise ValueError("advance_reduce: too few values")
    n_out = (ro.size - 1) if by_vertex else v.size
    if out is None:
        out = np.zeros(max(n_out, 1), dtype=values.dtype)
    out = np.ascontiguousarray(out, dtype=values.dtype)
    if out.size < n_out:
        raise ValueError("advance_reduce: result array too short")
    if out_len is None:
        out_len = out.size
    if out_len > out.size:
        raise ValueError("advance_reduce: out_len beyond the result array")
    d_ro, d_ci, d_v, d_rs, d_sc = (_dev_i32(torch, a) for a in (ro, ci, v, rs, sc))
    d_val = torch.from_numpy(values.view(carrier).copy()).cuda() if values.size else torch.zeros(1, dtype=torch.int64, device="cuda")
    d_out = torch.from_numpy(out.view(carrier).copy()).cuda() if out.size else torch.zeros(1, dtype=torch.int64, device="cuda")
    d_mask = _dev_i32(torch, mask) if mask is not None else None
    d_hits = torch.zeros(max(ci.size, 1), dtype=torch.int32, device="cuda") if record else None
    d_src = torch.full((max(ci.size, 1),), -1, dtype=torch.int32, device="cuda") if record else None
    torch.cuda.synchronize()
    _check(lib().grx_advance_reduce(_ptr(d_ro), _ptr(d_ci), _ptr(d_v), _ptr(d_rs), _ptr(d_sc), int(v.size), in_edges, REDUCE_TYPES[r_type],
                                    REDUCE_OPS[op], vt, int(bool(by_vertex)), int(bool(prefill)), int(out_len), _ptr(d_val), _ptr(d_out),
                                    ADVANCE_FUNCTORS[functor], _ptr(d_mask), _ptr(d_hits), _ptr(d_src), int(max_grid_size)),
           "advance::LaunchReduce")
    res = {"reduced": d_out.cpu().numpy().view(values.dtype)[:out.size]}
    if record:
        res["edge_hits"] = d_hits[:ci.size].cpu().numpy()
        res["edge_src"] = d_src[:ci.size].cpu().numpy()
    return res


SCAN_OUT_TYPES = {"int32": 0, "uint32": 1, "uint64": 2}
WAVE_OPS = {"inclusive_sum": 0, "inclusive_sum_dpp": 1, "inclusive_max_dpp": 2, "segmented_scan_dpp": 3, "wave_sum": 4,
            "rank_in_mask": 5, "block_scan": 6, "dpp_move": 7}
DPP_MOVE_IDENTITY = 0xA5A5A5A55A5A5A5A
_CARRIER = {1: "uint8", 4: "int32", 8: "int64"}


def _dev(torch, a, dtype=None):
    """a device copy of a numpy array of any 1-, 4- or 8-byte type (bit patterns travel as signed words); never of size 0"""
    a = np.array(a, dtype=dtype, order="C").reshape(-1)
    carrier = np.dtype(_CARRIER[a.dtype.itemsize])
    return torch.from_numpy(a.view(carrier)).cuda() if a.size else torch.zeros(1, dtype=getattr(torch, carrier.name), device="cuda")


def _host(t, dtype, n):
    return t.cpu().numpy().view(dtype)[:n]


def device_scan(values, out_type="uint64"):
    """graphio::DeviceExclusiveScan<out_type> of uint32 `values` (grx_device_scan), on the GPU: (prefix as out_type, 64-bit total)"""
    import torch
    values = np.ascontiguousarray(values, dtype=np.uint32)
    n = int(values.size)
    out_dtype = np.dtype(out_type)
    d_in = _dev(torch, values)
    d_out = torch.zeros(max(n, 1), dtype=torch.int64 if out_dtype.itemsize == 8 else torch.int32, device="cuda")
    total = C.c_ulonglong()
    torch.cuda.synchronize()
    _check(lib().grx_device_scan(_ptr(d_in), n, SCAN_OUT_TYPES[out_dtype.name], _ptr(d_out), C.byref(total)), "DeviceExclusiveScan")
    return _host(d_out, out_dtype, n), int(total.value)


def device_key_sort(key_arrays, key_bits):
    """ONE graphio::DeviceKeySort sorts the uint64 arrays of `key_arrays` one after the other, array a on its low key_bits[a]
    bits (grx_device_key_sort), on the GPU.  Returns the list of sorted arrays."""
    import torch
    arrays = [np.ascontiguousarray(k, dtype=np.uint64).reshape(-1) for k in key_arrays]
    bits = np.ascontiguousarray(key_bits, dtype=np.int32).reshape(-1)
    if bits.size != len(arrays):
        raise ValueError("device_key_sort: one key_bits per array")
    counts = np.array([a.size for a in arrays], dtype=np.int64)
    total = int(counts.sum())
    d_in = _dev(torch, np.concatenate(arrays) if arrays else np.zeros(0, dtype=np.uint64))
    d_out = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _check(lib().grx_device_key_sort(len(arrays), _i64p(counts), _p(bits), _ptr(d_in), _ptr(d_out)), "DeviceKeySort")
    out = _host(d_out, np.uint64, total)
    ends = np.cumsum(counts)
    return [out[int(e - c):int(e)] for c, e in zip(counts, ends)]


def device_transpose(row_offsets, col_indices, values=None):
    """graphio::DeviceTransposeCsr (grx_device_transpose), on the GPU: (inv_row_offsets, inv_col_indices[, inv_values]);
    `values` = one uint32 per edge that travels with it."""
    import torch
    ro, ci = _csr_arrays(row_offsets, col_indices)
    nodes, edges = int(ro.size - 1), int(ci.size)
    d_ro, d_ci = _dev_i32(torch, ro), _dev_i32(torch, ci)
    d_vals = d_ivals = None
    if values is not None:
        values = np.ascontiguousarray(values, dtype=np.uint32)
        if values.size != edges:
            raise ValueError("device_transpose: one value per edge")
        d_vals = _dev(torch, values)
        d_ivals = torch.full((max(edges, 1),), -7, dtype=torch.int32, device="cuda")
    d_iro = torch.full((nodes + 1,), -7, dtype=torch.int32, device="cuda")
    d_ici = torch.full((max(edges, 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _check(lib().grx_device_transpose(nodes, edges, _ptr(d_ro), _ptr(d_ci), _ptr(d_vals), _ptr(d_iro), _ptr(d_ici), _ptr(d_ivals)),
           "DeviceTransposeCsr")
    res = (d_iro.cpu().numpy(), d_ici.cpu().numpy()[:edges])
    return res if values is None else res + (_host(d_ivals, np.uint32, edges),)


def wave_ops(op, values, threads=256, r_op=None, heads=None, step=0):
    """One building block of util/device_intrinsics.hpp per element of `values` (grx_wave_ops), on the GPU: element i is lane
    i % 64 of a workgroup of `threads` threads.  `values`' dtype picks the value type; r_op (a REDUCE_OPS name) and `heads`
    belong to "segmented_scan_dpp", `step` (0..5) to "dpp_move".  Returns the result array; for "block_scan" the tuple
    (first result, first total, second result, second total), the second scan over the workgroup's elements in mirrored order.
    A combination the library does not instantiate raises RuntimeError."""
    import torch
    values = np.ascontiguousarray(values).reshape(-1)
    n = int(values.size)
    vt = REDUCE_VALUE_TYPES[values.dtype.name]
    out_dtype = np.dtype(np.uint32) if op == "rank_in_mask" else values.dtype
    d_in = _dev(torch, values)
    d_out = _dev(torch, np.zeros(max(n, 1), dtype=out_dtype))
    d_heads = _dev(torch, np.asarray(heads) != 0, dtype=np.uint8) if heads is not None else None
    if heads is not None and np.asarray(heads).size != n:
        raise ValueError("wave_ops: one head flag per value")
    d_aux = _dev(torch, np.zeros(max(3 * n, 1), dtype=values.dtype)) if op == "block_scan" else None
    second = REDUCE_OPS[r_op] if op == "segmented_scan_dpp" else int(step)
    torch.cuda.synchronize()
    _check(lib().grx_wave_ops(WAVE_OPS[op], second, vt, int(threads), n, _ptr(d_in), _ptr(d_heads), _ptr(d_out), _ptr(d_aux)),
           "wave block %s" % op)
    out = _host(d_out, out_dtype, n)
    if op != "block_scan":
        return out
    aux = _host(d_aux, values.dtype, 3 * n)
    return out, aux[:n], aux[n:2 * n], aux[2 * n:]


def bisect_queue(row_offsets, dist, visit_lookup, delta, queue, level, tag, parked=None, count_on_device=None, near_capacity=None,
                 far_capacity=None, mark_paths=False, guard=64, max_grid_size=0):
    """priority_queue::Bisect with the SSSP enactor's template arguments over `queue` (grx_bisect_queue), on the GPU.
    dist: uint32 distance per vertex; visit_lookup: int32 tag per vertex (returned updated); parked: the distance every queue
    entry was parked with, or None; count_on_device: the element count that goes through the packed device tail (the queue's
    length is then the loose upper bound), or None to pass the length by value.  Every output array is allocated `guard`
    entries longer than its capacity and pre-filled with -7.  Returns a dict: `near_len`, `near_edges`, `far_len` (the tails),
    `far_min`, `overflow`, the whole `near_v` / `near_row_start` / `near_scan` / `far_v` / `far_d` allocations, `visit_lookup`."""
    import torch
    ro = np.ascontiguousarray(row_offsets, dtype=np.int32)
    queue = np.ascontiguousarray(queue, dtype=np.int32).reshape(-1)
    n = int(queue.size)
    near_cap = int(near_capacity if near_capacity is not None else max(n, 1))
    far_cap = int(far_capacity if far_capacity is not None else max(n, 1))
    dist = np.ascontiguousarray(dist, dtype=np.uint32)
    d_ro, d_in = _dev_i32(torch, ro), _dev_i32(torch, queue)
    d_dist = _dev(torch, (dist.astype(np.uint64) << np.uint64(32)) | np.arange(dist.size, dtype=np.uint64)) if mark_paths else _dev(torch, dist)
    d_lookup = _dev_i32(torch, visit_lookup)
    d_parked = _dev(torch, parked, dtype=np.uint32) if parked is not None else None
    if parked is not None and np.asarray(parked).size != n:
        raise ValueError("bisect_queue: one parked distance per queue entry")
    d_count = None
    if count_on_device is not None:
        if not 0 <= int(count_on_device) <= n:
            raise ValueError("bisect_queue: the device count exceeds the queue")
        d_count = _dev(torch, np.array([int(count_on_device) | (12345 << 32)], dtype=np.uint64))   # (the edge half is not the count)
    near = [torch.full((near_cap + guard,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    far = [torch.full((far_cap + guard,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    near_tail, far_tail, far_min, overflow = C.c_ulonglong(), C.c_ulonglong(), C.c_uint32(), C.c_int()
    torch.cuda.synchronize()
    _check(lib().grx_bisect_queue(_ptr(d_ro), _ptr(d_dist), int(bool(mark_paths)), _ptr(d_lookup), float(delta), _ptr(d_in), _ptr(d_parked),
                                  n, _ptr(d_count), int(level), int(tag), near_cap, _ptr(near[0]), _ptr(near[1]), _ptr(near[2]), far_cap,
                                  _ptr(far[0]), _ptr(far[1]), C.byref(near_tail), C.byref(far_tail), C.byref(far_min), C.byref(overflow),
                                  int(max_grid_size)), "priority_queue::Bisect")
    return {"near_len": int(near_tail.value & 0xFFFFFFFF), "near_edges": int(near_tail.value >> 32), "far_len": int(far_tail.value),
            "far_min": int(far_min.value), "overflow": int(overflow.value), "near_v": near[0].cpu().numpy(),
            "near_row_start": near[1].cpu().numpy(), "near_scan": near[2].cpu().numpy(), "far_v": far[0].cpu().numpy(),
            "far_d": far[1].cpu().numpy().view(np.uint32), "visit_lookup": d_lookup.cpu().numpy()[:np.asarray(visit_lookup).size]}


class SsspProblem(_Handle):
    """SSSPProblem + SSSPEnactor behind the handle C ABI.  Every phase has arguments of its own (uint32 weights, delta, the source)
    and the family has no device_results, so the class is written out on _Handle."""

    _destroy = "grx_sssp_destroy"

    def __init__(self, mark_pred=False, instrument=False, device=0):
        self.mark_pred = bool(mark_pred)
        self._create("grx_sssp_create", int(mark_pred), int(instrument), device)
        self.nodes = 0

    def init(self, nodes, row_offsets, col_indices, weights, delta_factor=16):
        ro, ci = _csr_arrays(row_offsets, col_indices)
        w = np.ascontiguousarray(weights, dtype=np.uint32)
        self.nodes = int(nodes)
        _check(lib().grx_sssp_init(self._h, nodes, ci.shape[0], _p(ro), _p(ci), _u32p(w),
                                   delta_factor), "SSSPProblem::Init")
        return self

    def init_device(self, nodes, edges, d_row_offsets, d_col_indices, d_weights, delta):
        self.nodes = int(nodes)
        _check(lib().grx_sssp_init_device(self._h, nodes, edges, C.c_void_p(d_row_offsets), C.c_void_p(d_col_indices),
                                          C.c_void_p(d_weights), float(delta)), "SSSPProblem::Init(device)")
        return self

    def set_inverse_graph(self, d_inv_row_offsets=None, d_inv_col_indices=None, d_inv_weights=None, pull_min_edges=-1):
        """Enable pull relaxation of dense levels; no arrays = build the weighted transpose on the device."""
        _check(lib().grx_sssp_set_inverse_graph(self._h, C.c_void_p(d_inv_row_offsets), C.c_void_p(d_inv_col_indices),
                                                C.c_void_p(d_inv_weights), int(pull_min_edges)), "SSSPProblem::SetInverseGraph")
        return self

    def pull_levels(self):
        n = C.c_longlong()
        _check(lib().grx_sssp_pull_levels(self._h, C.byref(n)), "grx_sssp_pull_levels")
        return int(n.value)

    def reset(self, src, queue_sizing=1.0):
        _check(lib().grx_sssp_reset(self._h, int(src), float(queue_sizing)), "SSSPProblem::Reset")

    def enact(self, src, max_grid_size=0):
        return self._timed(lib().grx_sssp_enact, "SSSPEnactor::Enact", int(src), max_grid_size)

    def stats(self):
        v, e, it, l = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong()
        k, d = C.c_double(), C.c_float()
        _check(lib().grx_sssp_stats(self._h, C.byref(v), C.byref(e), C.byref(it), C.byref(l), C.byref(k), C.byref(d)),
               "grx_sssp_stats")
        return {"relaxed_vertices": v.value, "relaxed_edges": e.value, "iterations": it.value,
                "kernel_launches": l.value, "kernel_ms": k.value, "delta": d.value}

    def extract(self):
        dist, preds = _out(self.nodes, np.uint32), _out(self.nodes, wanted=self.mark_pred)
        _check(lib().grx_sssp_extract(self._h, _u32p(dist), _opt(preds)), "SSSPProblem::Extract")
        return dist[:self.nodes], _cut(preds, self.nodes)


def gunrock_sssp(nodes, row_offsets, col_indices, weights, src=0, mark_pred=True, delta_factor=16, queue_size=1.0,
                 src_mode=SRC_MANUALLY, device=0):
    """Call gunrock_sssp_func as reference shared_lib_tests/test_sssp.c does; returns (distances, predecessors)."""
    ro, ci = _csr_arrays(row_offsets, col_indices)
    w = np.ascontiguousarray(weights, dtype=np.uint32)
    gin = _graph_struct(nodes, ro, ci, w)
    gout = GunrockGraph()
    cfg = GunrockConfig()
    cfg.mark_pred, cfg.src_node, cfg.device = mark_pred, src, device
    cfg.delta_factor, cfg.queue_size, cfg.src_mode = delta_factor, queue_size, src_mode
    preds = _out(nodes)
    dt = GunrockDataType(VTXID_INT, SIZET_INT, VALUE_UINT)
    lib().gunrock_sssp_func(C.byref(gout), preds.ctypes.data_as(C.c_void_p), C.byref(gin), cfg, dt)
    return _take_node_values(gout, nodes, np.uint32), preds[:nodes]
