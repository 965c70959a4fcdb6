/*
 * gunrock/gunrock_mi355x.h -- handle-based C ABI over the engine's Problem / Enactor classes.
 *
 * gunrock.h's one-shot calls (upload, run, download, free) hide the phases the reference's own
 * drivers time separately (tests/bfs/test_bfs.cu:385-445: Init once, then Reset + timed Enact per
 * run, Extract, validate).  This header exposes those phases -- and the host graph builders the
 * drivers use -- as plain C entry points with plain pointers and sizes, so a foreign-language host
 * (ctypes / cgo / JNI) can keep a graph resident in HBM across runs.  Every function cites the
 * reference C++ interface it stands for.
 *
 * All functions return 0 on success, a positive hipError_t value on a HIP failure (already printed
 * to stderr in the reference's GRError format) or a negative value for a host-side error.
 * "d_" pointers are device (HBM) addresses; everything else is host memory.
 */
#ifndef GUNROCK_GUNROCK_MI355X_H_
#define GUNROCK_GUNROCK_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Host graphs: gunrock::Csr<int,int,int> (reference gunrock/csr.cuh:38-80)
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_graph grx_graph;

/* graphio::BuildMarketGraph<true>(file, csr, undirected, reversed)  (reference graphio/market.cuh:296-339) */
int grx_graph_from_market(const char *path, int undirected, int reversed, grx_graph **out);
/* The same with the reference's CSR cache rule (market.cuh:296-339, csr.cuh:140-232: "<dir>/.<name>_{undirected,reversed,
 * nonreversed}_csr" written after the first parse and preferred afterwards), made safe: the cache is BINARY ("....bin"), and
 * is used only when it was written for a source file of exactly this size and modification time; *cache_hit (may be NULL)
 * tells which way the graph came.  An unwritable directory is not an error. */
int grx_graph_from_market_cached(const char *path, int undirected, int reversed, int *cache_hit, grx_graph **out);
/* graphio::BuildRmatGraph<true>(nodes, edges, csr, undirected, a,b,c,d) on libc rand() (reference graphio/rmat.cuh:27-91) */
int grx_graph_rmat_libc(int nodes, int edges, int undirected, double a, double b, double c, double d, grx_graph **out);
/* seeded counter-based R-MAT: 2^scale vertices, `pairs` generated edges (mirrored when undirected) */
int grx_graph_rmat_seeded(int scale, long long pairs, uint64_t seed, int undirected,
                          double a, double b, double c, double d, grx_graph **out);
/* Csr::FromCoo<true>(coo, nodes, tuples)  (reference csr.cuh:247-340): stable sort, drop self loops + repeats */
int grx_graph_from_coo(int nodes, long long tuples, const int *rows, const int *cols, const int *vals, grx_graph **out);
/* wrap existing CSR arrays (copied) -- what bfs_app.cu:256-260 does with the caller's pointers */
int grx_graph_from_csr(int nodes, int edges, const int *row_offsets, const int *col_indices, const int *edge_values,
                       grx_graph **out);
int grx_graph_nodes(const grx_graph *g);
int grx_graph_edges(const grx_graph *g);
const int *grx_graph_row_offsets(const grx_graph *g);
const int *grx_graph_col_indices(const grx_graph *g);
const int *grx_graph_edge_values(const grx_graph *g);   /* NULL when the graph carries no values */
/* Csr::GetNodeWithHighestDegree (reference csr.cuh:442-455) / GetAverageDegree (csr.cuh:475-485) */
int grx_graph_highest_degree_node(grx_graph *g, int *max_degree);
int grx_graph_average_degree(grx_graph *g);
/* graphio::RandomNode (reference graphio/utils.cuh:38-45) */
int grx_random_node(int num_nodes);
void grx_graph_free(grx_graph *g);

/* Device-side seeded R-MAT tuple generation (same stream as grx_graph_rmat_seeded): writes `count` tuples
 * starting at generated-edge index `first` into d_rows / d_cols.  `stream` is a hipStream_t or NULL. */
int grx_rmat_seeded_device(int scale, long long first, long long count, uint64_t seed,
                           double a, double b, double c, double d, int *d_rows, int *d_cols, void *stream);

/* Device-side COO -> CSR with Csr::FromCoo's graph semantics (reference csr.cuh:247-340: stable sort by (row, col), self
 * loops and duplicates dropped, trailing empty rows kept; `undirected` mirrors every tuple first, as the reference's
 * loaders do, market.cuh:172-183).  Hand-written LSD radix sort + device-wide scan, all in HBM.
 *   sort : d_rows / d_cols = `pairs` tuples on the device; rows = CSR rows to produce, nodes = vertex id space.
 *          parts > 1 builds one rank's slice of a vertex-cut partition: only tuples whose source v has v mod parts == rank
 *          are kept and stored under local row v div parts (ownership rule of reference problem_base.cuh:185-210).
 *          Returns the number of CSR edges in *edges_out so the caller can allocate.
 *   emit : writes row_offsets[rows + 1] and col_indices[edges] into caller-owned device arrays.
 * Tuples must stay below 2^31 (SIZET_INT).  `stream` is a hipStream_t or NULL. */
typedef struct grx_coo2csr grx_coo2csr;
int grx_coo_to_csr_sort(grx_coo2csr **handle, int rows, int nodes, long long pairs, const int *d_rows, const int *d_cols,
                        int undirected, int parts, int rank, long long *edges_out, void *stream);
int grx_coo_to_csr_emit(grx_coo2csr *handle, int *d_row_offsets, int *d_col_indices, void *stream);
void grx_coo_to_csr_free(grx_coo2csr *handle);

/* ------------------------------------------------------------------------------------------------
 * BFS: BFSProblem + BFSEnactor (reference gunrock/app/bfs/bfs_problem.cuh:41-364, bfs_enactor.cuh:40-708)
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_bfs grx_bfs;

/* picks the <MARK_PREDECESSORS, ENABLE_IDEMPOTENCE> instantiation like dispatch_bfs (reference bfs_app.cu:299-348);
 * `instrument` selects BFSEnactor<true>: per-launch HIP-event timing of the operator kernels */
int grx_bfs_create(grx_bfs **out, int mark_pred, int idempotence, int instrument, int device);
/* BFSProblem::Init(false, csr, 1) (reference bfs_problem.cuh:188-261): uploads the CSR */
int grx_bfs_init(grx_bfs *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* same, for a CSR that already lives in HBM (pointers are borrowed for the life of the handle) */
int grx_bfs_init_device(grx_bfs *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* Enable direction-optimizing traversal (reference app/dobfs: DOBFSProblem::Init takes the graph AND its inverse,
 * dobfs_problem.cuh; alpha/beta as in tests/dobfs/test_dobfs.cu:530-534).  d_inv_* is the in-neighbour CSR in HBM
 * (borrowed); pass NULL, NULL when the graph is undirected/symmetric to reuse the forward arrays.  alpha/beta <= 0
 * keep the defaults.  Takes effect with traversal_mode = 2 in grx_bfs_enact.  Call after init. */
int grx_bfs_set_inverse_graph(grx_bfs *p, const int *d_inv_row_offsets, const int *d_inv_col_indices,
                              float alpha, float beta);
/* What gunrock_bfs_func does before its search: when the CSR is its own inverse (every edge mirrored; checked on the device)
 * the graph serves as its own in-neighbour lists; otherwise, with build_if_directed != 0, the transpose is built on the device and
 * owned by the handle (the reference's DOBFS driver builds the inverse graph on the host, tests/dobfs/test_dobfs.cu; its enactor
 * takes both, dobfs_enactor.cuh:397,569).  *enabled: traversal_mode 2 is available; *built: a transpose was built; *build_ms:
 * what that cost.  Any out pointer may be NULL.  Call after init. */
int grx_bfs_auto_inverse(grx_bfs *p, int build_if_directed, int *enabled, int *built, float *build_ms);
/* Enactor tuning knobs (the reference exposes alpha/beta on its DOBFS command line, tests/dobfs/test_dobfs.cu:530-534):
 * alpha, beta as above; lite_factor: a top-down level runs without queue output when frontier_edges*alpha*lite_factor
 * exceeds the unexplored edges (0 disables); tail_edge_limit: levels with at most this many edges run inside the
 * single-workgroup multi-level kernel (0 disables).  Non-positive alpha/beta and negative other values keep the current
 * setting.  Results do not depend on any of these. */
int grx_bfs_set_tuning(grx_bfs *p, float alpha, float beta, float lite_factor, int tail_edge_limit);
/* Top-down levels with more than tail_edge_limit and at most `edge_limit` edges run inside the persistent multi-workgroup
 * kernel (one resident workgroup per CU, grid barrier between levels; 0 disables).  This is what the reference's
 * traversal_mode 1 (TWC advance for low-degree, high-diameter graphs, tests/bfs/test_bfs.cu:563-566) is for. */
int grx_bfs_set_persistent_limit(grx_bfs *p, int edge_limit);
/* traversal_mode 1 / graphs of average degree <= 8: a top-down frontier of at most 4096 vertices and `edge_limit` edges (default
 * 8192; 0 = never) runs in the TWC workgroup -- thread / wave / workgroup tiers by neighbour-list length (reference
 * edge_map_forward/cta.cuh:224-545), frontier kept in LDS, level after level inside one launch -- until a level outgrows it. */
int grx_bfs_set_twc_limit(grx_bfs *p, int edge_limit);
/* Launch that kernel with hipLaunchCooperativeKernel (the runtime then refuses a grid that exceeds the occupancy query at
 * launch time; costs ~15-19 us of host time per launch).  Off by default: a plain launch of the same grid has the same
 * residency, and the grid barrier's timeout word reports a lost co-residency at run time either way. */
int grx_bfs_set_cooperative_launch(grx_bfs *p, int on);
/* Top-down levels with at least `min_edges` frontier edges run as a destination-binned advance: expand + status screen,
 * claims on the destination's owner XCD without atomics, then a vertex-ordered closing sweep that labels and enqueues
 * (0 = never; default 2^23).  This replaces the per-edge atomicCAS of the reference's functor (bfs_functor.cuh:56-58) on the
 * levels where it dominates.  Results do not depend on it. */
int grx_bfs_set_binned_min_edges(grx_bfs *p, long long min_edges);
/* Deferred labels of a direction-optimizing search (DESIGN.md 3.3 i): sweeps that find vertices in vertex order keep their
 * output bitmap and ONE pass at the end of Enact writes every label.  enabled: 1 / 0, -1 = leave; mask_limit: frontier
 * bitmaps a search may hold before it flushes the kept ones into the labels (4..12, 0 = leave; tests shrink it).  Takes
 * effect at the next grx_bfs_reset.  Labels are identical either way. */
int grx_bfs_set_label_deferral(grx_bfs *p, int enabled, int mask_limit);
/* Enactor tuning by name (returns 1 for an unknown name): "emit_queue_factor" (a compacting bottom-up sweep also writes its
 * finds as the next top-down queue when its input frontier is within this factor of the switch-back threshold),
 * "sparse_sweep_div", "speculative_emit" (1/0: the label pass is queued behind the closing top-down launch without waiting
 * for its read-back), "chain_sweeps" (bottom-up sweeps queued per host round trip), "label_pass" (1, the default: the closing
 * label pass loads every bitmap word once per workgroup tile; 0: the per-lane kernels it replaced; read at every launch of
 * the pass, so it can be flipped between searches), "walk_queue" (1, the default: the dense bottom-up sweep queues the row walks
 * of its pending vertices per wave and walks them 64 at a time, DESIGN.md 3.3 m; 0: the step-by-step walk loop it replaced; read
 * at every launch of a sweep), "fused_publish" (1, the default: where a tiled label pass is queued behind the launch that
 * usually ends the search, its workgroup 0 publishes the read-back that tells the host how the search ended, and Enact records
 * its completion event while the pass still runs, DESIGN.md 3.3 o; 0: a publishing kernel behind the pass; read at every Enact).
 * Relabelled copy (DESIGN.md 3.3 k): a symmetric problem (grx_bfs_set_inverse_graph without arrays, or grx_bfs_auto_inverse
 * on a symmetric graph) also builds a copy of its CSR renumbered hub-first, edgeless-last, and searches it; labels and
 * predecessors still come back in the caller's numbering.  "relabel" (1: search the copy; 0: the caller's numbering; -1, the
 * default: the copy on graphs of at least "relabel_min_nodes" vertices, default 2^23; effective at the next grx_bfs_reset, both
 * numberings are kept; returns 2 for 1 on a problem without a copy), "relabel_hubs" (most vertices in the hub tier, default
 * 65536, 0 = none; rebuilds the copy), "hub_slice" (DESIGN.md 3.3 n: the dense bottom-up sweeps answer probes of vertex ids
 * below this value from a copy of the frontier bitmap's first words in LDS; -1, the default: the size of the copy's hub tier
 * while a search runs on the copy, nothing in the caller's numbering; 0: off; capped at 131072 ids and at the bitmap's length;
 * read at every launch of a sweep).  Results never depend on any of them. */
int grx_bfs_set_option(grx_bfs *p, const char *name, double value);
/* The relabelled copy: hub-tier size, vertices with edges, the hub degree threshold, build time (ms) and the device bytes it
 * adds.  hubs = -1 when the problem has no copy. */
/* Deferred labels: how many times a search of this handle ran out of frontier bitmaps and flushed its kept levels into the
 * labels (summed over the handle's life; see grx_bfs_set_label_deferral's mask_limit). */
int grx_bfs_mask_flushes(grx_bfs *p, long long *flushes);
/* *idle = 1 when nothing is queued or running on the handle's stream (hipStreamQuery says hipSuccess), else 0.  grx_bfs_enact
 * returns only when everything it queued has completed, so right after it the answer is 1. */
int grx_bfs_stream_idle(grx_bfs *p, int *idle);
/* Read-backs that a label pass published on the enactor's behalf ("fused_publish"), summed over the handle's life. */
int grx_bfs_fused_publications(grx_bfs *p, long long *count);
int grx_bfs_relabel_info(grx_bfs *p, long long *hubs, long long *with_edges, int *threshold, float *build_ms, long long *bytes);
/* Direction-optimizing only: a level that would run count-only or bottom-up and has between `min_edges` and `max_edges`
 * frontier edges starts with a bottom-up pass that probes only the adjacency heads (the highest-degree in-neighbours); the
 * count-only top-down advance then handles what is left.  -1 = automatic bounds (edges/30 .. edges/7.8), min 0 = never,
 * max 0 = no upper bound.  Results do not depend on it. */
int grx_bfs_set_head_pass(grx_bfs *p, int min_edges, int max_edges);
/* BFSProblem::Reset(src, frontier_type, queue_sizing) (reference bfs_problem.cuh:272-360) */
int grx_bfs_reset(grx_bfs *p, int src, double queue_sizing);
/* BFSEnactor::Enact(context, problem, src, max_grid_size, traversal_mode) (reference bfs_enactor.cuh:573-579);
 * traversal_mode 0 = load-balanced top-down, 1 = low-degree/high-diameter choice of the reference driver (its TWC
 * advance; here LB advance + persistent mid-size levels kernel), 2 = direction-optimizing;
 * bracketed by HIP events on the problem's stream like the reference's GpuTimer (test_bfs.cu:408-438) */
int grx_bfs_enact(grx_bfs *p, int src, int max_grid_size, int traversal_mode, float *elapsed_ms);
/* BFSEnactor::GetStatistics (reference bfs_enactor.cuh:173-186) plus, when instrumented, operator-kernel
 * launch count and summed kernel time of the last Enact */
int grx_bfs_stats(grx_bfs *p, long long *total_queued, long long *search_depth, double *avg_duty,
                  long long *kernel_launches, double *kernel_ms);
/* instrumented enactors only: per-BSP-iteration record of the last Enact (input frontier length, its edge count,
 * operator kernel milliseconds, operator kind: 0 = top-down advance, 1 = bottom-up advance).  Fills up to
 * max_levels entries and returns the number of iterations recorded.  The `--v` per-iteration printout of the
 * reference driver (bfs_enactor.cuh:333-338) in data form. */
int grx_bfs_level_trace(grx_bfs *p, int max_levels, long long *frontier, long long *edges, double *ms, int *kind);
/* BFSProblem::Extract(h_labels, h_preds) (reference bfs_problem.cuh:144-177); h_preds may be NULL */
int grx_bfs_extract(grx_bfs *p, int *h_labels, int *h_preds);
/* device result arrays (valid until destroy / next init) */
int grx_bfs_device_results(grx_bfs *p, int **d_labels, int **d_preds);
void grx_bfs_destroy(grx_bfs *p);
/* The compacting filter operator by itself: reference filter::Kernel (gunrock/oprtr/filter/kernel.cuh:211-383) with the BFS
 * functor, whose CondFilter keeps valid vertex ids (bfs_functor.cuh:100-105).  d_in[n] in HBM, -1 = culled entry.
 * d_row_offsets != NULL: the output is a complete vertex frontier for the load-balanced advance -- id, first edge and the
 * exclusive prefix of the degrees in OUTPUT order; vertices without out-edges are dropped -- else ids only (row_start / scan
 * unused).  out_len entries were written (order unspecified), *out_edges = sum of their degrees.  Returns a HIP error code
 * ("Frontier queue overflow" when capacity is too small, filter/cta.cuh:526-529). */
int grx_filter_queue(int n, const int *d_in, const int *d_row_offsets, int capacity, int *d_out_v, int *d_out_row_start, int *d_out_scan,
                     int *out_len, long long *out_edges, int max_grid_size);

/* The advance operator by itself (reference advance::LaunchKernel, gunrock/oprtr/advance/kernel.cuh:101-129), with the library's
 * KernelPolicy<256, 4, 8, LB> and a small functor pair defined in lib/oprtr_app.hip.  All pointers are device pointers.
 * Graph: d_row_offsets / d_col_indices.  Input frontier as the operator consumes it: in_len entries of (vertex, first edge,
 * exclusive prefix of the degrees in queue order), in_edges = the sum of their degrees; every entry has at least one out-edge.
 * max_grid_size: workgroups at most, 0 = one resident grid. */
enum grx_advance_mode { GRX_ADVANCE_IDS = 0, GRX_ADVANCE_FRONTIER = 1, GRX_ADVANCE_COUNT_ONLY = 2 };
enum grx_advance_rule { GRX_ADVANCE_RULE_MASK = 0, GRX_ADVANCE_RULE_CLAIM = 1 };
/* PLAIN: CondEdge / ApplyEdge only; HOOKED: the same rule with ScreenEdge and IssueEdge / ResolveEdge (the operator's batch path) */
enum grx_advance_functor { GRX_ADVANCE_FUNCTOR_PLAIN = 0, GRX_ADVANCE_FUNCTOR_HOOKED = 1 };
/* values of advance::REDUCE_TYPE / advance::REDUCE_OP (reference advance/kernel_policy.cuh:58-79) */
enum grx_reduce_type { GRX_REDUCE_VERTEX = 1, GRX_REDUCE_EDGE = 2 };
enum grx_reduce_op {
    GRX_REDUCE_PLUS = 1, GRX_REDUCE_MINUS = 2, GRX_REDUCE_MULTIPLIES = 3, GRX_REDUCE_MODULUS = 4, GRX_REDUCE_BIT_OR = 5,
    GRX_REDUCE_BIT_AND = 6, GRX_REDUCE_BIT_XOR = 7, GRX_REDUCE_MAXIMUM = 8, GRX_REDUCE_MINIMUM = 9
};
enum grx_value_type { GRX_VALUE_INT = 0, GRX_VALUE_UINT = 1, GRX_VALUE_FLOAT = 2, GRX_VALUE_LONGLONG = 3, GRX_VALUE_ULONGLONG = 4 };
/* Plain advance.  rule MASK: an edge is accepted iff d_mask[destination] != 0 (d_mask == NULL: every edge; a destination reached
 * over several edges is enqueued once per edge); rule CLAIM: atomicCAS(&d_labels[destination], -1, depth) and the winner
 * accepts.  Every accepted edge e adds 1 to d_edge_hits[e] and stores its source vertex in d_edge_src[e] (either may be NULL).
 * mode IDS writes the accepted destinations to d_out_v; FRONTIER writes a complete frontier (as grx_filter_queue does,
 * destinations without out-edges dropped); COUNT_ONLY writes no output array.  *out_len = entries accepted (written),
 * *out_edges = the sum of their degrees (FRONTIER only, else 0); order unspecified.  Returns 0, a HIP error code ("Frontier
 * queue overflow" when `capacity` entries do not hold the output), or -1 for an argument that makes no sense. */
int grx_advance_queue(const int *d_row_offsets, const int *d_col_indices, const int *d_in_v, const int *d_in_row_start,
                      const int *d_in_scan, int in_len, int in_edges, int mode, int rule, int functor, const int *d_mask, int *d_labels,
                      int depth, int *d_edge_hits, int *d_edge_src, int capacity, int *d_out_v, int *d_out_row_start, int *d_out_scan,
                      int *out_len, long long *out_edges, int max_grid_size);
/* Reducing advance (advance::LaunchReduce) under rule MASK: d_reduced[i] = r_op over the accepted out-edges e = (v, u) of frontier
 * entry i of d_values[u] (VERTEX) or d_values[e] (EDGE); the operator's identity when no edge is accepted.  by_vertex: results
 * sit at d_reduced[v] and not at [i].  prefill: the first out_len entries of d_reduced (0 = in_len) are set to the identity
 * first; without it the caller has done that for the entries of this frontier and the others are left alone.  value_type
 * gives the element type of d_values and d_reduced.  Instantiated: PLUS, MULTIPLIES, MAXIMUM, MINIMUM for int, unsigned and
 * float; BIT_OR, BIT_AND, BIT_XOR for int and unsigned; PLUS, MAXIMUM, MINIMUM for long long and unsigned long long; each for
 * both reduce types and both by_vertex settings with the PLAIN functor (HOOKED: PLUS and MINIMUM of int and float, VERTEX by
 * position and EDGE by vertex).  Any other combination returns -2. */
int grx_advance_reduce(const int *d_row_offsets, const int *d_col_indices, const int *d_in_v, const int *d_in_row_start,
                       const int *d_in_scan, int in_len, int in_edges, int r_type, int r_op, int value_type, int by_vertex, int prefill,
                       long long out_len, const void *d_values, void *d_reduced, int functor, const int *d_mask, int *d_edge_hits,
                       int *d_edge_src, int max_grid_size);

/* The device building blocks under the operators, each by itself (lib/blocks_app.hip).  All d_ pointers are device pointers;
 * every function returns 0, a HIP error code, -1 for an argument that makes no sense or -2 for a combination that is not
 * instantiated. */
enum grx_scan_out { GRX_SCAN_INT = 0, GRX_SCAN_UINT = 1, GRX_SCAN_ULONGLONG = 2 };
/* graphio::DeviceExclusiveScan<out_type>: d_out[i] = d_in[0] + ... + d_in[i - 1], computed in 64 bits and stored as out_type;
 * *total (host) = the 64-bit grand total, read from the scratch word behind the tile offsets. */
int grx_device_scan(const unsigned *d_in, long long n, int out_type, void *d_out, unsigned long long *total);
/* ONE graphio::DeviceKeySort sorts `arrays` key arrays one after the other: array a has counts[a] keys (host array), stored
 * back to back in d_in, and is sorted on its low key_bits[a] (1..64) bits; the results land back to back in d_out. */
int grx_device_key_sort(int arrays, const long long *counts, const int *key_bits, const unsigned long long *d_in,
                        unsigned long long *d_out);
/* graphio::DeviceTransposeCsr: d_inv_row_offsets[nodes + 1], d_inv_col_indices[edges]; d_vals / d_inv_vals (both or neither):
 * one 32-bit value per edge that travels with it. */
int grx_device_transpose(int nodes, long long edges, const int *d_row_offsets, const int *d_col_indices, const unsigned *d_vals,
                         int *d_inv_row_offsets, int *d_inv_col_indices, unsigned *d_inv_vals);
enum grx_wave_op {
    GRX_WAVE_INCLUSIVE_SUM = 0,      /* util::WaveInclusiveSum: int, unsigned, unsigned long long */
    GRX_WAVE_INCLUSIVE_SUM_DPP = 1,  /* util::WaveInclusiveSumDpp: unsigned */
    GRX_WAVE_INCLUSIVE_MAX_DPP = 2,  /* util::WaveInclusiveMaxDpp: unsigned */
    GRX_WAVE_SEGMENTED_SCAN_DPP = 3, /* util::WaveSegmentedScanDpp<ReduceOps<r_op, type>>: the pairs of grx_advance_reduce but float MULTIPLIES */
    GRX_WAVE_SUM = 4,                /* util::WaveSum: int, unsigned, unsigned long long */
    GRX_WAVE_RANK_IN_MASK = 5,       /* util::RankInMask: unsigned long long masks in, unsigned ranks out */
    GRX_WAVE_BLOCK_SCAN = 6,         /* util::BlockScan<threads, type>::ExclusiveSum, twice: int, unsigned long long */
    GRX_WAVE_DPP_MOVE = 7            /* util::DppMove: unsigned, unsigned long long; r_op = step 0..5 of the scan network */
};
/* what a lane without a source shows after GRX_WAVE_DPP_MOVE (its low word for 32-bit values) */
#define GRX_DPP_MOVE_IDENTITY 0xA5A5A5A55A5A5A5Aull
/* A grid of workgroups of `threads` (64, 256 or 1024) threads; thread i of the launch, lane i % 64 of its wave, loads d_in[i],
 * calls the block and stores d_out[i]; threads past n take part with a zero.  r_op: the grx_reduce_op of a segmented scan
 * (d_heads[i] != 0 opens a segment at element i; NULL: no heads), or the step of a DPP move: 0..3 = row_shr 1, 2, 4, 8,
 * 4 = row_bcast:15 under row mask 0xA, 5 = row_bcast:31 under row mask 0xC.  BLOCK_SCAN scans the elements of a workgroup, then,
 * on the same storage, the same elements in mirrored order (thread t takes element threads - 1 - t of its workgroup):
 * d_out[i] = first result, d_aux[i], d_aux[n + i], d_aux[2n + i] = first total, second result and second total as thread i
 * received them.  d_aux is unused otherwise. */
int grx_wave_ops(int op, int r_op, int value_type, int threads, long long n, const void *d_in, const unsigned char *d_heads, void *d_out,
                 void *d_aux);
/* priority_queue::Bisect<256, 4, SSSPProblem<int, int, int, mark_paths>, PQFunctor> over the queue d_in (-1 = no entry) with a data
 * slice filled from the arguments: d_dist = one unsigned distance per vertex, or with mark_paths one packed
 * (distance << 32 | predecessor) word; d_visit_lookup; delta.  d_in_dist (or NULL): the distance each entry was parked with.
 * d_num_elements (or NULL): packed device tail whose low word is the element count; num_elements is then the upper bound that
 * sizes the grid.  Outputs: the near frontier (near_capacity entries of v, row_start, scan), the far pile (far_capacity
 * entries of vertex and distance), and on the host the packed near tail (count | edges << 32), the far tail, the smallest
 * far bucket (UINT_MAX when nothing was parked) and the overflow flag.  max_grid_size: 0 = one resident grid. */
int grx_bisect_queue(const int *d_row_offsets, const void *d_dist, int mark_paths, int *d_visit_lookup, float delta, const int *d_in,
                     const unsigned *d_in_dist, int num_elements, const unsigned long long *d_num_elements, unsigned level, int tag,
                     int near_capacity, int *d_near_v, int *d_near_row_start, int *d_near_scan, int far_capacity, int *d_far_v,
                     unsigned *d_far_d, unsigned long long *near_tail, unsigned long long *far_tail, unsigned *far_min, int *overflow,
                     int max_grid_size);

/* DisplayStats' counters (reference tests/bfs/test_bfs.cu:184-196): visited vertices and the sum of their
 * out-degrees -- the numerator of MTEPS = edges_visited / (elapsed_ms * 1000) */
void grx_bfs_count_visited(int nodes, const int *row_offsets, const int *labels,
                           long long *nodes_visited, long long *edges_visited);

/* ------------------------------------------------------------------------------------------------
 * CC: CCProblem + CCEnactor (reference gunrock/app/cc/cc_problem.cuh:36-440, cc_enactor.cuh:36-919)
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_cc grx_cc;

int grx_cc_create(grx_cc **out, int instrument, int device);
/* CCProblem::Init(false, csr, 1) (reference cc_problem.cuh:221-345) */
int grx_cc_init(grx_cc *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
int grx_cc_init_device(grx_cc *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* CCProblem::Reset(frontier_type) (reference cc_problem.cuh:361-440) */
int grx_cc_reset(grx_cc *p);
/* CCEnactor::Enact(problem, max_grid_size) (reference cc_enactor.cuh:889-919), HIP-event timed */
int grx_cc_enact(grx_cc *p, int max_grid_size, float *elapsed_ms);
/* sweeps of the last Enact: edge sweeps (hooks) and vertex sweeps (jumps / mask updates) -- I_h and I_j of the
 * roofline figure -- plus, when instrumented, kernel launches and their summed time */
int grx_cc_stats(grx_cc *p, long long *edge_sweeps, long long *vertex_sweeps, long long *kernel_launches, double *kernel_ms);
/* CCProblem::Extract(h_component_ids) (reference cc_problem.cuh:144-175); num_components = #{v: id[v] == v} */
/* *mirrored = 1 when Init found every edge (f, t), f < t, mirrored by (t, f): the hooking sweeps then park that orientation on first
 * sight (its mirror performs the identical root comparison), i.e. from the second edge sweep on half of the edges are skipped */
int grx_cc_mirrored(grx_cc *p, int *mirrored);
/* edges the hooking sweeps run over: all of them, or -- mirrored input -- only the from > to orientation of every edge, which the
 * problem materialises once at init (the other orientation performs the identical hooks) */
int grx_cc_sweep_edges(grx_cc *p, long long *edges);
int grx_cc_extract(grx_cc *p, int *h_component_ids, unsigned *num_components);
int grx_cc_device_results(grx_cc *p, int **d_component_ids);
void grx_cc_destroy(grx_cc *p);

/* ------------------------------------------------------------------------------------------------
 * MST: MSTProblem + MSTEnactor (reference gunrock/app/mst/mst_problem.cuh:44-520, mst_enactor.cuh:48-1260), a minimum
 * spanning FOREST.  The CSR is read as an undirected multigraph: every entry e = (u, v, w), u != v, is one edge {u, v} of
 * weight w (self-loops ignored; unsorted rows, duplicates, parallel edges and asymmetric input allowed).  Entries are ordered
 * by (w as signed int32, then e); under that strict order the forest is unique and is what Kruskal over the sorted entries
 * returns.  Any int32 weight is allowed.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_mst grx_mst;

int grx_mst_create(grx_mst **out, int instrument, int device);
/* MSTProblem::Init(false, csr, 1) (reference mst_problem.cuh:252-495).  -1: nodes < 1, edges < 0 or a NULL array;
 * -2: not a CSR of `nodes` vertices (offsets not from 0 to edges, decreasing, or a column outside [0, nodes)) */
int grx_mst_init(grx_mst *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *edge_values);
/* the same for a CSR already in HBM (borrowed, not freed) */
int grx_mst_init_device(grx_mst *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_edge_values);
/* MSTProblem::Reset (reference mst_problem.cuh:501-520) */
int grx_mst_reset(grx_mst *p);
/* MSTEnactor::Enact(problem, max_grid_size) (reference mst_enactor.cuh:1198), HIP-event timed */
int grx_mst_enact(grx_mst *p, int max_grid_size, float *elapsed_ms);
/* Borůvka rounds of the last Enact, entries their minimum steps read, kernel launches and -- when instrumented -- the summed time
 * of the rounds */
int grx_mst_stats(grx_mst *p, long long *rounds, long long *edges_scanned, long long *kernel_launches, double *kernel_ms);
/* per round of the last Enact: entries read by its minimum step and (instrumented) its time; returns the number of rounds */
int grx_mst_round_trace(grx_mst *p, int max_rounds, long long *entries, double *ms);
/* MSTProblem::Extract(h_mst_output) (reference mst_problem.cuh:218): h_selected[e] = 1 exactly on the forest's CSR entries;
 * total_weight = sum of their weights, forest_edges = their number (components = nodes - forest_edges) */
int grx_mst_extract(grx_mst *p, int *h_selected /* may be NULL */, long long *total_weight, int *forest_edges);
int grx_mst_device_results(grx_mst *p, int **d_selected);
void grx_mst_destroy(grx_mst *p);

/* ------------------------------------------------------------------------------------------------
 * MIS: MISProblem + MISEnactor (reference gunrock/app/mis/mis_problem.cuh:41-360, mis_enactor.cuh:40-440): a maximal
 * independent set and two greedy colourings.  The CSR is read as an undirected simple graph: u and v are neighbours when v
 * is in row u or u is in row v (self-loops ignored; unsorted rows, duplicates and asymmetric input allowed).  Vertices are
 * ordered by key(v) = (prio(v), v), compared lexicographically: prio is the caller's array as signed int32, or -- priorities
 * NULL -- fmix32((uint32)v + seed * 0x9E3779B9) as unsigned (fmix32 = MurmurHash3's 32-bit finaliser).  With H(v) = the
 * neighbours of v with a larger key, each mode's result is the unique solution of its equation, which is what the sequential
 * greedy pass over the vertices in descending key order writes:
 *   GRX_MIS_SET              ids[v] = 1 iff no u in H(v) has ids[u] = 1, else 0 (the lexicographically first maximal set)
 *   GRX_MIS_COLOR_ROUNDS     ids[v] = 1 + max(ids[u], u in H(v)), 1 when H(v) is empty: what the reference's schedule
 *                            (mis_functor.cuh:84-89, mis_enactor.cuh:234-363) writes when run to the end with distinct labels
 *   GRX_MIS_COLOR_FIRST_FIT  ids[v] = the smallest positive integer not among ids[u], u in H(v) (Jones-Plassmann)
 * Unlike the reference: ties cannot occur (its `>=` lets two adjacent vertices with equal labels take one colour); there is
 * no iteration cap (its driver stops after 20 and leaves -1), Enact runs to completion; the order is a seeded hash or the
 * caller's, not std::random_shuffle.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_mis grx_mis;
enum { GRX_MIS_SET = 0, GRX_MIS_COLOR_ROUNDS = 1, GRX_MIS_COLOR_FIRST_FIT = 2 };

int grx_mis_create(grx_mis **out, int instrument, int device);
/* MISProblem::Init (reference mis_problem.cuh:145-310).  priorities: `nodes` values or NULL (hashed with `seed`).
 * -1: nodes < 1, edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices, as grx_mst_init; -3: the handle has been
 * given a graph before (accepted or rejected): a handle takes one graph, create another */
int grx_mis_init(grx_mis *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *priorities,
                 unsigned seed);
/* the same for a CSR (and priorities, or NULL) already in HBM (borrowed, not freed) */
int grx_mis_init_device(grx_mis *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_priorities, unsigned seed);
/* enable = 0: one kernel launch and one read-back per round to the end, instead of finishing the long thin tail of the
 * schedule in launches that loop on the device (the default).  The result is the same; for measurements. */
int grx_mis_set_tail(grx_mis *p, int enable);
/* MISProblem::Reset (reference mis_problem.cuh:320-346): every vertex undecided */
int grx_mis_reset(grx_mis *p);
/* MISEnactor::Enact(problem, max_grid_size) (reference mis_enactor.cuh:419) for one of the modes above, HIP-event timed */
int grx_mis_enact(grx_mis *p, int mode, int max_grid_size, float *elapsed_ms);
/* of the last Enact: host-visible sweeps (kernel launches with a read-back), sweeps made inside the device-side tail loop,
 * row entries walked, polls (a blocked vertex asking its one blocking entry again), kernel launches (sweeps, tail windows and
 * the two kernels around the tail's ordering; the radix sort's own kernels are not counted) and -- when instrumented -- the
 * summed time of the rounds */
int grx_mis_stats(grx_mis *p, long long *rounds, long long *tail_sweeps, long long *entries_read, long long *polls,
                  long long *kernel_launches, double *kernel_ms);
/* per host-visible round of the last Enact: undecided vertices it started with and (instrumented) its time; returns the rounds */
int grx_mis_round_trace(grx_mis *p, int max_rounds, long long *vertices, double *ms);
/* MISProblem::Extract(h_mis_ids) (reference mis_problem.cuh:106); summary = the size of the set, or the number of colours */
int grx_mis_extract(grx_mis *p, int *h_ids /* may be NULL */, long long *summary);
int grx_mis_device_results(grx_mis *p, int **d_ids);
void grx_mis_destroy(grx_mis *p);

/* ------------------------------------------------------------------------------------------------
 * TC: TCProblem + TCEnactor: triangle counts and clustering coefficients (the reference snapshot has no app/tc; later Gunrock
 * releases do).  The CSR is read as grx_mis_* reads it: the simple undirected graph G in which u and v are neighbours when v
 * is in row u or u is in row v (self-loops ignored; unsorted rows, duplicates and one-way edges allowed), with M edges and
 * degrees d(v).  Every result has exactly one value:
 *   triangles[v]   the number of unordered pairs of neighbours of v that are neighbours (64-bit)
 *   total          the number of triangles of G = sum(triangles) / 3 (64-bit)
 *   clustering[v]  2 triangles[v] / (d(v) (d(v) - 1)) as one double division, 0.0 where d(v) < 2
 *   transitivity   3 total / sum over v of C(d(v), 2) as one double division, 0.0 when there is no wedge
 * Init orients every edge from the endpoint with the smaller (d, id) to the larger (no out-row exceeds floor(sqrt(2 M))) and
 * Enact intersects the out-rows of the two ends of every oriented edge, in one of three regimes picked by the row's length.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_tc grx_tc;
enum { GRX_TC_AUTO = 0, GRX_TC_LANE = 1, GRX_TC_LDS = 2, GRX_TC_GLOBAL = 3 };

int grx_tc_create(grx_tc **out, int instrument, int device);
/* TCProblem::Init: validates the CSR and builds the oriented graph on the device.  -1: nodes < 1, edges < 0 or a NULL array;
 * -2: not a CSR of `nodes` vertices, as grx_mis_init; -3: the handle has been given a graph before (accepted or rejected) */
int grx_tc_init(grx_tc *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM (borrowed, not freed) */
int grx_tc_init_device(grx_tc *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.
 *   "strategy"      GRX_TC_AUTO (default): rows up to "lane_max_row" entries take one lane per oriented edge, rows up to
 *                   "lds_entries" one workgroup with the row staged in LDS, longer rows one workgroup probing the row in global
 *                   memory; GRX_TC_LANE / GRX_TC_LDS / GRX_TC_GLOBAL force that regime for every row (under GRX_TC_LDS a row
 *                   beyond "lds_entries" still takes the global one).  The result does not depend on it.
 *   "lds_entries"   the staging budget in row entries (default 4096, at most 8192: 8 bytes of LDS each)
 *   "lane_max_row"  the longest row of the lane regime under GRX_TC_AUTO (default 32) */
int grx_tc_set_option(grx_tc *p, const char *name, double value);
/* TCProblem::Reset: the counts to zero */
int grx_tc_reset(grx_tc *p);
/* TCEnactor::Enact(problem, max_grid_size), HIP-event timed */
int grx_tc_enact(grx_tc *p, int max_grid_size, float *elapsed_ms);
/* oriented edges (M) and the largest out-row of the graph; of the last Enact: row entries streamed through an intersection,
 * kernel launches, the non-empty rows the lane / LDS / global regimes took (regime_rows[3], may be NULL) and -- when
 * instrumented -- the summed kernel time; build_ms: the HIP-event time of Init's oriented-graph build */
int grx_tc_stats(grx_tc *p, long long *oriented_edges, long long *max_out_row, long long *entries_probed, long long *kernel_launches,
                 long long *regime_rows, double *kernel_ms, double *build_ms);
int grx_tc_extract(grx_tc *p, long long *h_triangles /* may be NULL */, long long *total);
int grx_tc_clustering(grx_tc *p, double *h_coeff /* may be NULL */, double *transitivity);
/* device arrays of the handle: 64-bit counts and 32-bit degrees d(v), `nodes` each */
int grx_tc_device_results(grx_tc *p, long long **d_triangles, int **d_degrees);
void grx_tc_destroy(grx_tc *p);

/* ------------------------------------------------------------------------------------------------
 * KCORE: KcoreProblem + KcoreEnactor: the k-core decomposition (the reference snapshot has no app/kcore; later Gunrock releases
 * do).  The CSR is read as grx_mis_* / grx_tc_* read it: the simple undirected graph G with M edges and degrees d(v).  The
 * k-core is the largest subgraph in which every vertex has at least k neighbours inside the subgraph.  Every result has one value:
 *   core[v]      the largest k whose k-core holds v (int32); 0 exactly where d(v) = 0, never more than d(v)
 *   degeneracy   the largest core[v]
 *   shell[k]     the number of vertices with core[v] = k, k = 0 .. degeneracy (64-bit)
 *   members(k)   the mask core[v] >= k, the number of such vertices and the number of edges of G between them (64-bit)
 * and a run limited to K gives min(core[v], K).  A degeneracy ordering is not offered: it is not unique.
 * Init builds the symmetric simple neighbour CSR; Enact peels by levels (a vertex at the level takes one off every live
 * neighbour with a returning atomic; the next level is the smallest value left), in wide launches or in a loop on the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_kcore grx_kcore;
enum { GRX_KCORE_AUTO = 0, GRX_KCORE_ROUNDS = 1, GRX_KCORE_DEVICE_LOOP = 2 };

int grx_kcore_create(grx_kcore **out, int instrument, int device);
/* KcoreProblem::Init: validates the CSR and builds the neighbour CSR and d(v) on the device.  -1: nodes < 1, edges < 0 or a
 * NULL array; -2: not a CSR of `nodes` vertices, as grx_tc_init; -3: the handle has been given a graph before (accepted or
 * rejected) */
int grx_kcore_init(grx_kcore *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM (borrowed, not freed) */
int grx_kcore_init_device(grx_kcore *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  None changes a result.
 *   "schedule"          GRX_KCORE_AUTO (default): a step (the scan that opens a level, a sub-round, a rebuild of the live list)
 *                       is a launch of its own while it is wide, and everything else runs in a loop on the device, one launch
 *                       and one read-back for a whole stretch of sub-rounds and levels; GRX_KCORE_ROUNDS: every step is a launch
 *                       and a read-back (the plain form, for comparison); GRX_KCORE_DEVICE_LOOP: every step runs in the device loop
 *   "compact_below"     in [0, 1]: the live list is rebuilt at a level's start when the live vertices are at most this share of
 *                       its length (default 0.75; 0: never)
 *   "wave_min_row"      >= 1: rows of at least this many entries are walked by the whole wave, shorter ones by a lane (default 16)
 *   "loop_max_list"     under AUTO the device loop scans a live list of at most this length (default 32768)
 *   "loop_max_entries"  under AUTO the device loop runs a sub-round whose rows hold at most this many entries (default 8192) */
int grx_kcore_set_option(grx_kcore *p, const char *name, double value);
/* KcoreProblem::Reset: core[v] = d(v), every vertex with a neighbour live */
int grx_kcore_reset(grx_kcore *p);
/* KcoreEnactor::Enact(problem, k_limit, max_grid_size), HIP-event timed.  k_limit >= 0: the levels below k_limit are peeled
 * and the result is min(core[v], k_limit) */
int grx_kcore_enact(grx_kcore *p, int k_limit /* < 0: to the end */, int max_grid_size, float *elapsed_ms);
/* edges (M) and the largest d(v) of the graph; of the last Enact: the non-empty levels, the host-visible read-backs, the
 * vertices given a core number by peeling (those with d(v) = 0 count: `nodes` after a full run), row entries walked, rebuilds
 * of the live list, kernel launches and -- when instrumented -- the summed kernel time; build_ms: the HIP-event time of
 * Init's neighbour-CSR build */
int grx_kcore_stats(grx_kcore *p, long long *simple_edges, long long *max_degree, long long *levels, long long *rounds,
                    long long *vertices_peeled, long long *entries_read, long long *compactions, long long *kernel_launches,
                    double *kernel_ms, double *build_ms);
/* the non-empty levels of the last Enact in ascending order, at most max_levels of them: the level, the vertices peeled at it
 * and the time from its scan to the next level's by the device's constant-rate counter; returns the number of levels */
int grx_kcore_level_trace(grx_kcore *p, int max_levels, int *k, long long *vertices, double *ms);
int grx_kcore_extract(grx_kcore *p, int *h_core /* may be NULL */, int *degeneracy);
/* h_sizes[k] = the vertices with core k, for k < max_entries; returns degeneracy + 1 (negative: an error) */
int grx_kcore_shells(grx_kcore *p, int max_entries, long long *h_sizes);
/* the k-core of the last Enact's result: the mask core[v] >= k (one byte per vertex), its vertices and the edges of G inside */
int grx_kcore_members(grx_kcore *p, int k, unsigned char *h_mask /* may be NULL */, long long *vertices, long long *edges);
/* device arrays of the handle: 32-bit core numbers and 32-bit degrees d(v), `nodes` each */
int grx_kcore_device_results(grx_kcore *p, int **d_core, int **d_degrees);
void grx_kcore_destroy(grx_kcore *p);

/* ------------------------------------------------------------------------------------------------
 * TRUSS: TrussProblem + TrussEnactor: per-edge triangle support and the k-truss decomposition (the reference snapshot has no
 * app/truss; later Gunrock releases and the GraphChallenge do).  The CSR is read as grx_mis_* / grx_tc_* / grx_kcore_* read it:
 * the simple undirected graph G.  Its M edges (a, b), a < b, sorted by (a, b), are the canonical edge order; every per-edge array
 * is indexed by that rank e.  The k-truss is the largest subgraph in which every edge is in at least k - 2 triangles of the
 * subgraph.  Every result has one value:
 *   support[e]       the triangles of G that hold e (int32); sum(support) = 3 * triangles
 *   truss[e]         the largest k whose k-truss holds e (int32); 2 for an edge in no triangle, never more than support[e] + 2
 *   max_truss        the largest truss[e]; 0 when M = 0
 *   classes[k]       the number of edges with truss[e] = k, k = 0 .. max_truss (64-bit; entries 0 and 1 are 0)
 *   members(k)       the mask truss[e] >= k, the number of such edges and of the vertices at one of them (64-bit)
 *   vertex_truss[v]  the largest truss over the edges at v (int32); 0 for a vertex without a neighbour
 * and a run limited to K gives min(truss[e], K).  A truss ordering is not offered: it is not unique.
 * Init builds the canonical edges, the neighbour CSR with an edge id beside every entry and the supports; Enact peels by levels
 * (an edge at the level takes one off the two other edges of every live triangle with a returning atomic; the next level is the
 * smallest value left), in wide launches or in a loop on the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_truss grx_truss;
enum { GRX_TRUSS_AUTO = 0, GRX_TRUSS_ROUNDS = 1 };

int grx_truss_create(grx_truss **out, int instrument, int device);
/* TrussProblem::Init: validates the CSR, builds the edges, the neighbour CSR and support[] on the device.  -1: nodes < 1,
 * edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices, as grx_tc_init; -3: the handle has been given a graph before
 * (accepted or rejected) */
int grx_truss_init(grx_truss *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM (borrowed, not freed) */
int grx_truss_init_device(grx_truss *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* named options; 0: set, 1: unknown name, -1: a value out of range.  None changes a result.
 *   "schedule"          GRX_TRUSS_AUTO (default): a step (the scan that opens a level, a sub-round) is a launch of its own while
 *                       it is wide, and everything else runs in a loop on the device, one launch and one read-back for a whole
 *                       stretch of sub-rounds; GRX_TRUSS_ROUNDS: every step is a launch and a read-back (the plain form)
 *   "wave_min_row"      >= 1: an intersection whose shorter row has at least this many entries is walked by the whole wave, a
 *                       shorter one by a lane (default 32); set before Init it also holds for the support pass
 *   "loop_max_list"     under AUTO the device loop scans the edges of a graph with at most this many (default 32768)
 *   "loop_max_entries"  under AUTO the device loop runs a sub-round whose shorter rows hold at most this many entries
 *                       (default 8192) */
int grx_truss_set_option(grx_truss *p, const char *name, double value);
/* TrussProblem::Reset: the working array = support[], every edge live */
int grx_truss_reset(grx_truss *p);
/* TrussEnactor::Enact(problem, k_limit, max_grid_size), HIP-event timed.  k_limit >= 0: the levels below k_limit are peeled
 * and the result is min(truss[e], k_limit).  An Enact that does not follow a Reset makes its own */
int grx_truss_enact(grx_truss *p, int k_limit /* < 0: to the end */, int max_grid_size, float *elapsed_ms);
/* edges (M), triangles and the largest support[e] of the graph; of the last Enact: the non-empty levels, the sub-rounds (those of
 * the synchronous peel under either schedule; the scans of levels nobody is at are not counted), the edges peeled (M after a
 * full run), row entries walked by the support pass and by the peel, kernel launches, host-visible read-backs and -- when
 * instrumented -- the summed kernel time; build_ms and support_ms: the HIP-event times of Init's build and of its support pass */
int grx_truss_stats(grx_truss *p, long long *simple_edges, long long *triangles, long long *max_support, long long *levels,
                    long long *rounds, long long *edges_peeled, long long *support_entries, long long *peel_entries,
                    long long *kernel_launches, long long *readbacks, double *kernel_ms, double *build_ms, double *support_ms);
/* the non-empty levels of the last Enact in ascending order, at most max_levels of them: k, the edges peeled at it and the
 * time from its scan to the next level's by the device's constant-rate counter; returns the number of levels */
int grx_truss_level_trace(grx_truss *p, int max_levels, int *k, long long *edges, double *ms);
/* the canonical edges; returns M (negative: an error); either array may be NULL */
int grx_truss_edges(grx_truss *p, int *h_src, int *h_dst);
/* valid after Init, no Enact needed */
int grx_truss_support(grx_truss *p, int *h_support /* may be NULL */, long long *total_triangles);
int grx_truss_extract(grx_truss *p, int *h_truss /* may be NULL */, int *max_truss);
/* h_sizes[k] = the edges with truss k, for k < max_entries; returns max_truss + 1 (negative: an error) */
int grx_truss_classes(grx_truss *p, int max_entries, long long *h_sizes);
/* the k-truss of the last Enact's result: the mask truss[e] >= k (one byte per edge), its edges and the vertices at them */
int grx_truss_members(grx_truss *p, int k, unsigned char *h_mask /* may be NULL */, long long *edges, long long *vertices);
int grx_truss_vertex_truss(grx_truss *p, int *h_vertex_truss);
/* device arrays of the handle, M 32-bit entries each */
int grx_truss_device_results(grx_truss *p, int **d_truss, int **d_support, int **d_src, int **d_dst);
void grx_truss_destroy(grx_truss *p);

/* ------------------------------------------------------------------------------------------------
 * SCC: SccProblem + SccEnactor: strongly connected components (the reference snapshot has no app/scc; later Gunrock releases
 * do).  The directed counterpart of grx_cc_*: the CSR is read as a directed multigraph (duplicates and self-loops allowed and
 * without effect, rows unsorted, nothing symmetrised).  Every result has one value:
 *   comp[v]       the smallest vertex id of v's strongly connected component (int32)
 *   components    the number of components; trivial: those of one vertex; largest: the vertex count of the largest one and
 *                 largest_root its comp value (ties go to the smaller root)
 *   size[v]       the vertex count of v's component (int32)
 *   condensation  the distinct pairs (comp[u], comp[v]) over the edges u -> v between components, sorted by (from, to): a DAG
 * A topological order of the condensation is not offered: it is not unique.
 * Init adds the transpose; Enact trims (a vertex without a live in- or out-edge is a component, and so are two vertices whose
 * only live in-edges, or out-edges, are each other's), splits off the component of
 * one high-degree pivot by a forward and a backward search, and finishes the rest in colouring rounds (the largest id
 * propagated forward, a backward search from every vertex that kept its own), in wide launches or in a loop on the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_scc grx_scc;
enum { GRX_SCC_AUTO = 0, GRX_SCC_ROUNDS = 1, GRX_SCC_DEVICE_LOOP = 2 };
enum { GRX_SCC_PHASE_TRIM = 0, GRX_SCC_PHASE_PIVOT = 1, GRX_SCC_PHASE_COLOUR = 2 }; /* the kinds of grx_scc_phase_trace */

/* (no counterpart in the reference snapshot: this call and the ones below are shaped like grx_kcore_*) */
int grx_scc_create(grx_scc **out, int instrument, int device);
/* SccProblem::Init: validates the CSR and builds its transpose on the device (no reference counterpart).  -1: nodes < 1,
 * edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices, as grx_tc_init; -3: the handle has been given a graph before
 * (accepted or rejected) */
int grx_scc_init(grx_scc *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM (borrowed, not freed; no reference counterpart).  d_inv_row_offsets / d_inv_col_indices: the
 * transpose, borrowed and validated too, or both NULL: then it is built.  One of the two NULL is -1 */
int grx_scc_init_device(grx_scc *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_inv_row_offsets,
                        int *d_inv_col_indices);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  None changes a result (no reference
 * counterpart).
 *   "schedule"          GRX_SCC_AUTO (default): a step (a pass over the live list, a trim sub-round, a search level, a
 *                       propagation sweep) is a launch of its own while it is wide, and everything else runs in a loop on the
 *                       device, one launch and one read-back for a whole stretch of steps; GRX_SCC_ROUNDS: every step is a launch
 *                       and a read-back (the plain form, for comparison); GRX_SCC_DEVICE_LOOP: every step runs in the device loop
 *   "pivot_phase"       0 / 1 (default 1): 0 leaves everything after the first trim to the colouring rounds
 *   "trim"              0 / 1 (default 1).  0 is there for comparison and can be very slow: without trimming every component,
 *                       single vertices included, is left to the colouring rounds, and a chain of k small components whose ids
 *                       fall along the edges then costs k rounds of up to k sweeps each (2000 two-cycles with "pivot_phase" 0:
 *                       4.0 M sweeps, about 100 s measured)
 *   "pair_trim"         0 / 1 (default 1; it needs "trim"): when the peel has run dry, two vertices whose only live in-edges, or
 *                       out-edges, are each other's are finished as a component of two and the peel goes on from them
 *   "wave_min_row"      >= 1: rows of at least this many entries are walked by the whole wave, shorter ones by a lane (default 16)
 *   "loop_max_list"     under AUTO the device loop takes a step over at most this many vertices (default 32768)
 *   "loop_max_entries"  ... whose rows hold at most this many entries (default 8192) */
int grx_scc_set_option(grx_scc *p, const char *name, double value);
/* SccProblem::Reset: every vertex live in one region (no reference counterpart) */
int grx_scc_reset(grx_scc *p);
/* SccEnactor::Enact(problem, max_grid_size), HIP-event timed (no reference counterpart).  An Enact that does not follow a Reset
 * makes its own */
int grx_scc_enact(grx_scc *p, int max_grid_size, float *elapsed_ms);
/* of the last Enact (no reference counterpart): the vertices finished by trimming and the trim sub-rounds, the size of the
 * pivot's component (0 without a pivot phase), the colouring rounds, their propagation sweeps, the levels of all searches, row
 * entries walked, kernel launches and -- when instrumented -- the summed kernel time; build_ms: the HIP-event time of Init's
 * transpose (0 for a borrowed one) */
int grx_scc_stats(grx_scc *p, long long *trimmed, long long *trim_rounds, long long *pivot_component, long long *colour_rounds,
                  long long *sweeps, long long *bfs_levels, long long *entries_read, long long *kernel_launches, double *kernel_ms,
                  double *build_ms);
/* the phases of the last Enact in order, at most max_phases of them (no reference counterpart): the kind
 * (GRX_SCC_PHASE_*), the vertices finished in it and the time to the next phase's start by the device's constant-rate counter; returns the number of phases (the first 65536 are recorded) */
int grx_scc_phase_trace(grx_scc *p, int max_phases, int *kind, long long *vertices, double *ms);
/* (no reference counterpart) */
int grx_scc_extract(grx_scc *p, int *h_comp /* may be NULL */, long long *components);
/* (no reference counterpart) any pointer may be NULL */
int grx_scc_summary(grx_scc *p, long long *components, long long *trivial, long long *largest, int *largest_root);
/* (no reference counterpart) */
int grx_scc_sizes(grx_scc *p, int *h_size);
/* the first max_edges pairs of the condensation into h_from / h_to (either NULL, or max_edges 0: none is copied); returns the
 * number of pairs, which must fit an int, or a negated hipError_t (no reference counterpart) */
int grx_scc_condensation(grx_scc *p, int max_edges, int *h_from, int *h_to);
/* device arrays of the handle (no reference counterpart): comp (`nodes` int32) and the transpose it runs on (its own or the
 * borrowed one) */
int grx_scc_device_results(grx_scc *p, int **d_comp, int **d_inv_row_offsets, int **d_inv_col_indices);
void grx_scc_destroy(grx_scc *p);

/* ------------------------------------------------------------------------------------------------
 * MS-BFS: MsbfsProblem + MsbfsEnactor: breadth-first searches from k sources, 64 per pass over the edges (bit-parallel multi-source
 * BFS, Then et al., VLDB 2014; the reference snapshot has no counterpart).  The CSR is read as a directed multigraph, as grx_scc_*
 * reads it (duplicates and self-loops allowed and without effect, rows unsorted, nothing symmetrised).  Sources may repeat; each
 * gets its own row.  Every result is an integer with one value:
 *   depth[s][v]          int32, layout [source][vertex]: what grx_bfs_* labels v from sources[s]: 0 at the source, -1 where
 *                        unreachable.  Stored only on request: it is 4 * k * nodes bytes
 *   reached[s]           int64: the vertices with depth[s][v] >= 0, the source included
 *   dist_sum[s]          int64: the sum of those depths
 *   ecc[s]               int32: the largest of them
 *   sources_reaching[v]  int32: the sources s of the call with depth[s][v] >= 0 (a repeated source counts each time)
 *   in_dist_sum[v]       int64: the sum of depth[s][v] over them: the incoming distances of closeness centrality
 * Every vertex carries one 64-bit word per state array, bit b for the batch's source b.  A level is a push (the queue of frontier
 * vertices ORs its bits into the words of its out-neighbours with a returning atomic; the lane that finds a word empty queues the
 * vertex) or a pull (every vertex that some search has not reached ORs the frontier words of its in-neighbours and stops as soon
 * as nothing is missing).  Batches of 64 sources run one after another.  No float is produced on the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_msbfs grx_msbfs;
enum { GRX_MSBFS_AUTO = 0, GRX_MSBFS_PUSH = 1, GRX_MSBFS_PULL = 2, GRX_MSBFS_ALTERNATE = 3 };               /* option "direction" */
enum { GRX_MSBFS_INVERSE_AUTO = 0, GRX_MSBFS_INVERSE_NONE = 1, GRX_MSBFS_INVERSE_SELF = 2, GRX_MSBFS_INVERSE_BUILD = 3 }; /* option "inverse" */
enum { GRX_MSBFS_LEVEL_PUSH = 0, GRX_MSBFS_LEVEL_PULL = 1 };                                                 /* the kinds of the level trace */
enum { GRX_MSBFS_DEPTHS_NOT_STORED = -4, GRX_MSBFS_INVERSE_NOT_SYMMETRIC = -5 };                             /* codes next to -1 / -2 / -3 */

/* (no counterpart in the reference snapshot: this call and the ones below are shaped like the SCC handle's) */
int grx_msbfs_create(grx_msbfs **out, int instrument, int device);
/* MsbfsProblem::Init: validates the CSR (no reference counterpart).  -1: nodes < 1, edges < 0 or a NULL array; -2: not a CSR of
 * `nodes` vertices; -3: the handle has been given a graph before (accepted or rejected) */
int grx_msbfs_init(grx_msbfs *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM (borrowed, not freed; no reference counterpart).  d_inv_row_offsets / d_inv_col_indices: the
 * in-neighbour lists (the transpose), borrowed and validated too, or both NULL.  One of the two NULL is -1 */
int grx_msbfs_init_device(grx_msbfs *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_inv_row_offsets,
                          int *d_inv_col_indices);
/* named options; 0: set, 1: unknown name, -1: a value out of range.  None changes a result (no reference counterpart).
 *   "direction"     GRX_MSBFS_AUTO (default): push until the frontier's out-row entries times "alpha" exceed the row entries of
 *                   the vertices some search of the batch has not reached, then pull until the frontier's vertices times "beta"
 *                   fall below `nodes`; GRX_MSBFS_PUSH / GRX_MSBFS_PULL: every level that way; GRX_MSBFS_ALTERNATE: odd levels push,
 *                   even levels pull (both hand-overs on every graph, for tests).  Without in-neighbour lists every level is a push
 *   "inverse"       where a pull's in-neighbour lists come from, settled by the next Reset.  GRX_MSBFS_INVERSE_AUTO (default): the
 *                   ones lent at init_device, else the graph itself when the device symmetry check passes (sorted, duplicate-free
 *                   rows, every entry mirrored), else a transpose built on the device; GRX_MSBFS_INVERSE_NONE: none;
 *                   GRX_MSBFS_INVERSE_SELF: the graph itself, which that Reset refuses with GRX_MSBFS_INVERSE_NOT_SYMMETRIC when the
 *                   check does not pass (the check is conservative: unsorted rows or duplicates fail it); GRX_MSBFS_INVERSE_BUILD:
 *                   the lent ones, else a built transpose, without asking the check
 *   "alpha", "beta" > 0 (defaults 4 and 24)
 *   "wave_min_row"  >= 1: rows of at least this many entries are walked by the whole wave, shorter ones by a lane (default 16) */
int grx_msbfs_set_option(grx_msbfs *p, const char *name, double value);
/* MsbfsProblem::Reset: takes `count` >= 1 sources (copied) and sets every result to its value before the first level: depth 0 and
 * reached 1 at each source, nothing else reached (no reference counterpart).  store_depths 0: no depth array is kept.  -1: a NULL
 * array, count < 1 or a source outside [0, nodes), and GRX_MSBFS_INVERSE_NOT_SYMMETRIC as above: in both cases nothing has changed
 * and the handle stays usable (after the latter, with another "inverse") */
int grx_msbfs_reset(grx_msbfs *p, const int *sources, int count, int store_depths);
/* MsbfsEnactor::Enact(problem, max_grid_size), HIP-event timed (no reference counterpart).  An Enact that does not follow a Reset
 * repeats the last one */
int grx_msbfs_enact(grx_msbfs *p, int max_grid_size, float *elapsed_ms);
/* of the last Enact (no reference counterpart): batches, levels of all batches and how many were pushes and pulls, row entries
 * walked, kernel launches and -- when instrumented -- the summed level time; build_ms: the HIP-event time of a built transpose (0
 * when none was built).  Any pointer may be NULL */
int grx_msbfs_stats(grx_msbfs *p, long long *batches, long long *levels, long long *push_levels, long long *pull_levels,
                    long long *entries_read, long long *kernel_launches, double *kernel_ms, double *build_ms);
/* the levels of the last Enact in order, at most max_levels of them (no reference counterpart): the batch, the depth the level
 * assigns (1, 2, ...; a batch's last level reaches nothing, so a batch has its largest eccentricity + 1 levels), the kind
 * (GRX_MSBFS_LEVEL_*), the vertices and out-row entries of the frontier it starts from and -- when instrumented -- its time;
 * returns the number of levels.  Any array may be NULL */
int grx_msbfs_level_trace(grx_msbfs *p, int max_levels, int *batch, int *level, int *kind, long long *frontier, long long *edges,
                          double *ms);
/* rows [first_source, first_source + source_count) of depth[][] into h_depth, source_count * nodes int32 (no reference
 * counterpart).  GRX_MSBFS_DEPTHS_NOT_STORED after a Reset with store_depths 0; -1: a range outside the sources */
int grx_msbfs_extract_depths(grx_msbfs *p, int first_source, int source_count, int *h_depth);
/* `count` entries each, any pointer may be NULL (no reference counterpart) */
int grx_msbfs_source_summary(grx_msbfs *p, long long *reached, long long *dist_sum, int *ecc);
/* `nodes` entries each, any pointer may be NULL (no reference counterpart) */
int grx_msbfs_vertex_summary(grx_msbfs *p, int *sources_reaching, long long *in_dist_sum);
/* device arrays of the handle (no reference counterpart): depth (NULL when not stored) and the five summaries */
int grx_msbfs_device_results(grx_msbfs *p, int **d_depth, long long **d_reached, long long **d_dist_sum, int **d_ecc,
                             int **d_sources_reaching, long long **d_in_dist_sum);
void grx_msbfs_destroy(grx_msbfs *p);

/* ------------------------------------------------------------------------------------------------
 * BCC: BccProblem + BccEnactor: biconnected components (blocks), articulation points, bridges and 2-edge-connected components
 * (Tarjan and Vishkin, SIAM J. Comput. 1985, on a breadth-first forest; the reference snapshot has no counterpart, later Gunrock
 * releases do).  The CSR is read as grx_mis_*, grx_tc_*, grx_kcore_* and grx_truss_* read it: the simple undirected graph G (entries
 * symmetrised, duplicates and self-loops dropped, rows may be unsorted, a directed input is read undirected).  Parallel entries
 * collapse to one edge, so a doubled edge can still be a bridge.  The M canonical edges are (a, b), a < b, sorted by (a, b); edge
 * index e is the position in that list, as in grx_truss_edges.  Every result is an integer with one value:
 *   bcc[e]           the smallest canonical edge index in the block that holds edge e (int32, M entries)
 *   block_size[e]    the number of edges in the block of e (int32)
 *   bridge[e]        1 iff the block of e is that edge alone (uint8, M entries)
 *   articulation[v]  1 iff the edges at v carry at least two block ids (uint8, `nodes` entries)
 *   tecc[v]          the smallest vertex id in the 2-edge-connected component of v: its component in G minus the bridges (int32,
 *                    `nodes` entries; a vertex without a neighbour is its own)
 *   block-cut tree   the distinct pairs (v, bcc id) over the articulation points v and the blocks at them, sorted by (v, id)
 * An order of the block-cut tree (a root, a traversal) is not offered: it is not unique.
 * Init builds the neighbour CSR with edge ids; Enact finds the component minima by hook-and-jump, searches breadth-first from all of
 * them at once, computes subtree sizes, preorder numbers and low / high level by level, joins tree edges in a union-find, and labels
 * edges and vertices from the sets, in wide launches or in a loop on the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_bcc grx_bcc;
enum { GRX_BCC_AUTO = 0, GRX_BCC_ROUNDS = 1, GRX_BCC_DEVICE_LOOP = 2 };
enum {
    GRX_BCC_PHASE_FOREST = 0,
    GRX_BCC_PHASE_SIZES = 1,
    GRX_BCC_PHASE_NUMBER = 2,
    GRX_BCC_PHASE_LOWHIGH = 3,
    GRX_BCC_PHASE_LINK = 4,
    GRX_BCC_PHASE_LABEL = 5
}; /* the kinds of grx_bcc_phase_trace */

/* (no counterpart in the reference snapshot: this call and the ones below are shaped like grx_scc_* and grx_truss_*) */
int grx_bcc_create(grx_bcc **out, int instrument, int device);
/* BccProblem::Init: validates the CSR and builds the canonical edges and the neighbour CSR on the device (no reference counterpart).
 * -1: nodes < 1, edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices, as grx_kcore_init; -3: the handle has been given a
 * graph before (accepted or rejected) */
int grx_bcc_init(grx_bcc *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM (borrowed, not freed; no reference counterpart) */
int grx_bcc_init_device(grx_bcc *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  None changes a result (no reference
 * counterpart).
 *   "schedule"          GRX_BCC_AUTO (default): a level of one of the four level chains (search, sizes, numbering, low / high) is a
 *                       launch of its own while it is wide, and a stretch of narrow levels runs in a loop on the device, one launch
 *                       for up to 4096 levels; GRX_BCC_ROUNDS: every level is a launch (the plain form, for comparison);
 *                       GRX_BCC_DEVICE_LOOP: every level runs in the device loop
 *   "wave_min_row"      >= 1: rows of at least this many entries are walked by the whole wave, shorter ones by a lane (default 16,
 *                       taken over from grx_scc_*, not tuned).  A large value is a performance cliff, not an error: a hub's row is
 *                       then walked by one lane while the other 63 of its wave wait
 *   "loop_max_list"     under AUTO the device loop takes a level of at most this many vertices (default 32768, not tuned)
 *   "loop_max_entries"  ... whose rows hold at most this many entries (default 8192, not tuned) */
int grx_bcc_set_option(grx_bcc *p, const char *name, double value);
/* BccProblem::Reset (no reference counterpart) */
int grx_bcc_reset(grx_bcc *p);
/* BccEnactor::Enact(problem, max_grid_size), HIP-event timed (no reference counterpart).  An Enact that does not follow a Reset
 * makes its own */
int grx_bcc_enact(grx_bcc *p, int max_grid_size, float *elapsed_ms);
/* the simple edges M of the graph and, of the last Enact (no reference counterpart): the trees of the forest (components with an
 * edge), the levels of the search, row entries walked, kernel launches, host read-backs and -- when instrumented -- the summed
 * kernel time; build_ms: the HIP-event time of Init's build.  The seven one-thread launches that stamp the phase trace and the
 * memsets of an Enact are in neither kernel_launches nor kernel_ms */
int grx_bcc_stats(grx_bcc *p, long long *simple_edges, long long *trees, long long *levels, long long *entries_read,
                  long long *kernel_launches, long long *readbacks, double *kernel_ms, double *build_ms);
/* the six phases of the last Enact in order, at most max_phases of them (no reference counterpart): the kind (GRX_BCC_PHASE_*), the
 * vertices (forest, sizes, numbering, low / high), edges (link) or edges and vertices (label) it touched, and the time to the next
 * phase's start by the device's constant-rate counter; returns the number of phases (0 before the first Enact) */
int grx_bcc_phase_trace(grx_bcc *p, int max_phases, int *kind, long long *items, double *ms);
/* the canonical edges (either pointer may be NULL); returns M or a negated hipError_t; valid after init (no reference counterpart) */
int grx_bcc_edges(grx_bcc *p, int *h_src, int *h_dst);
/* the results of the last Enact; every pointer may be NULL.  Before an Enact: hipErrorNotReady (no reference counterpart) */
int grx_bcc_extract(grx_bcc *p, int *h_bcc, unsigned char *h_bridge, unsigned char *h_articulation, int *h_tecc, int *h_block_size);
/* any pointer may be NULL: the blocks, the bridges, the articulation points, the edges of the largest block and its id (ties go to
 * the smaller id; -1 without an edge), the 2-edge-connected components (single vertices counted), the vertices of the largest one
 * and its root (ties go to the smaller root).  Before an Enact: hipErrorNotReady (no reference counterpart) */
int grx_bcc_summary(grx_bcc *p, long long *blocks, long long *bridges, long long *articulation_points, long long *largest_block,
                    int *largest_block_id, long long *tecc_components, long long *largest_tecc, int *largest_tecc_root);
/* the first max_edges pairs of the block-cut tree into h_vertex / h_block (either NULL, or max_edges 0: none is copied); returns the
 * number of pairs, which must fit an int, or a negated hipError_t.  The pairs are built at the first call after an Enact and kept
 * on the device until the next Reset, so a count call followed by a fetch sorts once (no reference counterpart) */
int grx_bcc_block_cut(grx_bcc *p, int max_edges, int *h_vertex, int *h_block);
/* device arrays of the handle (no reference counterpart): bcc (M int32), tecc (`nodes` int32), the two masks (M and `nodes` uint8),
 * the canonical edges (M int32 each) and the spanning forest: parent (-1 at a root and at a vertex without a neighbour) and level
 * (`nodes` int32 each).  The forest is not unique: which neighbour of the level above is the parent depends on the run */
int grx_bcc_device_results(grx_bcc *p, int **d_bcc, int **d_tecc, unsigned char **d_bridge, unsigned char **d_articulation, int **d_src,
                           int **d_dst, int **d_parent, int **d_level);
void grx_bcc_destroy(grx_bcc *p);

/* ------------------------------------------------------------------------------------------------
 * Maximum flow and minimum cut: MaxflowProblem + MaxflowEnactor in app/maxflow/{maxflow_problem,maxflow_enactor,maxflow_functor}.hpp
 * (push-relabel: Goldberg and Tarjan, J. ACM 1988, with the global relabelling of Cherkassky and Goldberg, Algorithmica 1997; the
 * reference snapshot has no counterpart, later Gunrock releases ship `mf`).  The CSR is read as a directed multigraph with int32
 * capacities (NULL: 1 each): rows may be unsorted, self-loops are ignored, parallel arcs u -> v add up, u -> v and v -> u are
 * different arcs, so a symmetric CSR is an undirected network.  The M canonical pairs are the distinct {a < b} with an arc in either
 * direction (capacity 0 included), sorted by (a, b); pair p has cap_ab[p] and cap_ba[p], each the 64-bit sum of its direction, and
 * every per-pair array is indexed by p.  The results of Enact for (src, sink):
 *   value       the maximum flow (int64)
 *   side[v]     0: v is reachable from src in the residual graph of the final flow; 2: sink is reachable from v; 1: neither (uint8,
 *               `nodes` entries).  The sets 0 and 2 are the smallest and the largest source side of a minimum cut: one value each
 *   cut[p]      bit 0: positive capacity from a side-0 end to an end that is not side 0; bit 1: positive capacity from an end that
 *               is not side 2 to a side-2 end (uint8, M entries).  The capacities under either bit sum to value
 *   flow[p]     the net flow a -> b (negative: b -> a), -cap_ba[p] <= flow[p] <= cap_ab[p], conserved at every vertex but src and
 *               sink (int32, M entries).  Not unique: it depends on the run.  It is a valid maximum flow every time
 *   arc_flow[e] per CSR entry: a pair's net flow in a direction goes to that direction's entries in CSR order, each filled to its
 *               capacity before the next; entries of the other direction and self-loops get 0 (int32).  A function of flow[] and
 *               the input
 *   summary     value, the sizes of side 0, side 1 and side 2, the pairs with cut bit 0, the pairs with cut bit 1
 * Init builds the residual graph (a symmetric CSR over the pairs with the reverse entry on every entry); Enact runs the preflow
 * phase, the return phase and the cut, and reports only a flow it has certified on the device: no excess outside src and sink, and
 * sink not reachable from src.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_maxflow grx_maxflow;
enum { GRX_MAXFLOW_AUTO = 0, GRX_MAXFLOW_ROUNDS = 1, GRX_MAXFLOW_DEVICE_LOOP = 2 };
enum { GRX_MAXFLOW_PHASE_PREFLOW = 0, GRX_MAXFLOW_PHASE_RETURN = 1, GRX_MAXFLOW_PHASE_CUT = 2 }; /* the kinds of grx_maxflow_phase_trace */
enum { GRX_MAXFLOW_GAVE_UP = -4 }; /* grx_maxflow_enact: more than "max_rounds" rounds; next to -1 / -2 / -3 */

/* (no counterpart in the reference snapshot: this call and the ones below are shaped like grx_bcc_*) */
int grx_maxflow_create(grx_maxflow **out, int instrument, int device);
/* MaxflowProblem::Init: validates the CSR and builds the pairs and the residual graph on the device (no counterpart in the reference
 * snapshot).  -1: nodes < 1, nodes > 2^30, edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices, a negative capacity, or a
 * pair with cap_ab + cap_ba > 2^31 - 1 (one int32 residual per direction holds the whole pair); -3: the handle has been given a
 * graph before (accepted or rejected) */
int grx_maxflow_init(grx_maxflow *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *capacities);
/* the same for a CSR already in HBM (borrowed, not freed: it must outlive the handle, grx_maxflow_arc_flow reads it; no counterpart
 * in the reference snapshot) */
int grx_maxflow_init_device(grx_maxflow *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_capacities);
/* 0: set; 1: unknown name; -1: a value out of range (no counterpart in the reference snapshot).  No option changes a unique result.
 *   "schedule"          GRX_MAXFLOW_AUTO (default): a stretch of narrow steps (rounds, search levels) is one loop launch on the
 *                       device, a wide step is a launch of its own; GRX_MAXFLOW_ROUNDS: every step is a launch and a read-back;
 *                       GRX_MAXFLOW_DEVICE_LOOP: every step runs in the one-workgroup loop
 *   "wave_min_row"      rows of at least this many entries are walked by a whole wave (default 16, >= 1)
 *   "discharge_steps"   pushes or relabels of one vertex per round (default 4, 1 .. 1024)
 *   "relabel_interval"  a global relabel after this many relabels, as a multiple of `nodes` (default 0.1, >= 0; 0: after every
 *                       round that relabelled; 1e18: never again after the first of a phase)
 *   "max_rounds"        Enact stops with GRX_MAXFLOW_GAVE_UP behind this many rounds (default 4000000, 1 .. 2^30)
 *   "loop_max_list"     under AUTO the device loop takes a step of at most this many vertices (default 32768, not tuned)
 *   "loop_max_entries"  ... whose rows hold at most this many entries (default 8192, not tuned) */
int grx_maxflow_set_option(grx_maxflow *p, const char *name, double value);
/* MaxflowProblem::Reset (no counterpart in the reference snapshot): the residuals back at the capacities, excess and heights cleared.
 * -1: src or sink outside [0, nodes), or src == sink */
int grx_maxflow_reset(grx_maxflow *p, int src, int sink);
/* MaxflowEnactor::Enact(problem, max_grid_size), HIP-event timed (no counterpart in the reference snapshot).  Without a Reset since
 * the last Enact it resets to the last pair; before any Reset: hipErrorNotReady.  GRX_MAXFLOW_GAVE_UP: the rounds passed
 * "max_rounds" (or the certificate failed 64 times); the handle then holds no result and takes the next Reset */
int grx_maxflow_enact(grx_maxflow *p, int max_grid_size, float *elapsed_ms);
/* of the last Enact, any pointer may be NULL (no counterpart in the reference snapshot): M, the discharge rounds, the global
 * relabels, pushes and relabels (both depend on the schedule), row entries walked, kernel launches, host read-backs and -- when
 * instrumented -- the summed kernel time; build_ms: the HIP-event time of Init's build.  The one-thread launches that stamp the
 * phase trace and the memsets of an Enact are in neither kernel_launches nor kernel_ms */
int grx_maxflow_stats(grx_maxflow *p, long long *pairs, long long *rounds, long long *global_relabels, long long *pushes, long long *relabels,
                      long long *entries_read, long long *kernel_launches, long long *readbacks, double *kernel_ms, double *build_ms);
/* the three phases of the last Enact in order, at most max_phases of them (no counterpart in the reference snapshot): the kind
 * (GRX_MAXFLOW_PHASE_*), the rounds it ran (the cut: its search levels) and its time by the device's constant-rate counter, both
 * summed over the trips a failed certificate caused; returns the number of phases (0 before the first Enact) */
int grx_maxflow_phase_trace(grx_maxflow *p, int max_phases, int *kind, long long *rounds, double *ms);
/* the canonical pairs and their capacities (any pointer may be NULL); returns M or a negated hipError_t; valid after init (no
 * counterpart in the reference snapshot) */
long long grx_maxflow_pairs(grx_maxflow *p, int *h_a, int *h_b, int *h_cap_ab, int *h_cap_ba);
/* the results of the last Enact; every pointer may be NULL.  Before a finished Enact: hipErrorNotReady (no counterpart in the
 * reference snapshot) */
int grx_maxflow_extract(grx_maxflow *p, long long *value, int *h_flow, unsigned char *h_side, unsigned char *h_cut);
/* arc_flow[] of the last Enact, `edges` entries, computed at the first call behind an Enact.  Before a finished Enact:
 * hipErrorNotReady (no counterpart in the reference snapshot) */
int grx_maxflow_arc_flow(grx_maxflow *p, int *h_arc_flow);
/* value, |side 0|, |side 1|, |side 2|, pairs with cut bit 0, pairs with cut bit 1.  Before a finished Enact: hipErrorNotReady (no
 * counterpart in the reference snapshot) */
int grx_maxflow_summary(grx_maxflow *p, long long out[6]);
/* device arrays of the handle (no counterpart in the reference snapshot): flow (M int32), side (`nodes` uint8), cut (M uint8), the
 * canonical pairs (M int32 each), excess (`nodes` int64: sink's is value, src's is -value) and height (`nodes` int32: the labels of
 * the return phase, not unique) */
int grx_maxflow_device_results(grx_maxflow *p, int **d_flow, unsigned char **d_side, unsigned char **d_cut, int **d_a, int **d_b,
                               long long **d_excess, int **d_height);
void grx_maxflow_destroy(grx_maxflow *p);

/* ------------------------------------------------------------------------------------------------
 * Heavy-edge matching and graph contraction: MatchingProblem + MatchingEnactor in
 * app/matching/{matching_problem,matching_enactor,matching_functor}.hpp (the locally dominant matching: Preis, STACS 1999; Manne and
 * Bisseling, PPAM 2007; the reference snapshot has no counterpart).  One level of multilevel coarsening.  The CSR is read as an
 * undirected simple graph, as grx_bcc_* and grx_truss_* read it: either row may hold the edge, self-loops are ignored, rows may be
 * unsorted and hold duplicates.  The M canonical pairs {a < b} are sorted by (a, b) and every per-pair array is indexed by that
 * order.  `weights` is an int32 per CSR entry (any value) or NULL, which means 1 each; the weight w(i) of pair i is the largest of
 * its entries in both directions.  Pairs are strictly ordered by
 *     key(i) = ((uint32)w(i) ^ 0x80000000) << 32 | fmix32((uint32)i + seed * 0x9E3779B9)       (uint64; fmix32 of grx_mis_*)
 * and in_matching[i] = 1 iff no pair j that shares an end with i and has key(j) > key(i) has in_matching[j] = 1.  That equation has
 * one solution: the matching the greedy pass over the pairs in descending key order writes.  It is maximal, and its weight is at
 * least half of the maximum weight matching's.  The results of Enact:
 *   in_matching[i]  uint8, M entries
 *   mate[v]         the other end of v's pair, -1: unmatched (int32, `nodes` entries)
 *   medge[v]        the canonical index of v's pair, -1: unmatched (int32, `nodes` entries)
 *   summary         M, the matched pairs, their total weight (int64), the unmatched vertices, those of them with a neighbour
 * Contract builds the coarse graph of the last Enact: rep(v) = min(v, mate[v]) (v when unmatched), map[v] = the rank of rep(v) among
 * the representatives ascending, vweight[c] = the sum of the cluster's vertex weights, a coarse pair {map[a], map[b]} for every fine
 * pair with map[a] != map[b], its weight the sum of the w(i) that fall on it; it comes out as a mirrored CSR with ascending rows and
 * the pair's weight on both copies, which a next handle reads back unchanged.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_matching grx_matching;
enum { GRX_MATCHING_AUTO = 0, GRX_MATCHING_ROUNDS = 1, GRX_MATCHING_DEVICE_LOOP = 2 };
enum { GRX_MATCHING_STEP_WIDE = 0, GRX_MATCHING_STEP_LOOP = 1 }; /* the kinds of grx_matching_round_trace */
enum { GRX_MATCHING_GAVE_UP = -4, GRX_MATCHING_OVERFLOW = -5 };  /* next to -1 / -2 / -3 */
enum { GRX_BC_OVERFLOW = -6 };  /* grx_bc_run: a source's shortest-path counts do not fit float32 */

/* (no counterpart in the reference snapshot: this call and the ones below are shaped like grx_maxflow_*) */
int grx_matching_create(grx_matching **out, int instrument, int device);
/* MatchingProblem::Init: validates the CSR and builds the pairs, their weights and the neighbour CSR on the device.  -1: nodes < 1,
 * edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices; -3: the handle has been given a graph before (accepted or rejected) */
int grx_matching_init(grx_matching *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *weights, unsigned seed);
/* the same for a CSR (and weights, or NULL) already in HBM: borrowed, not freed, read by the build only */
int grx_matching_init_device(grx_matching *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_weights, unsigned seed);
/* 0: set; 1: unknown name; -1: a value out of range.  No option changes a result.
 *   "schedule"          GRX_MATCHING_AUTO (default): a stretch of narrow rounds is one loop launch on the device, a wide round is a
 *                       launch pair of its own; GRX_MATCHING_ROUNDS: every round is a launch pair and a read-back;
 *                       GRX_MATCHING_DEVICE_LOOP: every round runs in the one-workgroup loop
 *   "wave_min_row"      rows with at least this many entries left are walked by a whole wave (default 16, >= 1)
 *   "max_rounds"        Enact stops with GRX_MATCHING_GAVE_UP behind this many rounds (default 0: nodes / 2 + 1, which no run
 *                       passes; 0 .. 2^31)
 *   "loop_max_list"     under AUTO the device loop takes a round of at most this many vertices (default 32768, not tuned)
 *   "loop_max_entries"  ... whose rows hold at most this many entries (default 65536, not tuned) */
int grx_matching_set_option(grx_matching *p, const char *name, double value);
/* MatchingProblem::Reset: nobody matched, every vertex with a neighbour live; the coarse graph of a Contract is freed */
int grx_matching_reset(grx_matching *p);
/* MatchingEnactor::Enact(problem, max_grid_size), HIP-event timed.  Without a Reset since the last Enact it resets itself.
 * GRX_MATCHING_GAVE_UP: the rounds passed "max_rounds"; the handle then holds no result and takes the next Reset */
int grx_matching_enact(grx_matching *p, int max_grid_size, float *elapsed_ms);
/* of the last Enact, any pointer may be NULL: M, the rounds that matched a pair (the round count of the mutual-best form of the
 * definition; the closing round that only retires vertices is not in it), the rounds run inside the device loop, row entries
 * walked, one-entry polls, kernel launches and -- when instrumented -- the summed kernel time; build_ms: the HIP-event time of
 * Init's build */
int grx_matching_stats(grx_matching *p, long long *pairs, long long *rounds, long long *loop_rounds, long long *entries_read, long long *polls,
                       long long *kernel_launches, double *kernel_ms, double *build_ms);
/* the host's steps of the last Enact in order, at most max_steps of them: the kind (GRX_MATCHING_STEP_*), the rounds it ran (1 for a
 * wide round), the live list it started from and the pairs it matched; returns the number of steps (0 before the first Enact) */
int grx_matching_round_trace(grx_matching *p, int max_steps, int *kind, long long *rounds, long long *list, long long *matched);
/* the canonical pairs and their weights (any pointer may be NULL); returns M or a negated hipError_t; valid after init */
long long grx_matching_pairs(grx_matching *p, int *h_src, int *h_dst, int *h_weight);
/* the results of the last Enact; every pointer may be NULL.  Before a finished Enact: hipErrorNotReady */
int grx_matching_extract(grx_matching *p, unsigned char *h_in_matching, int *h_mate, int *h_medge);
/* M, matched pairs, their total weight, unmatched vertices, unmatched vertices of degree > 0.  Before a finished Enact:
 * hipErrorNotReady */
int grx_matching_summary(grx_matching *p, long long out[5]);
/* device arrays of the handle: in_matching (M uint8), mate and medge (`nodes` int32), the canonical pairs and their weights (M
 * int32 each) */
int grx_matching_device_results(grx_matching *p, unsigned char **d_in_matching, int **d_mate, int **d_medge, int **d_src, int **d_dst,
                                int **d_weight);
/* the coarse graph of the last Enact, built on the device and kept until the next Reset or Contract.  vertex_weights: `nodes` int32
 * in host or device memory, or NULL (1 each).  -1: no finished Enact; GRX_MATCHING_OVERFLOW: a coarse pair weight or vertex weight
 * is outside int32 (nothing is kept, nothing is wrapped).  *coarse_entries is twice the coarse pairs */
int grx_matching_contract(grx_matching *p, const int *vertex_weights, long long *coarse_nodes, long long *coarse_entries);
/* map (`nodes`), the coarse CSR (coarse_nodes + 1 offsets, coarse_entries columns and weights) and vweight (coarse_nodes), all int32;
 * every pointer may be NULL.  Without a Contract: hipErrorNotReady */
int grx_matching_coarse_extract(grx_matching *p, int *h_map, int *h_row_offsets, int *h_col_indices, int *h_weights, int *h_vweight);
/* the same arrays on the device, for grx_matching_init_device of the next level (they live until this handle's next Reset,
 * Contract or destroy).  Without a Contract: hipErrorNotReady and NULLs */
int grx_matching_coarse_device(grx_matching *p, int **d_map, int **d_row_offsets, int **d_col_indices, int **d_weights, int **d_vweight);
void grx_matching_destroy(grx_matching *p);

/* ------------------------------------------------------------------------------------------------
 * CLIQUE: CliqueProblem + CliqueEnactor: k-clique counts for k = 3 .. 6 (no counterpart in the reference snapshot).  The CSR is
 * read exactly as grx_tc_* / grx_kcore_* read it, as the simple undirected graph G: u and v are neighbours when either row holds the
 * other, self-loops are ignored, rows may be unsorted and may hold duplicates and one-way entries.  Every result has one value:
 *   cliques[v]  the number of k-cliques of G that contain v (int64, `nodes` entries)
 *   total       the number of k-cliques of G (int64); sum(cliques) = k * total
 * For k = 3 both are byte-identical to grx_tc_*'s triangles[] and total.  Init orients every edge from the end with the smaller
 * (rank[v], d(v), v) to the larger; every clique is then found once, at its smallest member u, inside N+(u).  `rank` is an int32
 * per vertex or NULL (all equal: TC's (d, id) orientation, no out-row beyond floor(sqrt(2 M))).  Among vertices of one rank those
 * go first that a peel lets go: a vertex leaves once at most max(rank, 0) neighbours of its own or a higher rank are left; the rest
 * follow by (d, id).  With grx_kcore_*'s core numbers as the rank that is the degeneracy orientation: no out-row is longer than the
 * degeneracy.  No rank changes a result.  Enact counts a row of up to "bitmap_rows" entries as nested ANDs and popcounts of the bit
 * matrix of N+(u) in LDS, a longer one by list intersections in global scratch.
 * Counts never wrap: Enact refuses (GRX_CLIQUE_OVERFLOW) when sum over u of C(d+(u), k - 1), a float64 computed on the device that
 * is at least `total` and every cliques[v], reaches "count_limit".
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_clique grx_clique;
enum { GRX_CLIQUE_AUTO = 0, GRX_CLIQUE_BITMAP = 1, GRX_CLIQUE_LIST = 2 };
enum { GRX_CLIQUE_OVERFLOW = -7 };  /* next to -1 / -2 / -3 */

int grx_clique_create(grx_clique **out, int instrument, int device);
/* CliqueProblem::Init: validates the CSR and builds the oriented graph on the device.  rank: `nodes` int32 or NULL.  -1: nodes < 1,
 * edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices, as grx_tc_init; -3: the handle has been given a graph before
 * (accepted or rejected) */
int grx_clique_init(grx_clique *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *rank /* or NULL */);
/* the same for a CSR (and a rank, or NULL) already in HBM: borrowed, not freed, the rank read by the build only */
int grx_clique_init_device(grx_clique *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, const int *d_rank /* or NULL */);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  None changes a result.
 *   "strategy"     GRX_CLIQUE_AUTO (default): rows up to "bitmap_rows" entries take the bitmap regime, longer ones the list regime;
 *                  GRX_CLIQUE_BITMAP / GRX_CLIQUE_LIST force that regime for every row (under GRX_CLIQUE_BITMAP a row beyond 1024
 *                  entries still takes the list regime)
 *   "bitmap_rows"  the longest row of the bitmap regime under GRX_CLIQUE_AUTO (default 512, 32 .. 1024; 512 rows take 32 KiB of LDS
 *                  for the matrix, 1024 rows 128 KiB)
 *   "count_limit"  Enact refuses when the bound reaches it (default and at most 2^62, at least 1); changes refusals only */
int grx_clique_set_option(grx_clique *p, const char *name, double value);
/* CliqueProblem::Reset: the counts to zero */
int grx_clique_reset(grx_clique *p);
/* CliqueEnactor::Enact(problem, k, max_grid_size), HIP-event timed.  -1: k outside 3 .. 6.  Without a Reset since the last Enact it
 * resets itself.  GRX_CLIQUE_OVERFLOW: the bound reached "count_limit"; no kernel ran, the handle holds no result and takes the next
 * Enact */
int grx_clique_enact(grx_clique *p, int k, int max_grid_size, float *elapsed_ms);
/* any pointer may be NULL.  Oriented edges (M) and the longest out-row of the graph; of the last Enact: the rows of at least
 * k - 1 entries (a shorter one holds no clique) and their oriented edges that the bitmap and the list regime took (regime_rows[2], regime_edges[2]), bit-row ANDs, list look-ups, the bound
 * of its k, kernel launches and -- when instrumented -- the summed kernel time; build_ms: the HIP-event time of Init's build */
int grx_clique_stats(grx_clique *p, long long *oriented_edges, long long *max_out_row, long long *regime_rows, long long *regime_edges,
                     long long *bit_ands, long long *list_lookups, double *bound, long long *kernel_launches, double *kernel_ms, double *build_ms);
/* Before a finished Enact (none yet, a Reset since, or a refused one): hipErrorNotReady */
int grx_clique_extract(grx_clique *p, long long *h_cliques /* may be NULL */, long long *total);
/* device arrays of the handle: 64-bit counts and 32-bit degrees d(v), `nodes` each */
int grx_clique_device_results(grx_clique *p, long long **d_cliques, int **d_degrees);
void grx_clique_destroy(grx_clique *p);

/* ------------------------------------------------------------------------------------------------
 * C4: C4Problem + C4Enactor: 4-cycle (butterfly) counts per vertex, per edge and in total (no counterpart in the reference
 * snapshot).  The CSR is read exactly as grx_tc_* / grx_clique_* read it, as the simple undirected graph G: u and v are neighbours
 * when either row holds the other, self-loops are ignored, rows may be unsorted and may hold duplicates and one-way entries.  A
 * 4-cycle is four distinct vertices a, b, c, d with the edges ab, bc, cd, da, counted as a subgraph (chords allowed: K_4 holds
 * three).  Every result has one value:
 *   cycles[v]       the 4-cycles through vertex v (int64, `nodes` entries)
 *   edge_cycles[e]  the 4-cycles through edge e (int64), in the canonical edge order of grx_c4_edges, which is grx_truss_edges': (a, b)
 *                   with a < b, sorted
 *   total           the 4-cycles of G (int64); sum(cycles) = sum(edge_cycles) = 4 * total
 * Init ranks the vertices by (degree, id) and renumbers the neighbour CSR by rank.  A 4-cycle is counted at its highest-ranked
 * vertex u as a pair of wedges u - v - w (v and w below u) with the same end w; W(u) is the number of wedges of u.  Enact counts a
 * start vertex in one of four regimes by W(u): by one lane, by a wave or a workgroup with an end -> count table in LDS, or by a
 * workgroup with a dense counter row in global scratch.
 * Counts never wrap: Enact refuses (GRX_C4_OVERFLOW) when sum over u of W(u) (dlow(u) - 1) / 2 (dlow: the neighbours of u below it), a
 * float64 computed on the device that is at least `total` and every single count, reaches "count_limit".
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_c4 grx_c4;
enum { GRX_C4_AUTO = 0, GRX_C4_LANE = 1, GRX_C4_WAVE = 2, GRX_C4_BLOCK = 3, GRX_C4_GLOBAL = 4 };  /* option "strategy" */
enum { GRX_C4_OVERFLOW = -7 };  /* next to -1 / -2 / -3; the value of GRX_CLIQUE_OVERFLOW */

int grx_c4_create(grx_c4 **out, int instrument, int device);
/* C4Problem::Init: validates the CSR and builds the canonical pairs and the rank-renumbered graph on the device.  -1: nodes < 1,
 * edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices, as grx_tc_init; -3: the handle has been given a graph before
 * (accepted or rejected) */
int grx_c4_init(grx_c4 *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM: borrowed, not freed, read by the build only */
int grx_c4_init_device(grx_c4 *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  None changes a count.
 *   "strategy"         GRX_C4_AUTO (default): every start vertex takes the smallest regime that holds its W; GRX_C4_LANE / _WAVE /
 *                      _BLOCK / _GLOBAL: no start vertex takes a smaller regime than this one (one whose W exceeds the forced regime's
 *                      capacity still takes the next larger one)
 *   "lane_max_wedges"  the largest W of the LANE regime (default 16, 0 .. 32)
 *   "table_slots"      slots of a wave's table, a power of two in 64 .. 1024 (default 1024); the WAVE regime holds W <= table_slots / 2
 *   "block_slots"      slots of a workgroup's table, a power of two in 256 .. 8192 (default 8192, 64 KiB of LDS); the BLOCK regime
 *                      holds W <= block_slots / 2
 *   "scratch_mib"      the GLOBAL regime runs min(grid, scratch_mib 2^20 / (4 nodes)) workgroups, at least 1, each with a counter row
 *                      of `nodes` int32 in global scratch (default 1024, 1 .. 65536)
 *   "edges"            1 (default): edge_cycles[] is counted too; 0: it is neither counted nor allocated
 *   "count_limit"      Enact refuses when the bound reaches it (default and at most 2^62, at least 1); changes refusals only */
int grx_c4_set_option(grx_c4 *p, const char *name, double value);
/* C4Problem::Reset: the counts to zero */
int grx_c4_reset(grx_c4 *p);
/* C4Enactor::Enact(problem, max_grid_size), HIP-event timed.  Without a Reset since the last Enact it resets itself.
 * GRX_C4_OVERFLOW: the bound reached "count_limit"; no kernel ran, the handle holds no result and takes the next Enact */
int grx_c4_enact(grx_c4 *p, int max_grid_size, float *elapsed_ms);
/* any pointer may be NULL.  The edges (M) and the wedges (the sum of W) of the graph; of the last Enact: the start vertices (W >= 2)
 * and their wedges per regime (regime_vertices[4], regime_wedges[4]: lane, wave, workgroup, global), the table probes of the wave and
 * workgroup regimes, kernel launches and -- when instrumented -- the summed kernel time; the bound; build_ms: the HIP-event time of
 * Init's build */
int grx_c4_stats(grx_c4 *p, long long *simple_edges, long long *wedges, long long *regime_vertices, long long *regime_wedges, long long *table_probes,
                 double *bound, long long *kernel_launches, double *kernel_ms, double *build_ms);
/* Before a finished Enact (none yet, a Reset since, or a refused one): hipErrorNotReady */
int grx_c4_extract(grx_c4 *p, long long *h_cycles /* may be NULL */, long long *total);
/* the canonical edges after Init: M int32 each, either may be NULL; returns M, or -(hipError_t) */
int grx_c4_edges(grx_c4 *p, int *h_src, int *h_dst);
/* M int64.  Before a finished Enact: hipErrorNotReady; -1 when that Enact ran with "edges" = 0 */
int grx_c4_extract_edges(grx_c4 *p, long long *h_edge_cycles);
/* device arrays of the handle: cycles (`nodes` int64), edge_cycles (M int64; NULL unless the last Enact finished with "edges" = 1),
 * the canonical pairs (M int32 each; NULL without an edge) */
int grx_c4_device_results(grx_c4 *p, long long **d_cycles, long long **d_edge_cycles, int **d_src, int **d_dst);
void grx_c4_destroy(grx_c4 *p);

/* ------------------------------------------------------------------------------------------------
 * RW: RwProblem + RwEnactor: random walks -- uniform, weighted and node2vec-biased (no counterpart in the reference snapshot).
 * Every draw is a fixed hash of (seed, walk, step, try) and every choice is exact integer arithmetic on it, so every output is an
 * integer with one value, whatever the grid, the strategy or the schedule.
 *   Graph.  The CSR is taken as given: directed, with self-loops and duplicate entries kept (a duplicate arc is twice as likely).
 *   Weights are optional, int32, >= 0.  Init builds its own device copy with every row sorted by (column, weight) and an inclusive
 *   int64 prefix sum of the weights per row.  All choices index the SORTED row: the walks do not depend on the order of the entries
 *   within a row.
 *   Draw(seed, walk, step, t) = Mix(seed ^ Mix((walk << 32) | (step << 8) | t)), Mix the splitmix64 finaliser
 *   (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31);
 *   walk < 2^31, step < 2^24, t < 2^8.
 *   First-order choice at vertex v with sorted row of d entries, given a draw r.  Unweighted: d == 0 ends the walk, otherwise
 *   k = ((r >> 32) * d) >> 32.  Weighted: T is the row's weight total, T == 0 ends the walk, otherwise t = (r * T) >> 64 (the full
 *   128-bit product) and k is the smallest index whose inclusive prefix exceeds t, found by bisection; zero-weight entries are never
 *   chosen.
 *   Step s of walk w (s = 0 .. length - 1), standing at v, having come from p (none at s = 0), with integer biases
 *   (b_return, b_in, b_out), each in 0 .. 65535.  First-order step, taken when the three biases are equal or at s = 0: the next
 *   vertex is the first-order choice with Draw(seed, w, s, 0).  Biased step, otherwise: amax is the largest of the three biases; for
 *   j = 0 .. tries - 1 the candidate x is the first-order choice with Draw(seed, w, s, 2j), its bias b is b_return if x == p, b_in
 *   if x occurs in the sorted out-row of p (bisection), else b_out, and it is accepted if
 *   ((Draw(seed, w, s, 2j + 1) >> 32) * amax) >> 32 < b.  If no try accepts, the candidate of the last try is taken.
 *   Outputs.  walks: int32, num_walks x (length + 1), row w starts with starts[w], and after a walk ends its row is filled with -1;
 *   lengths: int32 per walk, the number of vertices in the row; visits: int64 per vertex, the number of times it occurs in walks
 *   (only with "visits" = 1); steps: the total number of steps taken.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_rw grx_rw;
enum { GRX_RW_AUTO = 0, GRX_RW_LANE = 1, GRX_RW_TILE = 2 };  /* option "strategy" */

int grx_rw_create(grx_rw **out, int instrument, int device);
/* RwProblem::Init: validates the CSR and builds the sorted copy on the device.  weights may be NULL.  -1: nodes < 1, edges < 0 or a
 * NULL array; -2: offsets or columns that are not a CSR of `nodes` vertices, or a negative weight; -3: the handle took a graph */
int grx_rw_init(grx_rw *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *weights);
/* the same for a CSR (and weights, or NULL) in device memory: borrowed, and read only by the build */
int grx_rw_init_device(grx_rw *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_weights);
/* 0: set, 1: unknown name, -1: a value out of range
 *   "strategy"     GRX_RW_AUTO (default): by "length"; GRX_RW_LANE: every lane stores each vertex of its walk; GRX_RW_TILE: a wave
 *                  stages 64 walkers x 16 steps in LDS and writes whole 64-byte segments.  Never changes a result.
 *   "length"       0 .. 2^24 - 1 (default 0): the steps of a walk
 *   "seed"         an integer in [0, 2^53) (default 0)
 *   "weighted"     0 (default) or 1; 1 on a handle whose Init had no weights is -1
 *   "bias_return", "bias_in", "bias_out"   0 .. 65535 each (default 1)
 *   "tries"        1 .. 128 (default 32)
 *   "visits"       0 (default) or 1: Enact also counts the visits
 * "length", "seed", "weighted", the biases and "tries" define the result; nothing else changes it. */
int grx_rw_set_option(grx_rw *p, const char *name, double value);
/* RwProblem::Reset: the start vertices, one walk each.  -1: num_walks < 1, a NULL pointer or a start vertex outside 0 .. nodes - 1 */
int grx_rw_reset(grx_rw *p, int num_walks, const int *h_starts);
/* RwEnactor::Enact(problem, max_grid_size), HIP-event timed: one launch walks every walk from start to end.  max_grid_size never
 * changes a result.  Before a Reset: hipErrorNotReady */
int grx_rw_enact(grx_rw *p, int max_grid_size, float *elapsed_ms);
/* any pointer may be NULL.  Of the last Enact: its walks, the steps taken, the walks that ended early, the tries of the biased steps,
 * the biased steps no try accepted (forced fallbacks), kernel launches and -- when instrumented -- the summed kernel time; build_ms:
 * the HIP-event time of Init's build */
int grx_rw_stats(grx_rw *p, long long *walks, long long *steps, long long *ended_early, long long *biased_tries, long long *forced_fallbacks,
                 long long *kernel_launches, double *kernel_ms, double *build_ms);
/* any pointer may be NULL.  h_walks: num_walks x (length + 1) int32, dense; h_lengths: num_walks int32; h_visits: `nodes` int64.
 * Before a finished Enact: hipErrorNotReady; -1 for h_visits when the last Enact ran with "visits" = 0 */
int grx_rw_extract(grx_rw *p, int *h_walks, int *h_lengths, long long *h_visits, long long *steps);
/* device arrays of the handle after a finished Enact: walks (rows *walks_pitch entries apart, a multiple of 16, the first length + 1
 * of a row written), lengths, visits (NULL unless the last Enact ran with "visits" = 1) */
int grx_rw_device_results(grx_rw *p, int **d_walks, int **d_lengths, long long **d_visits, long long *walks_pitch);
void grx_rw_destroy(grx_rw *p);

/* ------------------------------------------------------------------------------------------------
 * SAMPLE: SampleProblem + SampleEnactor: neighbourhood sampling, multi-hop fanout subgraphs renumbered to dense local ids (no
 * counterpart in the reference snapshot).  A sample without replacement is Robert Floyd's subset algorithm over counter-based
 * draws, so every output is an integer with one value, exactly as for the walks.
 *   Graph.
 *   - The graph is taken as grx_rw_init takes it.  It is the CSR as given: directed, with self-loops and duplicate entries kept.
 *   - Weights are optional int32 >= 0.
 *   - The same -1 / -2 / -3 codes apply.
 *   - Init builds a device copy with every row sorted by (column, weight, entry).
 *   - `entry` is the index of the entry in the caller's col_indices.
 *   - For every sorted position the copy keeps that `entry`.
 *   - With weights it also keeps the inclusive int64 prefix sums per row.
 *   - Every pick indexes the SORTED row.
 *   Draw.  Draw(seed, v, hop, s) is rw's Draw(seed, walk = v, step = hop, t = s).  The function, the Python rw_draw and the limits
 *   are the same ones; s < 64 here.
 *   Picks of vertex v expanded at hop h, with sorted row of d entries and fanout f:
 *   - f = -1: the positions 0 .. d-1 in order, whatever the mode.  Weights are not consulted.
 *   - replace = 0 (unweighted only), 1 <= f <= 64:
 *     - If d <= f, the positions 0 .. d-1 in order.
 *     - Otherwise, for s = 0 .. f-1:
 *       - i = d - f + s;
 *       - t = ((Draw(seed, v, h, s) >> 32) * (i + 1)) >> 32;
 *       - pick_s = t, unless t equals an earlier pick of this row, in which case pick_s = i.
 *     - The picks are f distinct positions, in slot order.
 *   - replace = 1:
 *     - If d == 0 (weighted: the row total T == 0), there are no picks.
 *     - Otherwise there are f picks.
 *     - pick_s is rw's first-order choice with Draw(seed, v, h, s): ChooseUniform, or ChooseWeighted with option "weighted" = 1.
 *     - The picks are in slot order.
 *   Literals, computed with rw_draw:
 *   - (seed 7, v 5, hop 0, d 10, f 4) -> [2, 0, 8, 3].  This case has one collision.
 *   - (7, 5, 2, 10, 4) -> [2, 0, 7, 5].
 *   - (1, 0, 1, 9, 6) -> [2, 4, 3, 0, 7, 5].  This case has two collisions.
 *   Hops.
 *   - fanouts[0 .. H-1] with 1 <= H <= 16.
 *   - There are B >= 1 seeds.  They must be DISTINCT vertices, otherwise Reset returns -1.
 *   - The seeds take the local ids 0 .. B-1 in the given order and are frontier 0.
 *   - Hop h expands every vertex of frontier h in local-id order with fanouts[h].
 *   - A pick at position k of v's sorted row is one sampled edge with three fields:
 *     - row = local id of v;
 *     - col = the column at k;
 *     - eid = the entry kept at k.
 *   - The distinct columns that have no local id yet take the next local ids IN ASCENDING VERTEX ID.  They are frontier h+1.
 *   - A vertex is therefore expanded at most once.
 *   - An empty frontier ends the run, and the remaining hops add nothing.
 *   - Repeated picks and duplicate entries stay as parallel edges.
 *   Outputs.
 *   - vertices: int32[V], the vertex of every local id.
 *   - vertex_ptr: int64[H+2].  Local ids vertex_ptr[h] .. vertex_ptr[h+1]-1 were first reached at hop h, and hop 0 holds the seeds.
 *   - The sampled edges, as a CSR over local rows:
 *     - offsets: int64[V+1].  The rows of the last frontier are empty.
 *     - cols: int32[E], local ids.
 *     - eids: int32[E].
 *   - edge_ptr: int64[H+1].  The edges of hop h are edge_ptr[h] .. edge_ptr[h+1]-1.  This follows from the order of expansion.
 *   Only seed, replace, weighted, the fanouts and the seeds define the result.  The strategy, long_row, the grid, host or device
 *   input, and the order of entries within a row never change vertices, vertex_ptr, offsets, cols or edge_ptr.  A different entry
 *   order only changes which caller entry an eid names, by the tie rule above.
 *   Refusals.
 *   - The edge count of a hop is known before its sampler runs.
 *   - If E would exceed option "edge_limit", Enact returns GRX_SAMPLE_TOO_LARGE (-4, next to -1 / -2 / -3).
 *   - "edge_limit" defaults to 2^31 - 1, which is also its maximum; its minimum is 1.
 *   - On that refusal no further kernel runs, and the handle holds no result (hipErrorNotReady on extract).
 *   - The handle takes the next Reset / Enact normally.
 *   - replace = 0 with weighted = 1 is refused: set_option returns -1.
 *   - A fanout outside {-1, 1 .. 64} is -1, and so is H outside 1 .. 16.
 *   Explicitly out.  DESIGN.md 7 says why, in one clause each:
 *   - Weighted sampling without replacement is out.  Exponential keys are floats, so there is no one-valued integer form.
 *   - Fanouts above 64 are out.
 *   - First-occurrence local order is out, because it is schedule-dependent on a GPU.
 *   - The multi-GPU path is out.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_sample grx_sample;
enum { GRX_SAMPLE_AUTO = 0, GRX_SAMPLE_LANE = 1, GRX_SAMPLE_GROUP = 2 };  /* option "strategy" */
enum { GRX_SAMPLE_TOO_LARGE = -4 };  /* next to -1 / -2 / -3 */

int grx_sample_create(grx_sample **out, int instrument, int device);
/* SampleProblem::Init: validates the CSR and builds the sorted copy on the device.  weights may be NULL.  -1: nodes < 1, edges < 0
 * or a NULL array; -2: offsets or columns that are not a CSR of `nodes` vertices, or a negative weight; -3: the handle took a graph */
int grx_sample_init(grx_sample *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *weights);
/* the same for a CSR (and weights, or NULL) in device memory: borrowed, and read only by the build */
int grx_sample_init_device(grx_sample *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_weights);
/* 0: set, 1: unknown name, -1: a value out of range
 *   "strategy"     GRX_SAMPLE_AUTO (default): GROUP, and LANE with "replace" = 1 from 65 536 seeds on; GRX_SAMPLE_LANE: one lane per
 *                  frontier vertex runs the slots in order; GRX_SAMPLE_GROUP: g lanes per vertex, g the power of two with
 *                  f <= g <= 64.  Never changes a result.
 *   "seed"         an integer in [0, 2^53) (default 0)
 *   "replace"      0 (default) or 1; 0 while "weighted" is 1 is -1
 *   "weighted"     0 (default) or 1; 1 while "replace" is 0, or on a handle whose Init had no weights, is -1
 *   "edge_limit"   1 .. 2^31 - 1 (default 2^31 - 1): the sampled edges an Enact may hold
 *   "long_row"     at least 8 (default 4096): under a fanout of -1, longer rows are copied by workgroups.  Never changes a result.
 *   "eids"         1 (default) or 0: the entries are neither gathered nor allocated */
int grx_sample_set_option(grx_sample *p, const char *name, double value);
/* the fanout of every hop.  -1: hops outside 1 .. 16, a NULL list or a fanout outside {-1, 1 .. 64}; the list before stays */
int grx_sample_set_fanouts(grx_sample *p, int hops, const int *fanouts);
/* SampleProblem::Reset: the seeds.  -1: num_seeds < 1, a NULL pointer, a seed outside 0 .. nodes - 1 or two equal seeds */
int grx_sample_reset(grx_sample *p, int num_seeds, const int *h_seeds);
/* SampleEnactor::Enact(problem, max_grid_size), HIP-event timed: a host loop over the hops, one read-back each and one for the seeds'
 * own count.  max_grid_size never changes a result.  Before a Reset or set_fanouts: hipErrorNotReady.  GRX_SAMPLE_TOO_LARGE: a hop
 * would have passed "edge_limit"; its sampler did not run, the handle holds no result and takes the next Reset / Enact */
int grx_sample_enact(grx_sample *p, int max_grid_size, float *elapsed_ms);
/* any pointer may be NULL.  Of the last Enact: *hops = H; per hop (arrays of H) the rows expanded, the rows whose picks were drawn
 * (replace = 0: d > f) and the rows copied whole; the rows a fanout of -1 left to the long-row kernel; kernel launches, read-backs
 * and -- when instrumented -- the summed kernel time and its four parts phase_ms[4]: count + scan, sample, renumber, relabel;
 * build_ms: the HIP-event time of Init's build */
int grx_sample_stats(grx_sample *p, int *hops, long long *rows_expanded, long long *rows_sampled, long long *rows_copied, long long *long_rows,
                     long long *kernel_launches, long long *readbacks, double *kernel_ms, double *phase_ms, double *build_ms);
/* any pointer may be NULL.  V, E, vertex_ptr (H + 2 int64) and edge_ptr (H + 1 int64).  Before a finished Enact: hipErrorNotReady */
int grx_sample_sizes(grx_sample *p, long long *vertices, long long *edges, long long *vertex_ptr, long long *edge_ptr);
/* any pointer may be NULL.  h_vertices: V int32; h_offsets: V + 1 int64; h_cols, h_eids: E int32.  Before a finished Enact:
 * hipErrorNotReady; -1 for h_eids when the last Enact ran with "eids" = 0 */
int grx_sample_extract(grx_sample *p, int *h_vertices, long long *h_offsets, int *h_cols, int *h_eids);
/* device arrays of the handle after a finished Enact (NULL before; cols and eids NULL without an edge, eids NULL with "eids" = 0).
 * They stay valid until the next Reset or Enact */
int grx_sample_device_results(grx_sample *p, int **d_vertices, long long **d_offsets, int **d_cols, int **d_eids);
void grx_sample_destroy(grx_sample *p);

/* ------------------------------------------------------------------------------------------------
 * SIM: SimProblem + SimEnactor: vertex similarity by neighbourhoods -- the score of given pairs, and the k most similar vertices of
 * given sources (no counterpart in the reference snapshot).  The CSR is read exactly as grx_tc_* / grx_c4_* read it, as the simple
 * undirected graph G: u and v are neighbours when either row holds the other, self-loops are ignored, rows may be unsorted and may hold
 * duplicates and one-way entries.  d(v) is the degree in G, c(u, v) = |N(u) ^ N(v)| the common neighbours (c(u, u) = d(u)).  Every
 * metric is an exact fraction num / den:
 *   GRX_SIM_COMMON    c / 1
 *   GRX_SIM_JACCARD   c / (d(u) + d(v) - c)
 *   GRX_SIM_OVERLAP   c / min(d(u), d(v))
 *   GRX_SIM_SORENSEN  2 c / (d(u) + d(v))
 * den = 0 happens only with an isolated endpoint and reports num = 0, den = 0, score = 0.0.  num and den are int64 (on the device they
 * are sums of int32 degrees: the graph has at most INT_MAX / 2 edges); score is float64, the one IEEE division num / den, taken on the
 * host by the extract calls from the two integer arrays (the device holds no score).  Every output has one value, whatever the
 * strategy, the thresholds, the grid or the scratch budget.
 *   Pair mode: P >= 0 pairs (u[i], v[i]) in any order; repeats, u == v, adjacent and non-adjacent pairs allowed.  Per pair: common
 *   (int32), num, den, score.
 *   Top-k mode: S >= 0 sources (repeats allowed, every row independent) and k in 1 .. GRX_SIM_MAX_K.  The candidates of u are the
 *   vertices w != u with c(u, w) >= 1; with "skip_neighbors" those in N(u) are no candidates.  They are ranked by score descending, then
 *   by id ascending; scores are compared as num den' against num' den in 64-bit integers.  Per source a row of k: ids (int32, -1
 *   beyond the end), common, num, den, score (0 beyond the end); count[s] = min(k, candidates) and candidates[s], the number before
 *   the cut.
 * An id outside [0, nodes) is a bad argument (-1): it is found on the device before a kernel writes a result, and the handle stays
 * usable.  Init builds the neighbour CSR of G (rows ascending) and Wd(u) = the sum of d(v) over v in N(u), the wedges a top-k of u walks.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_sim grx_sim;
enum { GRX_SIM_AUTO = 0, GRX_SIM_LANE = 1, GRX_SIM_WAVE = 2, GRX_SIM_BLOCK = 3, GRX_SIM_GLOBAL = 4 };  /* option "strategy" */
enum { GRX_SIM_COMMON = 0, GRX_SIM_JACCARD = 1, GRX_SIM_OVERLAP = 2, GRX_SIM_SORENSEN = 3 };         /* option "metric" */
enum { GRX_SIM_MAX_K = 64 };
enum { GRX_SIM_TOO_LARGE = -4 };  /* next to -1 / -2 / -3; the value of GRX_SAMPLE_TOO_LARGE */

int grx_sim_create(grx_sim **out, int instrument, int device);
/* SimProblem::Init: validates the CSR and builds the neighbour CSR of G and Wd on the device.  -1: nodes < 1, edges < 0 or a NULL
 * array; -2: not a CSR of `nodes` vertices, as grx_tc_init; -3: the handle has been given a graph before (accepted or rejected) */
int grx_sim_init(grx_sim *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM: borrowed, not freed, read by the build only */
int grx_sim_init_device(grx_sim *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  Only "metric" and "skip_neighbors" change a
 * result.
 *   "metric"          GRX_SIM_COMMON / _JACCARD (default) / _OVERLAP / _SORENSEN
 *   "skip_neighbors"  1: top-k mode takes no candidate from N(u), the link-prediction form; 0 (default)
 *   "strategy"        GRX_SIM_AUTO (default): every pair and every source takes the smallest regime that holds it; GRX_SIM_LANE / _WAVE /
 *                     _BLOCK / _GLOBAL: nothing takes a smaller regime than this one.  Pair mode has the regimes LANE and WAVE (a
 *                     forced BLOCK or GLOBAL is WAVE there), top-k mode WAVE, BLOCK and GLOBAL (AUTO and LANE are its WAVE)
 *   "lane_max"        pair mode: a pair with d(u) + d(v) <= lane_max is one lane's two-pointer merge, a longer one the whole wave's
 *                     bisection (default 64, 0 .. 2^20)
 *   "table_slots"     slots of a wave's table, a power of two in 64 .. 1024 (default 1024); the WAVE regime holds Wd <= table_slots / 2
 *   "block_slots"     slots of a workgroup's table, a power of two in 256 .. 8192 (default 8192, 64 KiB of LDS); the BLOCK regime
 *                     holds Wd <= block_slots / 2
 *   "scratch_mib"     the GLOBAL regime runs min(grid, scratch_mib 2^20 / (4 nodes)) workgroups, at least 1, each with a counter row
 *                     of `nodes` int32 in global scratch (default 1024, 1 .. 65536) */
int grx_sim_set_option(grx_sim *p, const char *name, double value);
/* SimProblem::Reset: the handle holds no result and its counters are zero; the graph stays */
int grx_sim_reset(grx_sim *p);
/* SimEnactor::EnactPairs, HIP-event timed: h_u, h_v are num_pairs int32 each on the host (NULL allowed with num_pairs = 0).  -1: a
 * negative count, a NULL array or an id outside [0, nodes); GRX_SIM_TOO_LARGE: num_pairs > INT_MAX.  After either the handle holds no
 * pair result and takes the next call.  The top-k result of the handle, if any, stays */
int grx_sim_pairs(grx_sim *p, long long num_pairs, const int *h_u, const int *h_v, int max_grid_size, float *elapsed_ms);
/* the same for arrays in HBM: borrowed, read by this call only */
int grx_sim_pairs_device(grx_sim *p, long long num_pairs, const int *d_u, const int *d_v, int max_grid_size, float *elapsed_ms);
/* SimEnactor::EnactTopk, HIP-event timed: h_sources are num_sources int32 on the host.  -1: a negative count, a NULL array, k outside
 * 1 .. GRX_SIM_MAX_K or an id outside [0, nodes); GRX_SIM_TOO_LARGE: num_sources k > INT_MAX.  After either the handle holds no top-k
 * result and takes the next call.  The pair result of the handle, if any, stays */
int grx_sim_topk(grx_sim *p, long long num_sources, const int *h_sources, int k, int max_grid_size, float *elapsed_ms);
int grx_sim_topk_device(grx_sim *p, long long num_sources, const int *d_sources, int k, int max_grid_size, float *elapsed_ms);
/* any pointer may be NULL.  The edges (M) and the wedges (the sum of Wd) of the graph; of the last Enact: the wedges walked (the sum of
 * Wd over the sources), the pairs of the regimes lane and wave (regime_pairs[2]), the sources and their wedges of the regimes wave,
 * workgroup and global (regime_sources[3], regime_wedges[3]), the candidates of all sources, the table probes of the wave and workgroup
 * regimes (not reproducible to the last digit: a probe sequence depends on who claimed a slot first), kernel launches and -- when
 * instrumented -- the summed kernel time; build_ms: the HIP-event time of Init's build */
int grx_sim_stats(grx_sim *p, long long *simple_edges, long long *wedges, long long *wedges_walked, long long *regime_pairs, long long *regime_sources,
                  long long *regime_wedges, long long *candidates, long long *table_probes, long long *kernel_launches, double *kernel_ms,
                  double *build_ms);
/* any pointer may be NULL; num_pairs entries each.  Before a finished pair Enact (none yet, a Reset since, or a refused one):
 * hipErrorNotReady */
int grx_sim_extract_pairs(grx_sim *p, int *h_common, long long *h_num, long long *h_den, double *h_score);
/* any pointer may be NULL; h_ids .. h_score: num_sources x k entries, row s at s k; h_count, h_candidates: num_sources.  Before a
 * finished top-k Enact: hipErrorNotReady */
int grx_sim_extract_topk(grx_sim *p, int *h_ids, int *h_common, long long *h_num, long long *h_den, double *h_score, int *h_count, int *h_candidates);
/* device arrays of the handle (integers only), NULL without a finished Enact of their mode or with an empty query.  They stay valid
 * until the next Enact of their mode */
int grx_sim_device_results(grx_sim *p, int **d_pair_common, long long **d_pair_num, long long **d_pair_den, int **d_ids, int **d_common,
                           long long **d_num, long long **d_den, int **d_count, int **d_candidates);
void grx_sim_destroy(grx_sim *p);

/* ------------------------------------------------------------------------------------------------
 * SPGEMM: SpgemmProblem + SpgemmEnactor: the sparse matrix product C = A B with exact int64 values (no counterpart in the
 * reference snapshot).  A is rows x inner, B is inner x cols, both CSR read as given: duplicate entries add, a row may come in any
 * order, self-loops are ordinary entries.  Values are int32, or absent (NULL), which means 1 each.
 * C is rows x cols CSR: offsets int32[rows + 1], cols int32[nnz] strictly ascending inside a row, vals int64[nnz].  C is
 * structural (the GraphBLAS rule): entry (i, j) exists exactly when some k has A(i, k) and B(k, j) stored, also when the products
 * cancel to 0 -- then the stored value is 0.  With the option "pattern_only" the offsets and cols alone are produced; they equal
 * those of the numeric run.  Integer sums commute: every output has one value, whatever the schedule or the order of the rows.
 * The right operand, option "right":
 *   GRX_SPGEMM_SELF       (default) B = A; rows == inner is required
 *   GRX_SPGEMM_TRANSPOSE  B = A^T, built on the device at the first Enact that asks for it and kept
 *   GRX_SPGEMM_GIVEN      B from grx_spgemm_set_right / _set_right_device (calling either selects this mode)
 * Refusals, before any array of the result is written; after either the handle holds no result and takes the next call:
 *   GRX_SPGEMM_TOO_LARGE  nnz(C) or the products of one row, sum over k in A[i] of len(B[k]), are beyond INT_MAX
 *   GRX_SPGEMM_OVERFLOW   the bound max over i of (sum over k in A[i] of |a_ik| times the sum over j of |b_kj|), computed on the
 *                         device in saturating int64, reached the option "count_limit"
 * The library returns integers only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_spgemm grx_spgemm;
enum { GRX_SPGEMM_AUTO = 0, GRX_SPGEMM_LANE = 1, GRX_SPGEMM_WAVE = 2, GRX_SPGEMM_BLOCK = 3, GRX_SPGEMM_GLOBAL = 4 }; /* option "strategy" */
enum { GRX_SPGEMM_SELF = 0, GRX_SPGEMM_TRANSPOSE = 1, GRX_SPGEMM_GIVEN = 2 };                                        /* option "right" */
enum { GRX_SPGEMM_TOO_LARGE = -4 };  /* next to -1 / -2 / -3; the value of GRX_SIM_TOO_LARGE */
enum { GRX_SPGEMM_OVERFLOW = -7 };   /* the value of GRX_C4_OVERFLOW */
/* instrument != 0: every kernel is timed with HIP events (and waited for) */
int grx_spgemm_create(grx_spgemm **out, int instrument, int device);
/* A: rows >= 0, inner >= 0, nnz >= 0; vals may be NULL.  One per handle (-3 for a second one).  -1: a bad argument; -2: offsets or
 * cols are not a CSR of that shape (checked on the device) */
int grx_spgemm_init(grx_spgemm *p, int rows, int inner, int nnz, const int *offsets, const int *cols, const int *vals);
/* the same for arrays in device memory, which stay the caller's and must outlive the handle's Enacts */
int grx_spgemm_init_device(grx_spgemm *p, int rows, int inner, int nnz, int *d_offsets, int *d_cols, int *d_vals);
/* B: rows x cols with nnz entries, vals may be NULL; selects GRX_SPGEMM_GIVEN.  May be called again with another B.  -1: a bad
 * argument or rows != A's inner; -2: not a CSR of that shape (the handle then has no right operand); before Init: hipErrorNotReady */
int grx_spgemm_set_right(grx_spgemm *p, int rows, int cols, int nnz, const int *offsets, const int *col_indices, const int *vals);
int grx_spgemm_set_right_device(grx_spgemm *p, int rows, int cols, int nnz, int *d_offsets, int *d_col_indices, int *d_vals);
/* 0: set; 1: unknown name; -1: a value out of range (the option keeps its value)
 *   "right"         GRX_SPGEMM_SELF (default) / _TRANSPOSE / _GIVEN
 *   "pattern_only"  0 (default) / 1: offsets and cols only
 *   "strategy"      GRX_SPGEMM_AUTO (default): every row takes the smallest regime that holds its products w: lane (w <= lane_max: a
 *                   sorted list in one lane's private memory), wave (w <= table_slots / 2: a table in the wave's part of LDS),
 *                   workgroup (w <= block_slots / 2: the workgroup's LDS as one table), global (a dense int64 row and a bitmap per
 *                   workgroup slot in global scratch); GRX_SPGEMM_WAVE / _BLOCK / _GLOBAL: no row takes a smaller regime
 *   "lane_max"      0 .. 64 (default 64)
 *   "table_slots"   a power of two in 64 .. 1024 (default 1024); a slot is 12 bytes of LDS (4 in a pass without values)
 *   "block_slots"   a power of two in 256 .. 8192 (default 8192: 96 KiB of the CU's 160)
 *   "scratch_mib"   1 .. 65536 (default 1024): the global regime runs min(grid, scratch_mib 2^20 / (8 cols + 8 ceil(cols / 64)))
 *                   workgroups, at least one
 *   "count_limit"   1 .. 2^62 (default 2^62): the refusal GRX_SPGEMM_OVERFLOW */
int grx_spgemm_set_option(grx_spgemm *p, const char *name, double value);
/* the handle holds no result */
int grx_spgemm_reset(grx_spgemm *p);
/* C = A B.  -1: GRX_SPGEMM_SELF on a non-square A, or GRX_SPGEMM_GIVEN without a right operand; GRX_SPGEMM_TOO_LARGE,
 * GRX_SPGEMM_OVERFLOW: see above */
int grx_spgemm_enact(grx_spgemm *p, int max_grid_size, float *elapsed_ms);
/* any pointer may be NULL.  Of the last Enact: the rows and their products of the regimes lane, wave, workgroup and global
 * (regime_rows[4], regime_products[4]), the products of all rows, nnz(C), the table probes of the wave and workgroup regimes in
 * both passes (not reproducible to the last digit: a probe sequence depends on who claimed a slot first), kernel launches (the scan
 * counts as one), read-backs, the bound held against "count_limit" and -- when instrumented -- the summed kernel time and the part of
 * it each regime's kernels took in both passes (regime_ms[4]) */
int grx_spgemm_stats(grx_spgemm *p, long long *regime_rows, long long *regime_products, long long *products, long long *nnz, long long *table_probes,
                     long long *kernel_launches, long long *readbacks, double *bound, double *kernel_ms, double *regime_ms);
/* the shape of the result; before a finished Enact (none yet, a Reset since, or a refused one): hipErrorNotReady */
int grx_spgemm_sizes(grx_spgemm *p, int *rows, int *cols, long long *nnz);
/* any pointer may be NULL; rows + 1, nnz and nnz entries.  -1: h_vals of a pattern_only result.  Before a finished Enact:
 * hipErrorNotReady */
int grx_spgemm_extract(grx_spgemm *p, int *h_offsets, int *h_cols, long long *h_vals);
/* device arrays of the handle, NULL without a finished Enact (cols, vals: also with an empty result; vals: also with
 * pattern_only).  They stay valid until the next Enact */
int grx_spgemm_device_results(grx_spgemm *p, int **d_offsets, int **d_cols, long long **d_vals);
void grx_spgemm_destroy(grx_spgemm *p);

/* ------------------------------------------------------------------------------------------------
 * LP: LpProblem + LpEnactor: label-propagation communities with integer scores and a total tie rule (no counterpart in the
 * reference snapshot).  The CSR is read exactly as grx_matching_* reads it, as the simple undirected graph G with int32 weights
 * (NULL: 1 each; a pair's weight is the largest of its entries in both directions); a pair weight below 1 is refused.  L[v] is an
 * int32 label in [0, nodes).  The vote of a vertex with a neighbour: score(l) = the sum of w(v, u) over the neighbours u with
 * L[u] = l, in 64 bits; the new label is L[v] when its score is the largest, else the smallest label of the largest score.  An
 * isolated vertex keeps its label.
 *   GRX_LP_SYNC     every round computes all new labels from the labels of the round before
 *   GRX_LP_CLASSES  a round is one sub-step per class of a proper colouring (grx_lp_set_classes), in class order; a sub-step
 *                   updates its class in place from the current labels, so a round is the sequential sweep in (class, id) order.
 *                   This mode always reaches a fixed point.
 * A vertex is visited at its turn when it has not been visited since the Reset or a neighbour's label changed since its last
 * visit; no result depends on that, the counters `visits` and `entries_read` (the rows of the visits) are defined by it.  An Enact
 * ends in one of three states, none an error: GRX_LP_CONVERGED (a round changed nothing), GRX_LP_PERIOD2 (SYNC: the labels behind
 * round r are those behind round r - 2; the result is those behind r) or GRX_LP_CAPPED ("max_rounds" rounds have run).  Every
 * result has one value; the library returns integers only.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_lp grx_lp;
enum { GRX_LP_SYNC = 0, GRX_LP_CLASSES = 1 };                                  /* option "mode" */
enum { GRX_LP_AUTO = 0, GRX_LP_LANE = 1, GRX_LP_WAVE = 2, GRX_LP_BLOCK = 3 };  /* option "strategy" */
enum { GRX_LP_CONVERGED = 0, GRX_LP_PERIOD2 = 1, GRX_LP_CAPPED = 2 };          /* `state` of grx_lp_stats */
enum { GRX_LP_BAD_CLASSES = -8 };  /* next to -1 / -2 / -3 */

int grx_lp_create(grx_lp **out, int instrument, int device);
/* LpProblem::Init: validates the CSR and builds the pairs and the neighbour CSR on the device.  weights: `edges` int32 or NULL.
 * -1: nodes < 1, edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices, or a pair weight below 1; -3: the handle has been
 * given a graph before (accepted or rejected) */
int grx_lp_init(grx_lp *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *weights /* or NULL */);
/* the same for a CSR (and weights, or NULL) already in HBM: borrowed, not freed, read by the build only */
int grx_lp_init_device(grx_lp *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, int *d_weights /* or NULL */);
/* classes: `nodes` int32 in [0, num_classes), num_classes in 1 .. nodes (else -1), a proper colouring of G.  Validated on the device
 * over the pairs: GRX_LP_BAD_CLASSES when a pair has both ends in one class; then no classes are installed (an Enact in
 * GRX_LP_CLASSES mode answers hipErrorNotReady) */
int grx_lp_set_classes(grx_lp *p, const int *classes, int num_classes);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  None changes a result.
 *   "mode"          GRX_LP_CLASSES (default) or GRX_LP_SYNC
 *   "strategy"      GRX_LP_AUTO (default): a row of up to "lane_max_row" entries is voted by one lane, one of up to "wave_max_row"
 *                   by a wave with a table in LDS, a longer one by a workgroup; GRX_LP_LANE / _WAVE / _BLOCK force one for all rows
 *   "lane_max_row"  default 16, at least 0
 *   "wave_max_row"  default 512, at least 0
 *   "table_slots"   slots of a wave's label table, a power of two in 64 .. 1024 (default 1024); a workgroup's has four times as many.
 *                   A row with more distinct labels is voted in several passes and counted in fallback_rows
 *   "max_rounds"    an Enact stops behind this many rounds (default 0: 2 * nodes + 64; at most 2^30) */
int grx_lp_set_option(grx_lp *p, const char *name, double value);
/* LpProblem::Reset: L[v] = labels[v], or v for NULL; -1: a label outside [0, nodes) */
int grx_lp_reset(grx_lp *p, const int *labels /* or NULL */);
/* LpEnactor::Enact(problem, max_grid_size), HIP-event timed.  Without a Reset since the last Enact it resets itself to L[v] = v.
 * 0 in all three end states (grx_lp_stats tells which) */
int grx_lp_enact(grx_lp *p, int max_grid_size, float *elapsed_ms);
/* any pointer may be NULL.  The pairs (M) of the graph; of the last Enact: the rounds that changed a label, the end state, visits,
 * entries_read, the visited rows per regime (regime_rows[3]: lane, wave, workgroup), the rows that needed several passes, kernel
 * launches, host read-backs (at most rounds + 2) and -- when instrumented -- the summed kernel time; build_ms: the HIP-event time
 * of Init's build */
int grx_lp_stats(grx_lp *p, long long *pairs, long long *rounds, long long *state, long long *visits, long long *entries_read, long long *regime_rows,
                 long long *fallback_rows, long long *kernel_launches, long long *readbacks, double *kernel_ms, double *build_ms);
/* per round of the last Enact, the closing one included: the vertices visited and the labels changed; copies at most max_rounds
 * entries and returns how many there are */
int grx_lp_round_trace(grx_lp *p, int max_rounds, long long *list, long long *changed);
/* labels[] and community[] (the rank of a vertex's label among the labels in use, ascending), `nodes` int32 each, either may be
 * NULL; *communities: how many labels are in use.  Before a finished Enact (none yet, or a Reset since): hipErrorNotReady */
int grx_lp_extract(grx_lp *p, int *h_labels, int *h_community, long long *communities);
/* int64 per community of the last Enact: vertices, the sum of w over the pairs with both ends inside, the sum of the weighted
 * degrees; *total_weight: the sum of w over all pairs.  Any pointer may be NULL.  Before a finished Enact: hipErrorNotReady */
int grx_lp_summary(grx_lp *p, long long *h_size, long long *h_internal, long long *h_volume, long long *total_weight);
/* device arrays of the handle: labels and community, `nodes` int32 each */
int grx_lp_device_results(grx_lp *p, int **d_labels, int **d_community);
void grx_lp_destroy(grx_lp *p);

/* ------------------------------------------------------------------------------------------------
 * WL: WlProblem + WlEnactor: colour refinement, the 1-dimensional Weisfeiler-Leman test (no counterpart in the reference
 * snapshot).  The CSR is read as given, like grx_rw_*: a row is the multiset of its entries, duplicates and self-loops count,
 * one-way entries are one-way.  The start colours are the classes of labels[] (any int32 values; NULL: one class).  A round maps
 * the colouring c to c' with c'(u) = c'(v) iff c(u) = c(v) and the multisets {c(w) : w in row(u)} and {c(w) : w in row(v)} are
 * equal; the partition is stable when a round splits nothing, and it is then the coarsest equitable partition that refines the
 * labels.  The classes are numbered 0 .. count - 1 by ascending smallest member.  Rows are grouped by a seeded hash of their
 * multiset; a certificate that compares rows exactly stands behind every result, so every output is an integer with one value.
 * An Enact ends GRX_WL_STABLE or, behind "max_rounds" rounds, GRX_WL_CAPPED; neither is an error.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_wl grx_wl;
enum { GRX_WL_AUTO = 0, GRX_WL_LANE = 1, GRX_WL_WAVE = 2, GRX_WL_BLOCK = 3 };  /* option "strategy" */
enum { GRX_WL_STABLE = 0, GRX_WL_CAPPED = 1 };                                 /* `state` of grx_wl_stats */
enum { GRX_WL_TOO_LARGE = -4, GRX_WL_NOT_CERTIFIED = -5 };                     /* grx_wl_enact, next to -1 / -2 / -3 */

int grx_wl_create(grx_wl **out, int instrument, int device);
/* WlProblem::Init: validates the CSR on the device.  -1: nodes < 1, edges < 0 or a NULL array; -2: not a CSR of `nodes` vertices;
 * -3: the handle has been given a graph before (accepted or rejected) */
int grx_wl_init(grx_wl *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM: borrowed, not freed, read by every Enact (it has to outlive the handle) */
int grx_wl_init_device(grx_wl *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  Only "max_rounds" and "history" change
 * a result.
 *   "strategy"      the signature pass: GRX_WL_AUTO (default): a row of up to "lane_max_row" entries is summed by one lane, one
 *                   of up to "wave_max_row" by a wave, a longer one by a workgroup; GRX_WL_LANE / _WAVE / _BLOCK force one
 *   "lane_max_row"  default 16, at least 0
 *   "wave_max_row"  default 4096, at least 0
 *   "max_rounds"    -1 (default): refine until stable; h >= 0 (at most 2^30): the colouring after h rounds, every round certified
 *   "history"       1: keep the colouring behind every round for grx_wl_history; asks for "max_rounds" in 1 .. 64
 *   "max_repairs"   failed certificates an Enact takes before it gives up (default 64, 0 .. 2^30)
 *   "sig_bits"      the top bits of the signature that are compared, 1 .. 128 (default 128); fewer make the certificate fail more often
 *   "seed"          of the signatures, a whole number below 2^64
 *   "table_slots", "block_slots", "scratch_mib"   the certificate's count table, as for grx_sim_set_option: a vertex whose row and
 *                   its representative's together hold w entries is compared in a wave's table while w <= table_slots / 2, in the
 *                   workgroup's while w <= block_slots / 2, else in a dense counter row of global scratch */
int grx_wl_set_option(grx_wl *p, const char *name, double value);
/* WlProblem::Reset: the start labels, `nodes` int32 of any value, or NULL for one class.  An Enact without a Reset in front starts
 * from the labels of the last one */
int grx_wl_reset(grx_wl *p, const int *labels /* or NULL */);
/* WlEnactor::Enact(problem, max_grid_size), HIP-event timed.  0 in both end states (grx_wl_stats tells which); -1: "history"
 * without "max_rounds" in 1 .. 64; GRX_WL_TOO_LARGE: the history, (max_rounds + 1) * nodes colours, is beyond int32 offsets;
 * GRX_WL_NOT_CERTIFIED: more than "max_repairs" certificates failed.  After any of the three there is no result */
int grx_wl_enact(grx_wl *p, int max_grid_size, float *elapsed_ms);
/* any pointer may be NULL.  The entries of the graph; of the last Enact: the committed rounds (each split a class), the end state,
 * the classes, the failed certificates, the certificates run, the rows of all signature passes per regime (regime_rows[3]: lane,
 * wave, workgroup), the vertices compared per rung of the certificate (rung_rows[3]: wave, workgroup, global), kernel launches,
 * host read-backs (one for the labels, one per signature pass) and -- when instrumented -- the summed kernel time */
int grx_wl_stats(grx_wl *p, long long *entries, long long *rounds, long long *state, long long *classes, long long *repairs,
                 long long *certificate_runs, long long *regime_rows, long long *rung_rows, long long *kernel_launches, long long *readbacks,
                 double *kernel_ms);
/* the classes behind the labels and behind each committed round of the last Enact (rounds + 1 entries); copies at most max_rounds
 * entries and returns how many there are */
int grx_wl_round_trace(grx_wl *p, int max_rounds, long long *classes);
/* colour[]: `nodes` int32, the dense class of every vertex; class_size[]: int64 per class; representative[]: int32 per class, its
 * smallest member; any may be NULL; *classes: how many there are.  Before a finished Enact: hipErrorNotReady */
int grx_wl_extract(grx_wl *p, int *h_colour, long long *h_class_size, int *h_representative, long long *classes);
/* the dense colouring behind round `round` (0: the labels' classes) of the last Enact with "history", and its classes; -1: no
 * such round; hipErrorNotReady: no finished Enact with "history" */
int grx_wl_history(grx_wl *p, int round, int *h_colour, long long *classes);
/* device arrays of the handle, NULL without a finished Enact: colour (`nodes` int32), class_size (int64), representative (int32) */
int grx_wl_device_results(grx_wl *p, int **d_colour, long long **d_class_size, int **d_representative);
void grx_wl_destroy(grx_wl *p);

/* ------------------------------------------------------------------------------------------------
 * BIPARTITE: BipartiteProblem + BipartiteEnactor: a maximum matching of the bipartite graph rows -- columns of a CSR pattern of
 * shape (rows, cols), and its Dulmage-Mendelsohn decomposition (no counterpart in the reference snapshot).  The pattern is read as
 * given: values there are none, duplicates and unsorted rows mean nothing, empty rows and columns and a dimension of 0 are
 * allowed.  The size of the matching (the structural rank), the horizontal / square / vertical part of every row and column and
 * König's minimum vertex cover have one value whatever the schedule; the matching itself has not, and is validated: a device pass
 * over the entries certifies it and the parts before anything is reported as maximum.  An Enact ends GRX_BIPARTITE_MAXIMUM or,
 * behind "max_phases" phases that all augmented, GRX_BIPARTITE_CAPPED (a valid matching not known to be maximum); neither is an
 * error.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_bipartite grx_bipartite;
enum { GRX_BIPARTITE_AUTO = 0, GRX_BIPARTITE_LANE = 1, GRX_BIPARTITE_WAVE = 2, GRX_BIPARTITE_BLOCK = 3 };  /* option "strategy" */
enum { GRX_BIPARTITE_HORIZONTAL = 0, GRX_BIPARTITE_SQUARE = 1, GRX_BIPARTITE_VERTICAL = 2 };               /* row_part / col_part */
enum { GRX_BIPARTITE_MAXIMUM = 0, GRX_BIPARTITE_CAPPED = 1 };                                              /* `state` of the stats */
/* next to -1 / -2 / -3: the certificate failed (no result); reset was given no matching; the call needs a maximum matching and
 * the last Enact ended GRX_BIPARTITE_CAPPED */
enum { GRX_BIPARTITE_NOT_CERTIFIED = -4, GRX_BIPARTITE_BAD_MATCHING = -5, GRX_BIPARTITE_NOT_MAXIMUM = -6 };

int grx_bipartite_create(grx_bipartite **out, int instrument, int device);
/* BipartiteProblem::Init: validates the CSR on the device and builds its transpose, once.  -1: a negative size or a NULL array
 * (col_indices may be NULL without entries); -2: not a CSR of that shape; -3: the handle has been given a matrix before */
int grx_bipartite_init(grx_bipartite *p, int rows, int cols, int entries, const int *row_offsets, const int *col_indices);
/* the same for a CSR already in HBM: borrowed, not freed, read by every Enact (it has to outlive the handle) */
int grx_bipartite_init_device(grx_bipartite *p, int rows, int cols, int entries, int *d_row_offsets, int *d_col_indices);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  None changes a pinned result.
 *   "greedy"        1 (default): every unmatched row first claims its first free column; 0: the phases start from the matching
 *                   of the last reset exactly
 *   "max_phases"    0 (default): none; h > 0: at most h phases
 *   "strategy"      how a frontier column's entries are walked: GRX_BIPARTITE_AUTO (default): fewer than "wave_min_row" (16)
 *                   entries by one lane, fewer than "block_min_row" (2048) by a wave, the others by a workgroup;
 *                   GRX_BIPARTITE_LANE / _WAVE / _BLOCK force one
 *   "schedule"      0 (default): a level runs in the one-workgroup device loop when its frontier has at most "loop_max_list"
 *                   (32768) vertices with at most "loop_max_entries" (8192) entries, else as one launch; 1: every level is a
 *                   launch; 2: every level runs in the device loop */
int grx_bipartite_set_option(grx_bipartite *p, const char *name, double value);
/* BipartiteProblem::Reset: the matching the next Enact starts from: mate_row[r] = a column or -1, `rows` int32 on the host, or
 * NULL for the empty one.  Checked on the device: GRX_BIPARTITE_BAD_MATCHING when a mate is out of range, a pair is no entry or a
 * column is used twice (the start is then the empty matching) */
int grx_bipartite_reset(grx_bipartite *p, const int *mate_row /* or NULL */);
/* BipartiteEnactor::Enact(problem, max_grid_size), HIP-event timed.  0 in both end states; GRX_BIPARTITE_NOT_CERTIFIED: there is
 * no result */
int grx_bipartite_enact(grx_bipartite *p, int max_grid_size, float *elapsed_ms);
/* Of the last Enact; any pointer may be NULL.  *size: the pairs; *phases: the searches from the unmatched columns, the last one
 * (which found no end) included; *levels: their levels; *vertical_levels: the levels of the search from the unmatched rows;
 * certificate[3]: mates that are not mutual or no entry (0), entries the cover misses plus vertices in two parts (0), the size
 * of the cover (*size, when the state is GRX_BIPARTITE_MAXIMUM); regime_columns[3]: frontier vertices walked by a lane, a wave,
 * a workgroup; *loop_levels: levels that ran in the device loop; kernel_ms[6]: when instrumented, the summed kernel time, then
 * that of the root, level, device-loop and augmenting kernels and of the rest; *build_ms: the transpose */
int grx_bipartite_stats(grx_bipartite *p, long long *size, long long *phases, long long *levels, long long *vertical_levels,
                        long long *augmentations, long long *greedy_pairs, long long *state, long long *certificate,
                        long long *regime_columns, long long *loop_levels, long long *kernel_launches, long long *readbacks,
                        double *kernel_ms, double *build_ms);
/* One row per phase of the last Enact and a last one for the search from the unmatched rows: its levels, the paths it flipped,
 * host milliseconds.  Copies the first min(count, max_phases) rows into the arrays that are not NULL and returns the count */
int grx_bipartite_phase_trace(grx_bipartite *p, int max_phases, int *levels, long long *augmentations, double *ms);
/* The matching of the last Enact (either end state): `rows` and `cols` int32, -1 for unmatched; any may be NULL.  Before a
 * finished Enact: hipErrorNotReady */
int grx_bipartite_extract_matching(grx_bipartite *p, int *h_mate_row, int *h_mate_col, long long *size);
/* The coarse decomposition: GRX_BIPARTITE_HORIZONTAL / _SQUARE / _VERTICAL per row and per column; part_sizes[6]: rows then
 * columns in the three parts.  GRX_BIPARTITE_NOT_MAXIMUM behind a capped Enact */
int grx_bipartite_extract_parts(grx_bipartite *p, int *h_row_part, int *h_col_part, long long *part_sizes);
/* König's minimum vertex cover, 1 = in the cover: the rows outside the vertical part and the columns inside it */
int grx_bipartite_extract_cover(grx_bipartite *p, unsigned char *h_row_cover, unsigned char *h_col_cover);
/* The square part with every matched pair contracted, built on the device once per result and kept with the handle: *k vertices
 * (the square rows in ascending order), one arc local(r) -> local(mate_col[c]) per entry (r, c) with both ends in the square part;
 * d_row_offsets: k + 1 int32, d_col_indices: *arcs int32, d_rows: the row of every vertex (NULL when there is none).  Its
 * strongly connected components are the blocks of the fine decomposition.  GRX_BIPARTITE_NOT_MAXIMUM behind a capped Enact */
int grx_bipartite_square_graph(grx_bipartite *p, int *k, int *arcs, int **d_row_offsets, int **d_col_indices, int **d_rows);
/* device arrays of the handle, NULL without a finished Enact (the last four also behind a capped one): mate_row, mate_col,
 * row_part, col_part (int32), row_cover, col_cover (uint8) */
int grx_bipartite_device_results(grx_bipartite *p, int **d_mate_row, int **d_mate_col, int **d_row_part, int **d_col_part,
                                 unsigned char **d_row_cover, unsigned char **d_col_cover);
void grx_bipartite_destroy(grx_bipartite *p);

/* ------------------------------------------------------------------------------------------------
 * SM: SmProblem + SmEnactor: the occurrences of a small labelled pattern H in a graph G (subgraph matching; the reference
 * snapshot's app/sm is a stub).  G is the CSR read as the simple undirected graph, as TC and the clique family read it, with an
 * optional int32 label per vertex (NULL: all 0).  H has q vertices, 2 <= q <= GRX_SM_MAX_Q, is simple and connected, and has an
 * optional int32 label per vertex, -1 a wildcard that matches any label.  An embedding is an injective map f: V(H) -> V(G) that
 * respects the labels and maps every pattern edge onto an edge and, when `induced`, every pattern non-edge onto a non-edge.
 * Aut(H) are the label-preserving automorphisms of H (the wildcard a label of its own), aut their number (<= 720).  The results:
 * occurrences = embeddings / aut; count[v] = the occurrences whose image contains v (sum = q * occurrences).  All are integers
 * with one value whatever the options; for H = K_k they are the clique family's cliques[] and total.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_sm grx_sm;
enum { GRX_SM_AUTO = 0, GRX_SM_GROUP8 = 1, GRX_SM_WAVE = 2 };  /* option "strategy" */
enum { GRX_SM_MAX_Q = 6, GRX_SM_MAX_CONSTRAINTS = 15 };
/* grx_sm_enact, next to -1 / -2 / -3: the work bound exceeds "work_limit" (nothing ran); a count was no multiple of aut under
 * "symmetry" 0.  After either there is no result */
enum { GRX_SM_TOO_LARGE = -4, GRX_SM_NOT_CERTIFIED = -5 };

int grx_sm_create(grx_sm **out, int instrument, int device);
/* SmProblem::Init: validates the CSR on the device, builds the neighbour CSR and copies the labels, once.  nodes and edges may be
 * 0.  -1: a negative size or a NULL array (col_indices may be NULL without entries); -2: not a CSR of `nodes` vertices; -3: the
 * handle has been given a graph before */
int grx_sm_init(grx_sm *p, int nodes, int edges, const int *row_offsets, const int *col_indices, const int *labels /* or NULL */);
/* the same for a CSR and labels already in HBM: borrowed, not freed; the labels are read by every Enact */
int grx_sm_init_device(grx_sm *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices, const int *d_labels /* or NULL */);
/* The pattern of the next Enact: num_pairs pairs (a[i], b[i]); duplicates and both orientations of a pair are one edge.  -1, and
 * the pattern in force stays: q outside 2 .. GRX_SM_MAX_Q, an endpoint outside [0, q), a self-loop, a disconnected pattern, a
 * pattern label below -1.  May be called before init */
int grx_sm_set_pattern(grx_sm *p, int q, int num_pairs, const int *a, const int *b, const int *pattern_labels /* or NULL */, int induced);
/* Of the pattern in force, under the options in force (hipErrorNotReady without one); any pointer may be NULL.  order[]:
 * GRX_SM_MAX_Q entries, the matching order, -1 behind the q-th; the symmetry-breaking constraints f(lower[i]) < f(higher[i]),
 * GRX_SM_MAX_CONSTRAINTS entries each, -1 behind the *num_constraints-th */
int grx_sm_pattern_info(grx_sm *p, int *q, int *aut, int *order, int *num_constraints, int *lower, int *higher);
/* named options, for the next Enact; 0: set, 1: unknown name, -1: a value out of range.  None changes a result.
 *   "symmetry"      1 (default): the constraints of Grochow and Kellis let every occurrence be found once; 0: none, every
 *                   occurrence is found aut times and the counts are divided on the device (a remainder: GRX_SM_NOT_CERTIFIED)
 *   "per_vertex"    1 (default); 0: count[] is not written (it stays 0), only the totals
 *   "strategy"      GRX_SM_AUTO (default): an item whose two end rows have at most "group_max_row" (16) entries is searched by
 *                   8 lanes, the others by a wave; GRX_SM_GROUP8 / GRX_SM_WAVE force one
 *   "work_limit"    default 2^38, at most 2^62: Enact refuses when (q - 1) * hom(T, G) exceeds it
 *   "order"         the matching order: 0 (default) the rule; 1 the reverse-key rule; 2 ascending id where that is a connected
 *                   order, else 0.  For tests */
int grx_sm_set_option(grx_sm *p, const char *name, double value);
/* SmProblem::Reset: count[] and the totals to zero (an Enact on written counts does it itself) */
int grx_sm_reset(grx_sm *p);
/* SmEnactor::Enact(problem, max_grid_size), HIP-event timed.  hipErrorNotReady without a graph or a pattern;
 * GRX_SM_TOO_LARGE; GRX_SM_NOT_CERTIFIED */
int grx_sm_enact(grx_sm *p, int max_grid_size, float *elapsed_ms);
/* Of the last Enact; any pointer may be NULL.  *items: the CSR entries that passed levels 0 and 1; regime_items[2]: those searched
 * by 8 lanes, by a wave; *candidates: row entries streamed below them; *bisections: adjacency tests; *pairs: the edges of G;
 * *bound: hom(T, G) of the anchor tree in float64; when instrumented, *kernel_ms and its split over the bin, the two enumeration
 * launches and the division; *build_ms: the neighbour CSR */
int grx_sm_stats(grx_sm *p, long long *items, long long *regime_items, long long *candidates, long long *bisections, long long *occurrences,
                 long long *embeddings, long long *pairs, long long *longest_row, long long *kernel_launches, double *bound, double *kernel_ms,
                 double *bin_ms, double *group8_ms, double *wave_ms, double *finish_ms, double *build_ms);
/* h_count: `nodes` int64, or NULL.  Before a finished Enact, or behind a refused one: hipErrorNotReady */
int grx_sm_extract(grx_sm *p, long long *h_count /* or NULL */, long long *occurrences, long long *embeddings);
/* device arrays of the handle: count (`nodes` int64) and the degrees of G (`nodes` int32) */
int grx_sm_device_results(grx_sm *p, long long **d_count, int **d_degrees);
void grx_sm_destroy(grx_sm *p);

/* ------------------------------------------------------------------------------------------------
 * SSSP: SSSPProblem + SSSPEnactor (reference gunrock/app/sssp/sssp_problem.cuh:35-387, sssp_enactor.cuh:36-563)
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_sssp grx_sssp;

/* mark_pred selects SSSPProblem<..., MARK_PATHS = true> (reference tests/sssp/test_sssp.cu:588-633) */
int grx_sssp_create(grx_sssp **out, int mark_pred, int instrument, int device);
/* SSSPProblem::Init(false, csr, 1, delta_factor) (reference sssp_problem.cuh:185-288); weights are unsigned 32-bit */
int grx_sssp_init(grx_sssp *p, int nodes, int edges, const int *row_offsets, const int *col_indices,
                  const unsigned *edge_weights, int delta_factor);
/* CSR + weights already in HBM (borrowed); `delta` is the bucket width to use (0 = one bucket per distance) */
int grx_sssp_init_device(grx_sssp *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices,
                         const unsigned *d_edge_weights, float delta);
/* Enable PULL relaxation of dense levels: a level whose frontier has more than `pull_min_edges` out-edges (-1: 3/4 of the
 * edges, 0: never) takes, for every vertex, the minimum over its IN-edges of (neighbour's distance + weight) with the reducing
 * advance -- no atomicMin per edge -- instead of pushing along the frontier's out-edges (sssp_functor.cuh:54-64).  Needs the
 * in-neighbour lists WITH the weight of every in-edge, in HBM (borrowed); pass NULLs to have the weighted transpose built on
 * the device.  Distances do not depend on it.  Call after init. */
int grx_sssp_set_inverse_graph(grx_sssp *p, const int *d_inv_row_offsets, const int *d_inv_col_indices, const unsigned *d_inv_weights,
                               long long pull_min_edges);
/* levels of the last Enact that were relaxed by pulling */
int grx_sssp_pull_levels(grx_sssp *p, long long *levels);
/* SSSPProblem::Reset(src, frontier_type, queue_sizing) (reference sssp_problem.cuh:299-377) */
int grx_sssp_reset(grx_sssp *p, int src, double queue_sizing);
/* SSSPEnactor::Enact(context, problem, src, queue_sizing, max_grid_size) (reference sssp_enactor.cuh:485-563) */
int grx_sssp_enact(grx_sssp *p, int src, int max_grid_size, float *elapsed_ms);
/* work done by the last Enact: vertices dequeued, edge slots relaxed, BSP iterations; instrumented: kernel launches
 * and summed kernel time; the bucket width in use */
int grx_sssp_stats(grx_sssp *p, long long *relaxed_vertices, long long *relaxed_edges, long long *iterations,
                   long long *kernel_launches, double *kernel_ms, float *delta);
/* SSSPProblem::Extract(h_labels, h_preds): unsigned distances (UINT_MAX unreachable); preds = own id for the source and
 * unreached vertices (reference iota initialisation, sssp_problem.cuh:363-372); h_preds may be NULL */
int grx_sssp_extract(grx_sssp *p, unsigned *h_distances, int *h_preds);
void grx_sssp_destroy(grx_sssp *p);

/* ------------------------------------------------------------------------------------------------
 * Vertex-partitioned multi-GPU BFS: the LOCAL (one GPU, one rank) steps.  The reference has no multi-GPU code
 * (gunrock/app/problem_base.cuh:336-338 is a TODO); ownership follows its striped rule owner = v mod parts,
 * local id = v div parts (problem_base.cuh:185-210).  Collectives are the caller's job (RCCL via torch.distributed in
 * gunrockinst_amd/multi_gpu.py); none of these calls communicates.
 * ---------------------------------------------------------------------------------------------- */
typedef struct grx_pbfs grx_pbfs;

int grx_pbfs_create(grx_pbfs **out, int device);
/* local CSR in HBM (borrowed): rows = owned vertices in local-id order, column ids GLOBAL */
int grx_pbfs_init_device(grx_pbfs *p, int n_global, int parts, int rank, int n_local, int m_local,
                         int *d_row_offsets, int *d_col_indices);
/* labels = -1, bitmaps = 0; the owner of `src` seeds its frontier (BFSProblem::Reset role, bfs_problem.cuh:272-360) */
int grx_pbfs_reset(grx_pbfs *p, int src);
/* current local frontier: vertices with out-edges and the sum of their degrees */
int grx_pbfs_frontier(grx_pbfs *p, unsigned *len, unsigned *edges);
/* top-down, before the exchange: advance over the local frontier; every destination not forwarded before by this rank
 * is bucketed by owner.  h_send_counts[parts] = ids per destination rank; *d_send_buffer = the ids as LOCAL ids of their
 * owner, segments in rank order (what all_to_all_single wants). */
int grx_pbfs_advance_local(grx_pbfs *p, unsigned *h_send_counts, int **d_send_buffer);
/* top-down, after the exchange: the filter operator claims + labels the received local ids (first arrival wins) and
 * builds the next local frontier; returns its length / edge count */
int grx_pbfs_filter_received(grx_pbfs *p, const int *d_recv, int n_recv, unsigned *next_len, unsigned *next_edges);
/* direction-optimizing: local queue -> local frontier bitmap (entering bottom-up) */
int grx_pbfs_queue_to_bitmap(grx_pbfs *p);
/* the local frontier bitmap to all-gather: `words` 32-bit words, identical on every rank */
int grx_pbfs_frontier_bitmap(grx_pbfs *p, unsigned **d_bitmap, int *words);
/* bottom-up level over the owned unvisited vertices against the all-gathered bitmaps (parts x words_per_rank words; words
 * of a rank's stretch behind its bitmap are never read as vertex bits).  *found = vertices discovered, the next local
 * frontier's size.  *found_edges is NOT part of the contract: the dense sweep reports 0, a level loop needs no edge count
 * while it stays bottom-up, and grx_pbfs_bitmap_to_queue recomputes it exactly on the way back to top-down. */
int grx_pbfs_bottom_up(grx_pbfs *p, const unsigned *d_gathered, int words_per_rank, unsigned *found, unsigned *found_edges);
/* local frontier bitmap -> local queue (leaving bottom-up) */
int grx_pbfs_bitmap_to_queue(grx_pbfs *p, unsigned *len, unsigned *edges);
/* device pointer to the local labels (depth per owned vertex, local-id order, -1 unreached) */
int grx_pbfs_labels(grx_pbfs *p, int **d_labels);
/* device pointer to the local predecessors (GLOBAL id of a valid BFS parent per owned vertex; -1 source, -2 unreached);
 * top-down discoveries carry a parent only when mark_pred was set (grx_pbfs_set_options) */
int grx_pbfs_preds(grx_pbfs *p, int **d_preds);

/* ---- the whole level loop inside the library: one call per search, the halo exchange through RCCL over xGMI ----
 * The reference's enactor is a host loop around operator launches (bfs_enactor.cuh:208-553); this is that loop for the
 * vertex-partitioned problem, with the per-level exchange of SURVEY 8(e) issued from C++ on the engine's stream:
 *   top-down level : advance -> bucket by owner -> ncclAllGather of the P x P count matrix -> grouped ncclSend/ncclRecv of
 *                    the ids (and, with mark_pred, of their parents) -> filter (claim, label, next frontier)
 *                    -> ncclAllGather of the packed frontier tails (termination + direction rule);
 *   bottom-up level: ONE ncclAllGather of the per-rank frontier bitmaps whose trailing word carries each rank's frontier
 *                    size -> local sweep; the search stays bottom-up to the end once Beamer's edge rule fires.
 * grx_rccl_unique_id: rank 0 creates the 128-byte ncclUniqueId, the caller distributes it (any channel) and every rank calls
 * grx_pbfs_comm_init_rccl after grx_pbfs_init_device.  RCCL is dlopen'ed on first use (librccl.so.1).
 * grx_rccl_load only loads the library (0 = every symbol resolved): ranks agree on its outcome BEFORE any of them enters
 * ncclCommInitRank, which is collective and would block the ranks that did load while the others have already given up. */
int grx_rccl_load(void);
int grx_rccl_unique_id(char id[128]);
int grx_pbfs_comm_init_rccl(grx_pbfs *p, const char id[128]);
/* the same loop with the three exchanges performed by the caller, synchronously, on device pointers (tests run several
 * ranks on one GPU over gloo this way); counts and offsets are in 32-bit words, segments in rank order */
typedef int (*grx_all_gather_fn)(void *ctx, const void *d_send, void *d_recv, size_t words_per_rank);
typedef int (*grx_all_to_all_v_fn)(void *ctx, const void *d_send, const size_t *send_counts, const size_t *send_offsets,
                                   void *d_recv, const size_t *recv_counts, const size_t *recv_offsets);
int grx_pbfs_set_transport(grx_pbfs *p, void *ctx, grx_all_gather_fn all_gather, grx_all_to_all_v_fn all_to_all_v);
/* mark_pred: exchange (id, parent) pairs on top-down levels; alpha: direction rule factor (<= 0 keeps the default, 30) */
int grx_pbfs_set_options(grx_pbfs *p, int mark_pred, float alpha);
/* Reset + the whole search from `src` (a GLOBAL vertex id, the same on every rank); levels = BSP levels executed;
 * elapsed_ms = device time of this rank from the reset to the last level (HIP events on the engine's stream) */
int grx_pbfs_search(grx_pbfs *p, int src, int direction_optimizing, int *levels, float *elapsed_ms);
/* Tuning of the level loop by name (1 = unknown name): "lite_factor" (a top-down level runs count-only -- destinations marked with
 * byte stores, ONE all-to-all of per-owner bitmap slices, then bottom-up to the end -- when global frontier edges * alpha *
 * lite_factor > unexplored edges and no parents are wanted; 0 = never), "alpha", "sparse_sweep_div", "walk_queue" (as grx_bfs_set_option).  grx_pbfs_stat:
 * "marked_levels" = count-only levels run since the handle was created (-1 = unknown name). */
int grx_pbfs_set_option(grx_pbfs *p, const char *name, double value);
long long grx_pbfs_stat(grx_pbfs *p, const char *name);
void grx_pbfs_destroy(grx_pbfs *p);

/* library / build identification: returns a static string such as "gunrock-mi355x gfx950 ..." */
/* ------------------------------------------------------------------------------------------------
 * BC: BCProblem + BCEnactor (reference gunrock/app/bc/bc_problem.cuh:36-485, bc_enactor.cuh:36-634), the instantiation of
 * the reference's C entry point: <int, int, float>, MARK_PREDECESSORS (bc_app.cu:61-66).
 * ------------------------------------------------------------------------------------------------ */
typedef struct grx_bc grx_bc;
int grx_bc_create(grx_bc **out, int device);
/* BCProblem::Init (bc_problem.cuh:203-330): host CSR in / device CSR borrowed */
int grx_bc_init(grx_bc *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
int grx_bc_init_device(grx_bc *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* The driver loop of run_bc (bc_app.cu:86-113): bc_values = 0; for src (or, when src == -1, every vertex in turn)
 * Reset + Enact; bc_values *= 0.5.  elapsed_ms = device time of the whole loop.
 * Path counts are float32.  GRX_BC_OVERFLOW: a vertex the source reaches has more than 2^126 shortest paths to it (the count, or
 * its reciprocal, is no normal float: the dependencies above it would come out 0 or NaN).  The loop stops at that source, bc_values
 * are all 0, the sigmas are not results, and the handle takes the next run. */
int grx_bc_run(grx_bc *p, int src, int max_grid_size, double queue_sizing, float *elapsed_ms);
/* BCProblem::Extract (bc_problem.cuh:140-192); sigmas are those of the LAST source; any pointer may be NULL */
int grx_bc_extract(grx_bc *p, float *h_sigmas, float *h_bc_values, float *h_ebc_values);
void grx_bc_destroy(grx_bc *p);

/* ------------------------------------------------------------------------------------------------
 * PageRank: PRProblem + PREnactor (reference gunrock/app/pr/pr_problem.cuh:36-467, pr_enactor.cuh:36-622), the <int, float, int>
 * instantiation of its C entry point (pr_app.cu:213-296).  Ranks are pulled over the in-neighbour lists by the reducing
 * advance (the reference's R_TYPE / R_OP advance + SegReduceCsr, advance/kernel.cuh:733-761), so the problem needs the
 * inverse graph.
 * ------------------------------------------------------------------------------------------------ */
typedef struct grx_pr grx_pr;
int grx_pr_create(grx_pr **out, int device);
/* PRProblem::Init (pr_problem.cuh:186-307): host CSR in / device CSR borrowed */
int grx_pr_init(grx_pr *p, int nodes, int edges, const int *row_offsets, const int *col_indices);
int grx_pr_init_device(grx_pr *p, int nodes, int edges, int *d_row_offsets, int *d_col_indices);
/* in-neighbour lists: device CSC arrays (borrowed); or NULL, NULL with build_if_null = 0 for a symmetric graph (its CSR is its
 * own inverse) or build_if_null != 0 to have the transpose built on the device.  Call after init. */
int grx_pr_set_inverse_graph(grx_pr *p, const int *d_inv_row_offsets, const int *d_inv_col_indices, int build_if_null);
/* PRProblem::Reset(src, delta, threshold, frontier_type) (pr_problem.cuh:316-457); src = -1: every vertex teleports */
int grx_pr_reset(grx_pr *p, int src, float delta, float threshold);
/* PREnactor::Enact(context, problem, max_iteration, traversal_mode, max_grid_size) (pr_enactor.cuh:536-618), HIP-event timed */
int grx_pr_enact(grx_pr *p, int max_iter, int max_grid_size, float *elapsed_ms);
/* iterations run, peeling rounds (vertices without out-edges are removed round by round first, pr_enactor.cuh:220-300) and the
 * number of vertices left after peeling */
int grx_pr_stats(grx_pr *p, long long *iterations, long long *peeling_rounds, long long *surviving_nodes);
/* PRProblem::Extract (pr_problem.cuh:139-175): the first `count` ranks in descending order with their vertex ids
 * (count < 0: all); either pointer may be NULL */
int grx_pr_extract(grx_pr *p, float *h_rank_sorted, int *h_node_ids, int count);
/* device arrays: ranks indexed by vertex, vertex ids by descending rank */
int grx_pr_device_results(grx_pr *p, float **d_rank_by_vertex, int **d_node_ids_by_rank);
void grx_pr_destroy(grx_pr *p);

const char *grx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GUNROCK_GUNROCK_MI355X_H_ */
