// app/clique/clique_problem.hpp -- device data for k-clique counting.
//
// The reference snapshot has no app/clique; the shape is app/tc/tc_problem.hpp's, and so is the build, step for step, with
// app/tc's kernels where they fit unchanged.  The input CSR is read as TC reads it: an undirected simple graph G in which u and v are
// neighbours when either row holds the other, self-loops ignored, unsorted rows, duplicates and one-way edges allowed.  Init:
//   1. the M edges of G (graphio::PairGraph's Keys and CountKept) and d(v)
//   2. with a rank: the compacted pairs and the neighbour CSR (PairGraph's Pairs and Rows) and on them the peel that breaks the
//      rank's ties (RankPeel*Kernel): a vertex leaves in the first round in which at most max(rank, 0) neighbours of its own or a
//      higher rank are left
//   3. every edge oriented from the endpoint with the smaller (rank, round, d, id) to the larger (RankOrientKernel), sorted again:
//      the oriented CSR, rows ascending by id
//   4. the longest out-row, and sum over u of C(d+(u), k - 1) for k = 3 .. 6 in float64: the bounds Enact refuses by
// Without a rank, or with all ranks equal and <= 0, nobody with a neighbour leaves the peel, the order is TC's (d, id) and no out-row
// exceeds floor(sqrt(2M)).  With core numbers as the rank every vertex leaves (shell c is what the peel of the c-core removes at level
// c) with at most core(v) neighbours behind it, so no out-row exceeds the degeneracy; (core, d, id) alone would not give that (29
// against 24 on the seeded scale-10 R-MAT).  Any rank is as correct: the order stays total; only the rows may be longer, up to
// nodes - 1.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/clique/clique_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace clique {

template <bool _USE_DOUBLE_BUFFER>
struct CliqueProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<Count> d_cliques;  // the result, one 64-bit count per vertex
        DeviceArray<unsigned> d_degrees; // d(v) in G
        DeviceArray<int> d_oro;  // the oriented CSR
        DeviceArray<int> d_oci;
        DeviceArray<int> d_osrc;  // the row of every oriented entry
        DeviceArray<int> d_bitmap_rows;  // the bitmap regime's row list
        DeviceArray<int> d_list_edges;  // the list regime's oriented edges
        DeviceArray<int> d_words;  // BinKernel's counters
        DeviceArray<Count> d_counters;  // [0] cliques, [1] bit-row ANDs, [2] list look-ups; [4] sum of C(d, 2), [5] the largest out-row
        DeviceArray<double> d_bound;  // [k - 3]: sum over u of C(d+(u), k - 1)
        Grown<int> slabs;              // the list regime's scratch, grown by Enact
    };

    SliceHolder<DataSlice> data_slices;
    long long oriented_edges = 0;  // M
    long long max_out_row = 0;
    double bound[4] = {0, 0, 0, 0};  // for k = 3 .. 6
    long long total = 0;           // of the last Extract
    bool dirty = false;            // an Enact has written since the last Reset
    double build_ms = 0;           // HIP-event time of the oriented-graph build

    Oriented DeviceGraph() const
    {
        const DataSlice *ds = data_slices[0];
        return Oriented{ds->d_oro, ds->d_oci, ds->d_osrc};
    }

    // d_rank: one int32 per vertex on the device, or NULL (all equal)
    hipError_t Build(const int *d_rank)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = ds->d_words.Alloc(4))) return retval;
        if ((retval = ds->d_counters.Alloc(6))) return retval;
        if ((retval = ds->d_bound.Alloc(4))) return retval;

        // 1. the CSR must be one: the build indexes with what it reads
        if ((retval = this->ValidateCsr())) return retval;

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;

        if ((retval = ds->d_cliques.Alloc(n1))) return retval;
        if ((retval = ds->d_degrees.Alloc(n1))) return retval;
        if ((retval = ds->d_oro.Alloc(n1 + 1))) return retval;
        if ((retval = ds->d_bitmap_rows.Alloc(n1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_cliques, 0, sizeof(Count) * n1, stream), "CliqueProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_degrees, 0, sizeof(unsigned) * n1, stream), "CliqueProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_oro, 0, sizeof(int) * (n1 + 1), stream), "CliqueProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(Count) * 6, stream), "CliqueProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_bound, 0, sizeof(double) * 4, stream), "CliqueProblem memset failed");

        graphio::PairGraph pg(n);  // (its keys, keep flags and positions; the orientation is this family's own)
        graphio::DeviceKeySort oriented_sort;
        graphio::DeviceScratch<unsigned> round;  // with a rank: the peel round of every vertex
        if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
        if (d_rank) {  // the compacted pairs and the neighbour CSR, for the peel that breaks the rank's ties
            if ((retval = pg.Pairs(stream))) return retval;
            oriented_edges = pg.pairs;
            if (oriented_edges > 0) {
                if ((retval = pg.Rows(stream))) return retval;
                if ((retval = PeelRounds(pg, d_rank, round, stream))) return retval;
                GR_CHECK(hipMemcpyAsync(ds->d_degrees, pg.d_deg, sizeof(unsigned) * static_cast<size_t>(n), hipMemcpyDeviceToDevice, stream),
                         "CliqueProblem degree copy failed");
            }
        } else {
            if ((retval = pg.CountKept(stream, &oriented_edges))) return retval;
        }
        if (oriented_edges > 0) {
            const int grid_m = graphio::PairGrid(m);
            if (!d_rank) {
                hipLaunchKernelGGL(tc::DegreeKernel, dim3(grid_m), dim3(256), 0, stream, pg.d_sorted, pg.d_keep, m, pg.col_bits, ds->d_degrees);
                GR_CHECK(hipGetLastError(), "DegreeKernel launch failed");
            }
            GR_CHECK(oriented_sort.Reserve(oriented_edges), "CliqueProblem sort scratch failed");
            graphio::DeviceScratch<unsigned> outdeg;  // n + 1 words, the last one 0: its scan is the offsets
            if ((retval = outdeg.Alloc(n1 + 1))) return retval;
            GR_CHECK(hipMemsetAsync(outdeg.p, 0, sizeof(unsigned) * (n1 + 1), stream), "CliqueProblem memset failed");
            if (d_rank)
                hipLaunchKernelGGL(RankOrientKernel, dim3(graphio::PairGrid(oriented_edges)), dim3(256), 0, stream, pg.d_ckeys, nullptr, nullptr,
                                   oriented_edges, pg.col_bits, d_rank, round.p, ds->d_degrees, oriented_sort.Keys(), outdeg.p);
            else
                hipLaunchKernelGGL(RankOrientKernel, dim3(grid_m), dim3(256), 0, stream, pg.d_sorted, pg.d_keep, pg.d_pos, m, pg.col_bits, nullptr,
                                   nullptr, ds->d_degrees, oriented_sort.Keys(), outdeg.p);
            GR_CHECK(hipGetLastError(), "RankOrientKernel launch failed");
            GR_CHECK(graphio::DeviceExclusiveScan<int>(outdeg.p, ds->d_oro, n + 1, pg.d_sums, stream), "CliqueProblem offset scan failed");
            unsigned long long *d_osorted = nullptr;
            GR_CHECK(oriented_sort.Sort(oriented_edges, pg.key_bits, stream, &d_osorted), "CliqueProblem oriented sort failed");
            const size_t ms = static_cast<size_t>(oriented_edges);
            if ((retval = ds->d_oci.Alloc(ms))) return retval;
            if ((retval = ds->d_osrc.Alloc(ms))) return retval;
            if ((retval = ds->d_list_edges.Alloc(ms))) return retval;
            hipLaunchKernelGGL(tc::EmitOrientedKernel, dim3(graphio::PairGrid(oriented_edges)), dim3(256), 0, stream, d_osorted, oriented_edges,
                               pg.col_bits, ds->d_oci, ds->d_osrc);
            GR_CHECK(hipGetLastError(), "EmitOrientedKernel launch failed");
            GR_CHECK(hipStreamSynchronize(stream), "CliqueProblem build sync failed");  // (outdeg goes here)
        }
        hipLaunchKernelGGL(tc::RowSummaryKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_degrees, ds->d_oro, n, ds->d_counters + 4);
        GR_CHECK(hipGetLastError(), "RowSummaryKernel launch failed");
        hipLaunchKernelGGL(BoundKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_oro, n, ds->d_bound);
        GR_CHECK(hipGetLastError(), "BoundKernel launch failed");
        Count summary[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(summary, ds->d_counters + 4, sizeof(summary), hipMemcpyDeviceToHost, stream), "CliqueProblem read-back failed");
        GR_CHECK(hipMemcpyAsync(bound, ds->d_bound, sizeof(bound), hipMemcpyDeviceToHost, stream), "CliqueProblem read-back failed");
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "CliqueProblem build sync failed");
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        max_out_row = static_cast<long long>(summary[1]);
        return retval;
    }

    // round.p[v] = the round in which RankPeel*Kernel let v go (clique_functor.hpp), kNeverPeeled for one that stays.  One launch
    // and one 4-byte read-back per round; the rounds are the depth of the peel inside the rank's classes.
    hipError_t PeelRounds(const graphio::PairGraph &pg, const int *d_rank, graphio::DeviceScratch<unsigned> &round, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        const int n = static_cast<int>(this->nodes);
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        graphio::DeviceScratch<int> live, lists, counts;
        if ((retval = round.Alloc(n1))) return retval;
        if ((retval = live.Alloc(n1))) return retval;
        if ((retval = lists.Alloc(2 * n1))) return retval;
        if ((retval = counts.Alloc(2))) return retval;
        GR_CHECK(hipMemsetAsync(counts.p, 0, sizeof(int) * 2, stream), "CliqueProblem memset failed");
        auto grid = [](long long waves) { return static_cast<int>(waves < 4 ? 1 : waves > 4 * 8192 ? 8192 : (waves + 3) / 4); };
        hipLaunchKernelGGL(RankPeelInitKernel, dim3(grid(n)), dim3(256), 0, stream, pg.d_ro, pg.d_ci, d_rank, n, live.p, round.p, lists.p, counts.p);
        GR_CHECK(hipGetLastError(), "RankPeelInitKernel launch failed");
        for (unsigned r = 0;; ++r) {
            const int in = r & 1, out = in ^ 1;
            int count = 0;
            GR_CHECK(hipMemcpyAsync(&count, counts.p + in, sizeof(int), hipMemcpyDeviceToHost, stream), "CliqueProblem read-back failed");
            GR_CHECK(hipStreamSynchronize(stream), "CliqueProblem peel sync failed");
            if (count == 0) break;
            GR_CHECK(hipMemsetAsync(counts.p + out, 0, sizeof(int), stream), "CliqueProblem memset failed");
            hipLaunchKernelGGL(RankPeelRoundKernel, dim3(grid(count)), dim3(256), 0, stream, pg.d_ro, pg.d_ci, d_rank, lists.p + in * n1, count, r, live.p,
                               round.p, lists.p + out * n1, counts.p + out);
            GR_CHECK(hipGetLastError(), "RankPeelRoundKernel launch failed");
        }
        return retval;
    }

    // One Init per object (grx_clique_init refuses a second one).  h_rank: `nodes` int32 on the host, or NULL
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, const int *h_rank, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, false))) return retval;
        data_slices.Make();
        graphio::DeviceScratch<int> rank;
        if (h_rank) {
            const size_t bytes = sizeof(int) * static_cast<size_t>(this->nodes);
            if ((retval = rank.Alloc(static_cast<size_t>(this->nodes)))) return retval;
            GR_CHECK(hipMemcpy(rank.p, h_rank, bytes, hipMemcpyHostToDevice), "CliqueProblem rank copy failed");
        }
        return Build(rank.p);
    }

    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, const int *d_rank)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        data_slices.Make();
        return Build(d_rank);
    }

    // the counts to zero
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        GR_CHECK(hipMemsetAsync(ds->d_cliques, 0, sizeof(Count) * static_cast<size_t>(this->nodes), stream), "CliqueProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(Count) * 4, stream), "CliqueProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(int) * 4, stream), "CliqueProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "CliqueProblem Reset sync failed");
        total = 0;
        dirty = false;
        return retval;
    }

    // h_cliques may be NULL: then only the total is read
    hipError_t Extract(long long *h_cliques)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        Count t = 0;
        GR_CHECK(hipMemcpyAsync(&t, ds->d_counters, sizeof(t), hipMemcpyDeviceToHost, stream), "CliqueProblem read total failed");
        if (h_cliques)
            GR_CHECK(hipMemcpyAsync(h_cliques, ds->d_cliques, sizeof(Count) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost, stream),
                     "CliqueProblem read d_cliques failed");
        GR_CHECK(hipStreamSynchronize(stream), "CliqueProblem Extract sync failed");
        total = static_cast<long long>(t);
        return retval;
    }
};

}  // namespace clique
}  // namespace app
}  // namespace gunrock
