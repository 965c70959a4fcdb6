// app/c4/c4_problem.hpp -- device data for 4-cycle (butterfly) counting.
//
// The reference snapshot has no app/c4; the shape is app/clique/clique_problem.hpp's.  The input CSR is read as TC reads it: an
// undirected simple graph G in which u and v are neighbours when either row holds the other, self-loops ignored, unsorted rows,
// duplicates and one-way edges allowed.  Init:
//   1. the M canonical pairs of G (graphio::PairGraph's Keys and Pairs): src[e] < dst[e] in (src, dst) order, the order of every
//      per-edge array, and d(v) counted over them
//   2. the vertices sorted by (d, id): rank[] and its inverse
//   3. both directions of every pair as a key (rank << cb | rank), sorted: the neighbour CSR renumbered by rank, rows ascending.  The
//      offsets and dlow[] by bisection of the keys; the canonical pair of an entry by bisection of the pairs' keys, as FillRowsKernel
//      finds it (DESIGN.md 3.22 says why this and not PairGraph::Rows on renumbered pairs)
//   4. per entry (u, v) with v below u the prefix of row v below u (one bisection), summed into W[u]
//   5. the wedges, the largest W and sum over u of W(u) (dlow(u) - 1) / 2 in float64: the bound Enact refuses by
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/c4/c4_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace c4 {

template <bool _USE_DOUBLE_BUFFER>
struct C4Problem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<Count> d_cycles;  // the result, one 64-bit count per vertex
        DeviceArray<Count> d_edge_cycles;  // one per canonical pair; allocated by the first Enact that credits edges
        DeviceArray<int> d_src;  // the canonical pairs
        DeviceArray<int> d_dst;
        DeviceArray<int> d_inv;  // rank -> vertex
        DeviceArray<int> d_ro;  // the renumbered neighbour CSR
        DeviceArray<int> d_ci;
        DeviceArray<int> d_eid;
        DeviceArray<int> d_pre;
        DeviceArray<int> d_dlow;
        DeviceArray<int> d_wedges;  // W per start vertex
        DeviceArray<int> d_lists;  // 2 n: BlockKernel's and GlobalKernel's start vertices
        DeviceArray<unsigned long long> d_words;  // W_COUNT words of the kernels, then [0] the wedges, [1] the largest W
        DeviceArray<double> d_bound;
        Grown<int> rows;                 // the GLOBAL regime's counter rows, grown by Enact, all 0 between launches
    };

    SliceHolder<DataSlice> data_slices;
    long long simple_edges = 0;   // M
    long long wedges = 0;         // the sum of W
    long long max_wedges = 0;     // the largest W
    double bound = 0;
    long long total = 0;          // of the last Extract
    bool dirty = false;           // an Enact has written since the last Reset
    double build_ms = 0;          // HIP-event time of the build

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT + 2))) return retval;
        if ((retval = ds->d_bound.Alloc(1))) return retval;

        // 1. the CSR must be one: the build indexes with what it reads
        if ((retval = this->ValidateCsr())) return retval;

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;

        if ((retval = ds->d_cycles.Alloc(n1))) return retval;
        if ((retval = ds->d_inv.Alloc(n1))) return retval;
        if ((retval = ds->d_ro.Alloc(n1 + 1))) return retval;
        if ((retval = ds->d_dlow.Alloc(n1))) return retval;
        if ((retval = ds->d_wedges.Alloc(n1))) return retval;
        if ((retval = ds->d_lists.Alloc(2 * n1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_cycles, 0, sizeof(Count) * n1, stream), "C4Problem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_ro, 0, sizeof(int) * (n1 + 1), stream), "C4Problem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_dlow, 0, sizeof(int) * n1, stream), "C4Problem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_wedges, 0, sizeof(int) * n1, stream), "C4Problem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * (W_COUNT + 2), stream), "C4Problem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_bound, 0, sizeof(double), stream), "C4Problem memset failed");

        graphio::PairGraph pg(n);
        graphio::DeviceKeySort rank_sort, row_sort;
        graphio::DeviceScratch<unsigned> deg;
        graphio::DeviceScratch<int> rank;
        if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
        if ((retval = pg.Pairs(stream))) return retval;
        simple_edges = pg.pairs;
        if (simple_edges > 0) {
            const long long M = simple_edges, entries = 2 * M;
            const int grid_n = graphio::PairGrid(n + 1), grid_m = graphio::PairGrid(M), grid_e = graphio::PairGrid(entries);
            // 2. the rank
            if ((retval = deg.Alloc(n1))) return retval;
            if ((retval = rank.Alloc(n1))) return retval;
            GR_CHECK(hipMemsetAsync(deg.p, 0, sizeof(unsigned) * n1, stream), "C4Problem memset failed");
            hipLaunchKernelGGL(PairDegreeKernel, dim3(grid_m), dim3(256), 0, stream, pg.d_src, pg.d_dst, M, deg.p);
            GR_CHECK(hipGetLastError(), "PairDegreeKernel launch failed");
            GR_CHECK(rank_sort.Reserve(n), "C4Problem sort scratch failed");
            hipLaunchKernelGGL(RankKeysKernel, dim3(grid_n), dim3(256), 0, stream, deg.p, n, pg.col_bits, rank_sort.Keys());
            GR_CHECK(hipGetLastError(), "RankKeysKernel launch failed");
            unsigned long long *d_ranked = nullptr;
            GR_CHECK(rank_sort.Sort(n, pg.key_bits, stream, &d_ranked), "C4Problem rank sort failed");
            hipLaunchKernelGGL(RankKernel, dim3(grid_n), dim3(256), 0, stream, d_ranked, n, pg.col_bits, rank.p, ds->d_inv);
            GR_CHECK(hipGetLastError(), "RankKernel launch failed");
            // 3. the renumbered rows
            GR_CHECK(row_sort.Reserve(entries), "C4Problem sort scratch failed");
            hipLaunchKernelGGL(RowKeysKernel, dim3(grid_m), dim3(256), 0, stream, pg.d_src, pg.d_dst, rank.p, M, pg.col_bits, row_sort.Keys());
            GR_CHECK(hipGetLastError(), "RowKeysKernel launch failed");
            unsigned long long *d_rows = nullptr;
            GR_CHECK(row_sort.Sort(entries, pg.key_bits, stream, &d_rows), "C4Problem row sort failed");
            const size_t es = static_cast<size_t>(entries);
            if ((retval = ds->d_ci.Alloc(es))) return retval;
            if ((retval = ds->d_eid.Alloc(es))) return retval;
            if ((retval = ds->d_pre.Alloc(es))) return retval;
            hipLaunchKernelGGL(OffsetsKernel, dim3(grid_n), dim3(256), 0, stream, d_rows, entries, n, pg.col_bits, ds->d_ro, ds->d_dlow);
            GR_CHECK(hipGetLastError(), "OffsetsKernel launch failed");
            // 4. the entries and W
            hipLaunchKernelGGL(EntriesKernel, dim3(grid_e), dim3(256), 0, stream, d_rows, entries, pg.col_bits, ds->d_ro, ds->d_inv, pg.d_ckeys, M,
                               ds->d_ci, ds->d_eid, ds->d_pre, ds->d_wedges);
            GR_CHECK(hipGetLastError(), "EntriesKernel launch failed");
            // 5. the summary
            hipLaunchKernelGGL(SummaryKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_wedges, ds->d_dlow, n, ds->d_words + W_COUNT,
                               ds->d_bound);
            GR_CHECK(hipGetLastError(), "SummaryKernel launch failed");
            ds->d_src.Adopt(graphio::Take(pg.d_src));
            ds->d_dst.Adopt(graphio::Take(pg.d_dst));
        }
        unsigned long long summary[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(summary, ds->d_words + W_COUNT, sizeof(summary), hipMemcpyDeviceToHost, stream), "C4Problem read-back failed");
        GR_CHECK(hipMemcpyAsync(&bound, ds->d_bound, sizeof(bound), hipMemcpyDeviceToHost, stream), "C4Problem read-back failed");
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "C4Problem build sync failed");  // (the sorts' buffers go behind this)
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        wedges = static_cast<long long>(summary[0]);
        max_wedges = static_cast<long long>(summary[1]);
        return retval;
    }

    // One Init per object (grx_c4_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, false))) return retval;
        data_slices.Make();
        return Build();
    }

    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        data_slices.Make();
        return Build();
    }

    // the per-edge counts, once a first Enact asks for them
    hipError_t NeedEdgeCycles()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if (ds->d_edge_cycles || simple_edges < 1) return retval;
        if ((retval = ds->d_edge_cycles.Alloc(static_cast<size_t>(simple_edges)))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_edge_cycles, 0, sizeof(Count) * static_cast<size_t>(simple_edges), this->graph_slices[0]->stream), "C4Problem memset failed");
        return retval;
    }

    // the counts to zero
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        GR_CHECK(hipMemsetAsync(ds->d_cycles, 0, sizeof(Count) * static_cast<size_t>(this->nodes), stream), "C4Problem memset failed");
        if (ds->d_edge_cycles)
            GR_CHECK(hipMemsetAsync(ds->d_edge_cycles, 0, sizeof(Count) * static_cast<size_t>(simple_edges), stream), "C4Problem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "C4Problem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "C4Problem Reset sync failed");
        total = 0;
        dirty = false;
        return retval;
    }

    // h_cycles may be NULL: then only the total is read
    hipError_t Extract(long long *h_cycles)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        unsigned long long t = 0;
        GR_CHECK(hipMemcpyAsync(&t, ds->d_words + W_TOTAL, sizeof(t), hipMemcpyDeviceToHost, stream), "C4Problem read total failed");
        if (h_cycles)
            GR_CHECK(hipMemcpyAsync(h_cycles, ds->d_cycles, sizeof(Count) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost, stream),
                     "C4Problem read d_cycles failed");
        GR_CHECK(hipStreamSynchronize(stream), "C4Problem Extract sync failed");
        total = static_cast<long long>(t);
        return retval;
    }

    // either may be NULL
    hipError_t Edges(int *h_src, int *h_dst)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t bytes = sizeof(int) * static_cast<size_t>(simple_edges);
        if (simple_edges < 1) return retval;
        if (h_src) GR_CHECK(hipMemcpy(h_src, ds->d_src, bytes, hipMemcpyDeviceToHost), "C4Problem read d_src failed");
        if (h_dst) GR_CHECK(hipMemcpy(h_dst, ds->d_dst, bytes, hipMemcpyDeviceToHost), "C4Problem read d_dst failed");
        return retval;
    }

    hipError_t ExtractEdges(long long *h_edge_cycles)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if (simple_edges < 1 || !h_edge_cycles) return retval;
        GR_CHECK(hipMemcpy(h_edge_cycles, ds->d_edge_cycles, sizeof(Count) * static_cast<size_t>(simple_edges), hipMemcpyDeviceToHost),
                 "C4Problem read d_edge_cycles failed");
        return retval;
    }
};

}  // namespace c4
}  // namespace app
}  // namespace gunrock
