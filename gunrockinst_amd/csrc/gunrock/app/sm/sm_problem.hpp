// app/sm/sm_problem.hpp -- device data of subgraph matching.
//
// The reference snapshot has no working app/sm; the shape is app/clique/clique_problem.hpp's.  The input CSR is read as TC and the
// clique family read it: the simple undirected graph G in which u and v are neighbours when either row holds the other, self-loops
// ignored, unsorted rows, duplicates and one-way entries allowed.  Init:
//   1. the CSR is validated on the device (graphio::DeviceValidateCsr) before anything indexes with what it reads
//   2. graphio::PairGraph's Keys, Pairs and Rows: the M canonical pairs and the mirrored neighbour CSR of 2M entries, rows ascending
//   3. the row of every entry, the row lengths and the longest row
//   4. the labels, one int32 per vertex: copied from the host, borrowed from the device, or none (all 0)
// Bound() runs the leaf-to-root dynamic programme of hom(T, G) for a plan's anchor tree T: h[leaf][v] = 1, h[x][v] = the product
// over the children c of x of the sum over u in N(v) of h[c][u], in float64, one row-sum pass per tree edge.  Every array is an
// owning DeviceArray member.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/sm/sm_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace sm {

template <bool _USE_DOUBLE_BUFFER>
struct SmProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<Count> d_count;     // the result, one 64-bit count per vertex
        DeviceArray<Count> d_counters;  // C_*
        DeviceArray<unsigned> d_words;  // W_*
        DeviceArray<int> d_nro, d_nci, d_src;  // the neighbour CSR and the row of every entry
        DeviceArray<unsigned> d_deg;
        DeviceArray<unsigned> d_longest;
        DeviceArray<int> own_labels;
        const int *d_labels = nullptr;  // own_labels, the caller's, or NULL
        DeviceArray<int> d_items8, d_items64;
        DeviceArray<double> d_bound;
        Grown<double> h;  // q x nodes: the dynamic programme's tables
    };

    SliceHolder<DataSlice> data_slices;
    long long pairs = 0;        // M
    long long longest_row = 0;
    bool dirty = false;         // an Enact has written since the last Reset
    double build_ms = 0;

    Graph DeviceGraph() const
    {
        const DataSlice *ds = data_slices[0];
        return Graph{ds->d_nro, ds->d_nci, ds->d_src, ds->d_deg, ds->d_labels, static_cast<int>(this->nodes), 2 * pairs};
    }

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = this->ValidateCsr())) return retval;

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;
        if ((retval = ds->d_count.Alloc(n1))) return retval;
        if ((retval = ds->d_counters.Alloc(C_COUNT))) return retval;
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        if ((retval = ds->d_deg.Alloc(n1))) return retval;
        if ((retval = ds->d_longest.Alloc(1))) return retval;
        if ((retval = ds->d_bound.Alloc(1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_deg, 0, sizeof(unsigned) * n1, stream), "SmProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_longest, 0, sizeof(unsigned), stream), "SmProblem memset failed");

        graphio::PairGraph pg(n);
        if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
        if ((retval = pg.Pairs(stream))) return retval;
        if ((retval = pg.Rows(stream))) return retval;
        pairs = pg.pairs;
        ds->d_nro.Adopt(graphio::Take(pg.d_ro));
        if (pairs > 0) ds->d_nci.Adopt(graphio::Take(pg.d_ci));
        else if ((retval = ds->d_nci.Alloc(1))) return retval;
        const size_t entries = static_cast<size_t>(2 * pairs);
        if ((retval = ds->d_src.Alloc(entries))) return retval;
        if ((retval = ds->d_items8.Alloc(entries))) return retval;
        if ((retval = ds->d_items64.Alloc(entries))) return retval;
        hipLaunchKernelGGL(RowOfEntryKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_nro.p, n, ds->d_src.p, ds->d_deg.p, ds->d_longest.p);
        GR_CHECK(hipGetLastError(), "RowOfEntryKernel launch failed");
        unsigned longest = 0;
        GR_CHECK(hipMemcpyAsync(&longest, ds->d_longest, sizeof(longest), hipMemcpyDeviceToHost, stream), "SmProblem read-back failed");
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "SmProblem build sync failed");  // (pg goes here)
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        longest_row = longest;
        return Reset();
    }

    // One Init per object (grx_sm_init refuses a second one).  h_labels: `nodes` int32 on the host, or NULL
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, const int *h_labels, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, false))) return retval;
        DataSlice *ds = data_slices.Make();
        if (h_labels) {
            if ((retval = ds->own_labels.Alloc(static_cast<size_t>(this->nodes)))) return retval;
            if (this->nodes > 0)
                GR_CHECK(hipMemcpy(ds->own_labels, h_labels, sizeof(int) * static_cast<size_t>(this->nodes), hipMemcpyHostToDevice),
                         "SmProblem label copy failed");
            ds->d_labels = ds->own_labels;
        }
        return Build();
    }

    // d_labels is borrowed, as the CSR is
    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, const int *d_labels)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        data_slices.Make()->d_labels = d_labels;
        return Build();
    }

    // hom(T, G) of the plan's anchor tree, labels ignored, into *bound
    hipError_t Bound(const PlanLevels &plan, double *bound)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        *bound = 0;
        if (n < 1) return retval;
        const size_t nn = static_cast<size_t>(n);
        if ((retval = ds->h.Need(nn * static_cast<size_t>(plan.q)))) return retval;
        const dim3 grid(graphio::PairGrid(n)), block(256);
        hipLaunchKernelGGL(oprtr::FillKernel<double>, dim3(graphio::PairGrid(n * plan.q)), block, 0, stream, ds->h.p, n * plan.q, 1.0);
        GR_CHECK(hipGetLastError(), "FillKernel launch failed");
        const Graph g = DeviceGraph();
        for (int l = plan.q - 1; l >= 1; --l) {  // a child's level is behind its parent's: its table is complete when it is read
            hipLaunchKernelGGL(BoundRowKernel, grid, block, 0, stream, g, ds->h.p + nn * l, ds->h.p + nn * plan.level[l].parent);
            GR_CHECK(hipGetLastError(), "BoundRowKernel launch failed");
        }
        GR_CHECK(hipMemsetAsync(ds->d_bound, 0, sizeof(double), stream), "SmProblem memset failed");
        hipLaunchKernelGGL(BoundSumKernel, grid, block, 0, stream, ds->h.p, n, ds->d_bound.p);
        GR_CHECK(hipGetLastError(), "BoundSumKernel launch failed");
        GR_CHECK(hipMemcpyAsync(bound, ds->d_bound, sizeof(double), hipMemcpyDeviceToHost, stream), "SmProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "SmProblem bound sync failed");
        return retval;
    }

    // the counts to zero
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        GR_CHECK(hipMemsetAsync(ds->d_count, 0, sizeof(Count) * static_cast<size_t>(this->nodes > 0 ? this->nodes : 1), stream), "SmProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(Count) * C_COUNT, stream), "SmProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * W_COUNT, stream), "SmProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "SmProblem Reset sync failed");
        dirty = false;
        return retval;
    }
};

}  // namespace sm
}  // namespace app
}  // namespace gunrock
