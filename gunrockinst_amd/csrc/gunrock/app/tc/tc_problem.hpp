// app/tc/tc_problem.hpp -- device data for triangle counting and clustering coefficients.
//
// The reference snapshot has no app/tc; the shape is this tree's Problem (compare app/mis/mis_problem.hpp).  The input CSR is read
// as MIS reads it: an undirected simple graph G in which u and v are neighbours when either row holds the other, self-loops
// ignored, unsorted rows, duplicates and one-way edges allowed.  Init builds on the device, with the in-tree radix sort and scan:
//   1. one key (min << cb | max) per CSR entry, self-loops as the sentinel; sorted; duplicates flagged off: the M edges of G
//      (graphio::PairGraph's Keys and CountKept, graphio/pair_graph.hpp)
//   2. d(v) by two atomic adds per edge
//   3. every edge oriented from the endpoint with the smaller (d, id) to the larger, keyed (src << cb | dst) at its rank, sorted
//      again: the oriented CSR with rows ascending by id; its offsets are the scanned out-degrees
// Out-rows are short: v's out-neighbours all have d >= d+(v) (their (d, id) is larger and d+(v) <= d(v)), so the sum of degrees
// 2M >= d+(v)^2, d+(v) <= floor(sqrt(2M)).
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/tc/tc_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace tc {

template <bool _USE_DOUBLE_BUFFER>
struct TCProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<Count> d_triangles;  // the result, one 64-bit count per vertex
        DeviceArray<unsigned> d_degrees;  // d(v) in G
        DeviceArray<int> d_oro;  // the oriented CSR
        DeviceArray<int> d_oci;
        DeviceArray<int> d_osrc;  // the row of every oriented entry
        DeviceArray<int> d_rows[2];  // the LDS and the global regime's row lists
        DeviceArray<int> d_words;  // BinKernel's counters
        DeviceArray<Count> d_counters;  // [0] triangles, [1] entries probed; [2] sum of C(d, 2), [3] the largest out-row
        DeviceArray<double> d_coeff;  // clustering coefficients (allocated at the first request)
    };

    SliceHolder<DataSlice> data_slices;
    long long oriented_edges = 0; // M
    long long max_out_row = 0;
    long long wedges = 0;         // sum over v of C(d(v), 2)
    long long total = 0;          // of the last Extract
    double build_ms = 0;          // HIP-event time of the oriented-graph build

    Oriented DeviceGraph() const
    {
        const DataSlice *ds = data_slices[0];
        return Oriented{ds->d_oro, ds->d_oci, ds->d_osrc};
    }

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = ds->d_words.Alloc(4))) return retval;
        if ((retval = ds->d_counters.Alloc(4))) return retval;

        // 1. the CSR must be one: the build indexes with what it reads
        if ((retval = this->ValidateCsr())) return retval;

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;

        if ((retval = ds->d_triangles.Alloc(n1))) return retval;
        if ((retval = ds->d_degrees.Alloc(n1))) return retval;
        if ((retval = ds->d_oro.Alloc(n1 + 1))) return retval;
        if ((retval = ds->d_rows[0].Alloc(n1))) return retval;
        if ((retval = ds->d_rows[1].Alloc(n1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_degrees, 0, sizeof(unsigned) * n1, stream), "TCProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_oro, 0, sizeof(int) * (n1 + 1), stream), "TCProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(Count) * 4, stream), "TCProblem memset failed");

        graphio::PairGraph pg(n);  // (its keys, keep flags and positions; the orientation is TC's own)
        graphio::DeviceKeySort oriented_sort;
        if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
        if ((retval = pg.CountKept(stream, &oriented_edges))) return retval;
        if (oriented_edges > 0) {
            hipLaunchKernelGGL(DegreeKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, pg.d_sorted, pg.d_keep, m, pg.col_bits, ds->d_degrees);
            GR_CHECK(hipGetLastError(), "DegreeKernel launch failed");
            GR_CHECK(oriented_sort.Reserve(oriented_edges), "TCProblem sort scratch failed");
            graphio::DeviceScratch<unsigned> outdeg;  // n + 1 words, the last one 0: its scan is the offsets
            if ((retval = outdeg.Alloc(n1 + 1))) return retval;
            GR_CHECK(hipMemsetAsync(outdeg.p, 0, sizeof(unsigned) * (n1 + 1), stream), "TCProblem memset failed");
            hipLaunchKernelGGL(OrientKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, pg.d_sorted, pg.d_keep, pg.d_pos, m, pg.col_bits, ds->d_degrees,
                               oriented_sort.Keys(), outdeg.p);
            GR_CHECK(hipGetLastError(), "OrientKernel launch failed");
            GR_CHECK(graphio::DeviceExclusiveScan<int>(outdeg.p, ds->d_oro, n + 1, pg.d_sums, stream), "TCProblem offset scan failed");
            unsigned long long *d_osorted = nullptr;
            GR_CHECK(oriented_sort.Sort(oriented_edges, pg.key_bits, stream, &d_osorted), "TCProblem oriented sort failed");
            if ((retval = ds->d_oci.Alloc(static_cast<size_t>(oriented_edges)))) return retval;
            if ((retval = ds->d_osrc.Alloc(static_cast<size_t>(oriented_edges)))) return retval;
            hipLaunchKernelGGL(EmitOrientedKernel, dim3(graphio::PairGrid(oriented_edges)), dim3(256), 0, stream, d_osorted, oriented_edges, pg.col_bits, ds->d_oci,
                               ds->d_osrc);
            GR_CHECK(hipGetLastError(), "EmitOrientedKernel launch failed");
            GR_CHECK(hipStreamSynchronize(stream), "TCProblem build sync failed");  // (outdeg goes here)
        }
        hipLaunchKernelGGL(RowSummaryKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_degrees, ds->d_oro, n, ds->d_counters + 2);
        GR_CHECK(hipGetLastError(), "RowSummaryKernel launch failed");
        Count summary[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(summary, ds->d_counters + 2, sizeof(summary), hipMemcpyDeviceToHost, stream), "TCProblem read-back failed");
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "TCProblem build sync failed");
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        wedges = static_cast<long long>(summary[0]);
        max_out_row = static_cast<long long>(summary[1]);
        return retval;
    }

    // One Init per object (grx_tc_init refuses a second one)
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

    // the counts to zero
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        GR_CHECK(hipMemsetAsync(ds->d_triangles, 0, sizeof(Count) * static_cast<size_t>(this->nodes), stream), "TCProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(Count) * 2, stream), "TCProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(int) * 4, stream), "TCProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "TCProblem Reset sync failed");
        total = 0;
        return retval;
    }

    // h_triangles may be NULL: then only the total is read
    hipError_t Extract(long long *h_triangles)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        Count t = 0;
        GR_CHECK(hipMemcpyAsync(&t, ds->d_counters, sizeof(t), hipMemcpyDeviceToHost, stream), "TCProblem read total failed");
        if (h_triangles)
            GR_CHECK(hipMemcpyAsync(h_triangles, ds->d_triangles, sizeof(Count) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost, stream),
                     "TCProblem read d_triangles failed");
        GR_CHECK(hipStreamSynchronize(stream), "TCProblem Extract sync failed");
        total = static_cast<long long>(t);
        return retval;
    }

    // h_coeff may be NULL: then only the transitivity 3 total / sum C(d, 2) is computed (one double division; 0 for no wedge)
    hipError_t Clustering(double *h_coeff, double *transitivity)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if ((retval = Extract(nullptr))) return retval;
        if (transitivity) *transitivity = wedges > 0 ? static_cast<double>(3 * total) / static_cast<double>(wedges) : 0.0;
        if (!h_coeff) return retval;
        const size_t n = static_cast<size_t>(this->nodes);
        if (!ds->d_coeff && (retval = ds->d_coeff.Alloc(n))) return retval;
        hipLaunchKernelGGL(ClusteringKernel, dim3(graphio::PairGrid(this->nodes)), dim3(256), 0, stream, ds->d_triangles, ds->d_degrees,
                           static_cast<long long>(this->nodes), ds->d_coeff);
        GR_CHECK(hipGetLastError(), "ClusteringKernel launch failed");
        GR_CHECK(hipMemcpyAsync(h_coeff, ds->d_coeff, sizeof(double) * n, hipMemcpyDeviceToHost, stream), "TCProblem read d_coeff failed");
        GR_CHECK(hipStreamSynchronize(stream), "TCProblem Clustering sync failed");
        return retval;
    }
};

}  // namespace tc
}  // namespace app
}  // namespace gunrock
