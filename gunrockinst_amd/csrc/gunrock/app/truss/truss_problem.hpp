// app/truss/truss_problem.hpp -- device data for per-edge triangle support and the k-truss decomposition.
//
// The reference snapshot has no app/truss; the shape is this tree's Problem (compare app/kcore/kcore_problem.hpp).  The input CSR
// is read as MIS, TC and k-core read it.  Init builds on the device, with the in-tree radix sort and scan:
//   1. to 3. graphio::PairGraph's Keys, Pairs and Rows (graphio/pair_graph.hpp): the M canonical edges src[e] < dst[e] in
//      (src, dst) order and the neighbour CSR, 2M entries, rows ascending by id, every entry with the id of its edge
//   4. the support pass (truss_functor.hpp) into support[], kept: Reset copies it into the working array val[]
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/truss/truss_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace truss {

template <bool _USE_DOUBLE_BUFFER>
struct TrussProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_src;  // the canonical edges
        DeviceArray<int> d_dst;
        DeviceArray<int> d_nro;  // the neighbour CSR, rows ascending,
        DeviceArray<int> d_nci;
        DeviceArray<int> d_neid;  // and the edge of every entry
        DeviceArray<int> d_support;  // triangles per edge
        DeviceArray<int> d_val;  // the working array: support, then truss - 2
        DeviceArray<int> d_stamp;  // 0: live; else the sub-round in which the edge is in the frontier
        DeviceArray<int> d_truss;  // the result of the last Enact
        DeviceArray<int> d_queue;  // every edge once, in peeling order
        DeviceArray<int> d_vertex;  // `nodes` words: Members' flags, VertexTruss's result
        DeviceArray<unsigned> d_words;  // W_* of truss_functor.hpp, and three words behind them for the summaries
        DeviceArray<unsigned long long> d_counters;  // [0] entries walked by the peel; [1], [2] Members' counts; [3] the trace's end; [4] the
                                                   // support pass's entries; [5] sum(support)
        DeviceArray<int> d_trace_k;
        DeviceArray<int> d_trace_tail;
        DeviceArray<unsigned long long> d_trace_clock;
        DeviceArray<unsigned long long> d_classes;  // allocated at the first request
        DeviceArray<unsigned char> d_mask;  // allocated at the first request
    };

    SliceHolder<DataSlice> data_slices;
    long long simple_edges = 0;  // M
    long long triangles = 0;
    long long max_support = 0;
    long long min_support = 0;
    long long support_entries = 0;  // tail entries walked by the support pass
    long long trace_capacity = 0;
    long long class_capacity = 0;
    int max_truss = 0;       // of the last Extract
    int wave_min_row = kWaveMinRow;  // of the support pass (Init runs before any option can be meant for it: the default)
    bool fresh = false;      // Reset has run and Enact has not
    bool enacted = false;    // truss[] holds a result
    double build_ms = 0;     // HIP-event time of the build of the edges and the neighbour CSR
    double support_ms = 0;   // and of the support pass

    Graph DeviceGraph() const
    {
        const DataSlice *ds = data_slices[0];
        return Graph{ds->d_nro, ds->d_nci, ds->d_neid, ds->d_src, ds->d_dst};
    }

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT + 4))) return retval;
        if ((retval = ds->d_counters.Alloc(8))) return retval;

        // the CSR must be one: the build indexes with what it reads
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(unsigned long long) * 8, stream), "TrussProblem memset failed");
        if ((retval = this->ValidateCsr())) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * (W_COUNT + 4), stream), "TrussProblem memset failed");

        graphio::BuildEvents ev;
        if ((retval = ev.Create(3))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;

        if ((retval = ds->d_vertex.Alloc(n1))) return retval;
        graphio::PairGraph pg(n);  // steps 1 to 3
        if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
        if ((retval = pg.Pairs(stream))) return retval;
        if ((retval = pg.Rows(stream))) return retval;
        ds->d_src.Adopt(graphio::Take(pg.d_src));
        ds->d_dst.Adopt(graphio::Take(pg.d_dst));
        ds->d_nro.Adopt(graphio::Take(pg.d_ro));
        ds->d_nci.Adopt(graphio::Take(pg.d_ci));
        ds->d_neid.Adopt(graphio::Take(pg.d_eid));
        const long long M = pg.pairs;
        simple_edges = M;
        const size_t m1 = static_cast<size_t>(M > 0 ? M : 1);
        if ((retval = ds->d_support.Alloc(m1))) return retval;
        if ((retval = ds->d_val.Alloc(m1))) return retval;
        if ((retval = ds->d_stamp.Alloc(m1))) return retval;
        if ((retval = ds->d_truss.Alloc(m1))) return retval;
        if ((retval = ds->d_queue.Alloc(m1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_support, 0, sizeof(int) * m1, stream), "TrussProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_truss, 0, sizeof(int) * m1, stream), "TrussProblem memset failed");
        if ((retval = ev.Record(1, stream))) return retval;

        unsigned summary[2] = {0u, kNoLevel};
        unsigned *d_out = ds->d_words + W_COUNT;
        GR_CHECK(hipMemcpyAsync(d_out, summary, sizeof(summary), hipMemcpyHostToDevice, stream), "TrussProblem summary init failed");
        if (M > 0) {
            hipLaunchKernelGGL(SupportKernel, dim3(graphio::PairGrid(M)), dim3(kTrussThreads), 0, stream, DeviceGraph(), M, wave_min_row, ds->d_support,
                               ds->d_counters + 4);
            GR_CHECK(hipGetLastError(), "SupportKernel launch failed");
            hipLaunchKernelGGL(SupportSummaryKernel, dim3(graphio::PairGrid(M)), dim3(256), 0, stream, ds->d_support, M, d_out, ds->d_counters + 5);
            GR_CHECK(hipGetLastError(), "SupportSummaryKernel launch failed");
        }
        if ((retval = ev.Record(2, stream))) return retval;
        unsigned long long sums[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(summary, d_out, sizeof(summary), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
        GR_CHECK(hipMemcpyAsync(sums, ds->d_counters + 4, sizeof(sums), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem build sync failed");
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        if ((retval = ev.Elapsed(1, 2, &support_ms))) return retval;
        max_support = summary[0];
        min_support = summary[1] == kNoLevel ? 0 : summary[1];
        support_entries = static_cast<long long>(sums[0]);
        triangles = static_cast<long long>(sums[1] / 3);
        trace_capacity = max_support + 2;
        if ((retval = ds->d_trace_k.Alloc(static_cast<size_t>(trace_capacity)))) return retval;
        if ((retval = ds->d_trace_tail.Alloc(static_cast<size_t>(trace_capacity)))) return retval;
        if ((retval = ds->d_trace_clock.Alloc(static_cast<size_t>(trace_capacity)))) return retval;
        return retval;
    }

    // One Init per object (grx_truss_init refuses a second one)
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

    // val[e] = support[e]: every edge live
    hipError_t Reset(FrontierType /*frontier_type*/ = EDGE_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t bytes = sizeof(int) * static_cast<size_t>(simple_edges);
        if (bytes) {
            GR_CHECK(hipMemcpyAsync(ds->d_val, ds->d_support, bytes, hipMemcpyDeviceToDevice, stream), "TrussProblem Reset copy failed");
            GR_CHECK(hipMemsetAsync(ds->d_stamp, 0, bytes, stream), "TrussProblem memset failed");
        }
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * W_COUNT, stream), "TrussProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(unsigned long long) * 4, stream), "TrussProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem Reset sync failed");
        fresh = true;
        return retval;
    }

    hipError_t Edges(int *h_src, int *h_dst)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t bytes = sizeof(int) * static_cast<size_t>(simple_edges);
        if (bytes && h_src) GR_CHECK(hipMemcpyAsync(h_src, ds->d_src, bytes, hipMemcpyDeviceToHost, stream), "TrussProblem read d_src failed");
        if (bytes && h_dst) GR_CHECK(hipMemcpyAsync(h_dst, ds->d_dst, bytes, hipMemcpyDeviceToHost, stream), "TrussProblem read d_dst failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem Edges sync failed");
        return retval;
    }

    hipError_t Support(int *h_support)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t bytes = sizeof(int) * static_cast<size_t>(simple_edges);
        if (bytes && h_support) {
            GR_CHECK(hipMemcpyAsync(h_support, ds->d_support, bytes, hipMemcpyDeviceToHost, stream), "TrussProblem read d_support failed");
            GR_CHECK(hipStreamSynchronize(stream), "TrussProblem Support sync failed");
        }
        return retval;
    }

    // h_truss may be NULL: then only max_truss (the largest value, 0 without an edge) is read
    hipError_t Extract(int *h_truss)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        unsigned summary[2] = {0u, kNoLevel};
        unsigned *d_out = ds->d_words + W_COUNT;
        GR_CHECK(hipMemcpyAsync(d_out, summary, sizeof(summary), hipMemcpyHostToDevice, stream), "TrussProblem summary init failed");
        if (simple_edges > 0) {
            hipLaunchKernelGGL(SupportSummaryKernel, dim3(graphio::PairGrid(simple_edges)), dim3(256), 0, stream, ds->d_truss, simple_edges, d_out,
                               ds->d_counters + 6);
            GR_CHECK(hipGetLastError(), "SupportSummaryKernel launch failed");
        }
        GR_CHECK(hipMemcpyAsync(summary, d_out, sizeof(summary), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
        const size_t bytes = sizeof(int) * static_cast<size_t>(simple_edges);
        if (bytes && h_truss) GR_CHECK(hipMemcpyAsync(h_truss, ds->d_truss, bytes, hipMemcpyDeviceToHost, stream), "TrussProblem read d_truss failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem Extract sync failed");
        max_truss = static_cast<int>(summary[0]);
        return retval;
    }

    // h_sizes[k] = the edges with truss k, k = 0 .. max_truss, as far as max_entries reaches; *count = max_truss + 1
    hipError_t Classes(int max_entries, long long *h_sizes, int *count)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if ((retval = Extract(nullptr))) return retval;
        const long long classes = static_cast<long long>(max_truss) + 1;
        if (count) *count = static_cast<int>(classes);
        if (!h_sizes || max_entries < 1) return retval;
        if (classes > class_capacity) {
            if ((retval = ds->d_classes.Alloc(static_cast<size_t>(classes)))) return retval;
            class_capacity = classes;
        }
        GR_CHECK(hipMemsetAsync(ds->d_classes, 0, sizeof(unsigned long long) * static_cast<size_t>(classes), stream), "TrussProblem memset failed");
        if (simple_edges > 0) {  // (k-core's kernel: the lanes of a wave that hold the same value add once)
            hipLaunchKernelGGL(kcore::ShellKernel, dim3(graphio::PairGrid(simple_edges)), dim3(256), 0, stream, ds->d_truss, simple_edges, ds->d_classes);
            GR_CHECK(hipGetLastError(), "ShellKernel launch failed");
        }
        const long long take = classes < max_entries ? classes : max_entries;
        GR_CHECK(hipMemcpyAsync(h_sizes, ds->d_classes, sizeof(long long) * static_cast<size_t>(take), hipMemcpyDeviceToHost, stream),
                 "TrussProblem read d_classes failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem Classes sync failed");
        return retval;
    }

    // the k-truss: h_mask (may be NULL) = truss >= k per edge, its edges and the vertices at one of them
    hipError_t Members(int k, unsigned char *h_mask, long long *edges, long long *vertices)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t M = static_cast<size_t>(simple_edges);
        if (!ds->d_mask && (retval = ds->d_mask.Alloc(M > 0 ? M : 1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_counters + 1, 0, sizeof(unsigned long long) * 2, stream), "TrussProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_vertex, 0, sizeof(int) * static_cast<size_t>(this->nodes), stream), "TrussProblem memset failed");
        if (M > 0) {
            hipLaunchKernelGGL(MemberEdgesKernel, dim3(graphio::PairGrid(simple_edges)), dim3(256), 0, stream, DeviceGraph(), ds->d_truss, simple_edges, k,
                               ds->d_mask, ds->d_vertex, ds->d_counters + 1);
            GR_CHECK(hipGetLastError(), "MemberEdgesKernel launch failed");
            hipLaunchKernelGGL(CountFlagsKernel, dim3(graphio::PairGrid(this->nodes)), dim3(256), 0, stream, ds->d_vertex, static_cast<long long>(this->nodes),
                               ds->d_counters + 2);
            GR_CHECK(hipGetLastError(), "CountFlagsKernel launch failed");
        }
        unsigned long long out[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(out, ds->d_counters + 1, sizeof(out), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
        if (h_mask && M > 0) GR_CHECK(hipMemcpyAsync(h_mask, ds->d_mask, M, hipMemcpyDeviceToHost, stream), "TrussProblem read d_mask failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem Members sync failed");
        if (edges) *edges = static_cast<long long>(out[0]);
        if (vertices) *vertices = static_cast<long long>(out[1]);
        return retval;
    }

    hipError_t VertexTruss(int *h_vertex)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t bytes = sizeof(int) * static_cast<size_t>(this->nodes);
        GR_CHECK(hipMemsetAsync(ds->d_vertex, 0, bytes, stream), "TrussProblem memset failed");
        if (simple_edges > 0) {
            hipLaunchKernelGGL(VertexTrussKernel, dim3(graphio::PairGrid(simple_edges)), dim3(256), 0, stream, DeviceGraph(), ds->d_truss, simple_edges,
                               ds->d_vertex);
            GR_CHECK(hipGetLastError(), "VertexTrussKernel launch failed");
        }
        if (h_vertex) GR_CHECK(hipMemcpyAsync(h_vertex, ds->d_vertex, bytes, hipMemcpyDeviceToHost, stream), "TrussProblem read d_vertex failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem VertexTruss sync failed");
        return retval;
    }
};

}  // namespace truss
}  // namespace app
}  // namespace gunrock
