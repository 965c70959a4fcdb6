// app/kcore/kcore_problem.hpp -- device data for the k-core decomposition.
//
// The reference snapshot has no app/kcore; the shape is this tree's Problem (compare app/tc/tc_problem.hpp).  The input CSR is read
// as MIS and TC read it: an undirected simple graph G in which u and v are neighbours when either row holds the other, self-loops
// ignored, unsorted rows, duplicates and one-way edges allowed.  Init builds on the device, with the in-tree radix sort and scan:
//   1. one key (min << cb | max) per CSR entry, self-loops as the sentinel; sorted; duplicates flagged off: the M edges of G
//      (graphio::PairGraph's Keys step, graphio/pair_graph.hpp)
//   2. d(v) by two atomic adds per edge; its exclusive scan is the offsets of the neighbour CSR, 2M entries
//   3. both directions of every edge scattered through per-row cursors: the symmetric simple neighbour CSR (rows unordered)
// core[] is the working array and the result (kcore_functor.hpp): Reset copies d(v) into it.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/kcore/kcore_functor.hpp>
#include <gunrock/app/problem_base.hpp>
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // (only TC's DegreeKernel is used here)
#include <gunrock/app/tc/tc_functor.hpp>
#pragma clang diagnostic pop
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace kcore {

template <bool _USE_DOUBLE_BUFFER>
struct KcoreProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_core;  // the working degrees, then the result
        DeviceArray<int> d_degrees;  // d(v) in G (nodes + 1 words, the last 0: scanned into the offsets)
        DeviceArray<int> d_nro;  // the neighbour CSR
        DeviceArray<int> d_nci;
        DeviceArray<int> d_queue;  // every vertex once, in peeling order
        DeviceArray<int> d_list[2];  // the live list, rebuilt from one into the other
        DeviceArray<unsigned> d_words;  // W_* of kcore_functor.hpp
        DeviceArray<unsigned long long> d_counters;  // [0] row entries walked; [1], [2] Members' counts; [3] the end of the trace's clock
        DeviceArray<int> d_trace_k;  // one entry per level scan (max degree + 1: levels are distinct values)
        DeviceArray<int> d_trace_tail;
        DeviceArray<unsigned long long> d_trace_clock;
        DeviceArray<unsigned long long> d_shell;  // allocated at the first request
        DeviceArray<unsigned char> d_mask;  // allocated at the first request
    };

    SliceHolder<DataSlice> data_slices;
    long long simple_edges = 0;  // M
    long long max_degree = 0;
    long long min_degree = 0;    // the smallest positive d(v)
    long long zeros = 0;         // vertices with d(v) = 0
    long long trace_capacity = 0;
    long long shell_capacity = 0;
    int degeneracy = 0;          // of the last Extract
    bool fresh = false;          // Reset has run and Enact has not: core[] holds d(v) and the words are clear
    double build_ms = 0;         // HIP-event time of the neighbour-CSR build

    Graph DeviceGraph() const
    {
        const DataSlice *ds = data_slices[0];
        return Graph{ds->d_nro, ds->d_nci};
    }

    // d_out[0..2] of SummaryKernel over d_values
    hipError_t Summary(const int *d_values, unsigned *out)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const unsigned init[3] = {0u, kNoLevel, 0u};
        unsigned *d_out = ds->d_words + W_COUNT;  // (three words behind the shared ones)
        GR_CHECK(hipMemcpyAsync(d_out, init, sizeof(init), hipMemcpyHostToDevice, stream), "KcoreProblem summary init failed");
        hipLaunchKernelGGL(SummaryKernel, dim3(graphio::PairGrid(this->nodes)), dim3(256), 0, stream, d_values, static_cast<long long>(this->nodes), d_out);
        GR_CHECK(hipGetLastError(), "SummaryKernel launch failed");
        GR_CHECK(hipMemcpyAsync(out, d_out, sizeof(init), hipMemcpyDeviceToHost, stream), "KcoreProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "KcoreProblem read-back sync failed");
        return retval;
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
        if ((retval = ds->d_counters.Alloc(4))) return retval;

        // 1. the CSR must be one: the build indexes with what it reads
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * (W_COUNT + 4), stream), "KcoreProblem memset failed");
        if ((retval = this->ValidateCsr())) return retval;

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;

        if ((retval = ds->d_core.Alloc(n1))) return retval;
        if ((retval = ds->d_degrees.Alloc(n1 + 1))) return retval;
        if ((retval = ds->d_nro.Alloc(n1 + 1))) return retval;
        if ((retval = ds->d_queue.Alloc(n1))) return retval;
        if ((retval = ds->d_list[0].Alloc(n1))) return retval;
        if ((retval = ds->d_list[1].Alloc(n1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_degrees, 0, sizeof(int) * (n1 + 1), stream), "KcoreProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_nro, 0, sizeof(int) * (n1 + 1), stream), "KcoreProblem memset failed");

        graphio::PairGraph pg(n);  // (its keys and keep flags; the unordered rows are k-core's own)
        graphio::DeviceScratch<unsigned> cursor;
        graphio::DeviceScratch<unsigned long long> sums;
        simple_edges = 0;
        if (m > 0) {
            if ((retval = cursor.Alloc(n1))) return retval;
            if ((retval = sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(n + 1))))) return retval;
            GR_CHECK(hipMemsetAsync(cursor.p, 0, sizeof(unsigned) * n1, stream), "KcoreProblem memset failed");
            if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
            hipLaunchKernelGGL(tc::DegreeKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, pg.d_sorted, pg.d_keep, m, pg.col_bits,
                               reinterpret_cast<unsigned *>(ds->d_degrees.p));
            GR_CHECK(hipGetLastError(), "DegreeKernel launch failed");
            GR_CHECK(graphio::DeviceExclusiveScan<int>(reinterpret_cast<unsigned *>(ds->d_degrees.p), ds->d_nro, n + 1, sums.p, stream),
                     "KcoreProblem offset scan failed");
            int entries = 0;  // 2M <= 2 * edges; edges is an int, and so is every offset: refuse what does not fit
            GR_CHECK(hipMemcpyAsync(&entries, ds->d_nro + n, sizeof(int), hipMemcpyDeviceToHost, stream), "KcoreProblem read-back failed");
            GR_CHECK(hipStreamSynchronize(stream), "KcoreProblem read-back sync failed");
            if (entries < 0) return hipErrorInvalidValue;
            simple_edges = entries / 2;
            if (entries > 0) {
                if ((retval = ds->d_nci.Alloc(static_cast<size_t>(entries)))) return retval;
                hipLaunchKernelGGL(NeighbourScatterKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, pg.d_sorted, pg.d_keep, m, pg.col_bits, ds->d_nro,
                                   cursor.p, ds->d_nci);
                GR_CHECK(hipGetLastError(), "NeighbourScatterKernel launch failed");
            }
        }
        unsigned summary[3] = {0, 0, 0};
        if ((retval = Summary(ds->d_degrees, summary))) return retval;
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "KcoreProblem build sync failed");
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        max_degree = summary[0];
        min_degree = summary[1] == kNoLevel ? 0 : summary[1];
        zeros = summary[2];
        trace_capacity = max_degree + 1;
        if ((retval = ds->d_trace_k.Alloc(static_cast<size_t>(trace_capacity)))) return retval;
        if ((retval = ds->d_trace_tail.Alloc(static_cast<size_t>(trace_capacity)))) return retval;
        if ((retval = ds->d_trace_clock.Alloc(static_cast<size_t>(trace_capacity)))) return retval;
        return retval;
    }

    // One Init per object (grx_kcore_init refuses a second one)
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

    // core[v] = d(v): every vertex with a neighbour is live
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        GR_CHECK(hipMemcpyAsync(ds->d_core, ds->d_degrees, sizeof(int) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToDevice, stream),
                 "KcoreProblem Reset copy failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * W_COUNT, stream), "KcoreProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(unsigned long long) * 4, stream), "KcoreProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "KcoreProblem Reset sync failed");
        degeneracy = 0;
        fresh = true;
        return retval;
    }

    // h_core may be NULL: then only the degeneracy (the largest value) is read
    hipError_t Extract(int *h_core)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        unsigned summary[3] = {0, 0, 0};
        if ((retval = Summary(ds->d_core, summary))) return retval;
        degeneracy = static_cast<int>(summary[0]);
        if (h_core) {
            GR_CHECK(hipMemcpyAsync(h_core, ds->d_core, sizeof(int) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost, stream),
                     "KcoreProblem read d_core failed");
            GR_CHECK(hipStreamSynchronize(stream), "KcoreProblem Extract sync failed");
        }
        return retval;
    }

    // h_sizes[c] = the vertices with core c, c = 0 .. degeneracy, as far as max_entries reaches; *count = degeneracy + 1
    hipError_t Shells(int max_entries, long long *h_sizes, int *count)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if ((retval = Extract(nullptr))) return retval;
        const long long shells = static_cast<long long>(degeneracy) + 1;
        if (count) *count = static_cast<int>(shells);
        if (!h_sizes || max_entries < 1) return retval;
        if (shells > shell_capacity) {
            if ((retval = ds->d_shell.Alloc(static_cast<size_t>(shells)))) return retval;
            shell_capacity = shells;
        }
        GR_CHECK(hipMemsetAsync(ds->d_shell, 0, sizeof(unsigned long long) * static_cast<size_t>(shells), stream), "KcoreProblem memset failed");
        hipLaunchKernelGGL(ShellKernel, dim3(graphio::PairGrid(this->nodes)), dim3(256), 0, stream, ds->d_core, static_cast<long long>(this->nodes), ds->d_shell);
        GR_CHECK(hipGetLastError(), "ShellKernel launch failed");
        const long long take = shells < max_entries ? shells : max_entries;
        GR_CHECK(hipMemcpyAsync(h_sizes, ds->d_shell, sizeof(long long) * static_cast<size_t>(take), hipMemcpyDeviceToHost, stream),
                 "KcoreProblem read d_shell failed");
        GR_CHECK(hipStreamSynchronize(stream), "KcoreProblem Shells sync failed");
        return retval;
    }

    // the k-core: h_mask (may be NULL) = core >= k, its vertices and the edges of G inside it
    hipError_t Members(int k, int wave_min_row, unsigned char *h_mask, long long *vertices, long long *edges)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t n = static_cast<size_t>(this->nodes);
        if (!ds->d_mask && (retval = ds->d_mask.Alloc(n))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_counters + 1, 0, sizeof(unsigned long long) * 2, stream), "KcoreProblem memset failed");
        hipLaunchKernelGGL(MembersKernel, dim3(graphio::PairGrid(this->nodes)), dim3(kKcoreThreads), 0, stream, DeviceGraph(), ds->d_core,
                           static_cast<long long>(this->nodes), k, wave_min_row, ds->d_mask, ds->d_counters + 1);
        GR_CHECK(hipGetLastError(), "MembersKernel launch failed");
        unsigned long long out[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(out, ds->d_counters + 1, sizeof(out), hipMemcpyDeviceToHost, stream), "KcoreProblem read-back failed");
        if (h_mask) GR_CHECK(hipMemcpyAsync(h_mask, ds->d_mask, n, hipMemcpyDeviceToHost, stream), "KcoreProblem read d_mask failed");
        GR_CHECK(hipStreamSynchronize(stream), "KcoreProblem Members sync failed");
        if (vertices) *vertices = static_cast<long long>(out[0]);
        if (edges) *edges = static_cast<long long>(out[1]);
        return retval;
    }
};

}  // namespace kcore
}  // namespace app
}  // namespace gunrock
