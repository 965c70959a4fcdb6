// app/truss/truss_problem.hpp -- device data for per-edge triangle support and the k-truss decomposition.
//
// The reference snapshot has no app/truss; the shape is this tree's Problem (compare app/kcore/kcore_problem.hpp).  The input CSR
// is read as MIS, TC and k-core read it.  Init builds on the device, with the in-tree radix sort and scan:
//   1. one key (min << cb | max) per CSR entry, self-loops as the sentinel; sorted; duplicates flagged off; the kept keys
//      compacted: the M canonical edges src[e] < dst[e] in (src, dst) order (TC's first step, with TC's kernels)
//   2. the same edges keyed (max << cb | min) and sorted: the lower parts of the rows; both key arrays bisected per vertex give
//      d(v) and, scanned, the offsets of the neighbour CSR, 2M entries
//   3. row v = its lower neighbours, then its upper ones: ascending by id, every entry with the id of its edge
//   4. the support pass (truss_functor.hpp) into support[], kept: Reset copies it into the working array val[]
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/truss/truss_functor.hpp>
#include <gunrock/graphio/device_sort.hpp>

namespace gunrock {
namespace app {
namespace truss {

template <bool _USE_DOUBLE_BUFFER>
struct TrussProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        int *d_src = nullptr;      // the canonical edges
        int *d_dst = nullptr;
        int *d_nro = nullptr;      // the neighbour CSR, rows ascending,
        int *d_nci = nullptr;
        int *d_neid = nullptr;     // and the edge of every entry
        int *d_support = nullptr;  // triangles per edge
        int *d_val = nullptr;      // the working array: support, then truss - 2
        int *d_stamp = nullptr;    // 0: live; else the sub-round in which the edge is in the frontier
        int *d_truss = nullptr;    // the result of the last Enact
        int *d_queue = nullptr;    // every edge once, in peeling order
        int *d_vertex = nullptr;   // `nodes` words: Members' flags, VertexTruss's result
        unsigned *d_words = nullptr;               // W_* of truss_functor.hpp, and three words behind them for the summaries
        unsigned long long *d_counters = nullptr;  // [0] entries walked by the peel; [1], [2] Members' counts; [3] the trace's end; [4] the
                                                   // support pass's entries; [5] sum(support)
        int *d_trace_k = nullptr;
        int *d_trace_tail = nullptr;
        unsigned long long *d_trace_clock = nullptr;
        unsigned long long *d_classes = nullptr;  // allocated at the first request
        unsigned char *d_mask = nullptr;          // allocated at the first request
    };

    DataSlice **data_slices = nullptr;
    int malformed = 0;
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

    ~TrussProblem() override
    {
        if (data_slices) {
            DataSlice *ds = data_slices[0];
            if (ds) {
                void *bufs[] = {ds->d_src, ds->d_dst, ds->d_nro, ds->d_nci, ds->d_neid, ds->d_support, ds->d_val, ds->d_stamp, ds->d_truss,
                                ds->d_queue, ds->d_vertex, ds->d_words, ds->d_counters, ds->d_trace_k, ds->d_trace_tail, ds->d_trace_clock,
                                ds->d_classes, ds->d_mask};
                for (void *b : bufs)
                    if (b) util::GRError(hipFree(b), "TrussProblem hipFree failed", __FILE__, __LINE__);
                delete ds;
            }
            delete[] data_slices;
        }
    }

    static int Grid(long long work)
    {
        long long blocks = (work + 255) / 256;
        if (blocks < 1) blocks = 1;
        if (blocks > 2048) blocks = 2048;  // 256 CUs x 8 workgroups, grid-stride the rest
        return static_cast<int>(blocks);
    }

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
        GR_CHECK(hipMalloc(&ds->d_words, sizeof(unsigned) * (W_COUNT + 4)), "TrussProblem hipMalloc failed");
        GR_CHECK(hipMalloc(&ds->d_counters, sizeof(unsigned long long) * 8), "TrussProblem hipMalloc failed");

        // the CSR must be one: the build indexes with what it reads
        int bad = 0;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * (W_COUNT + 4), stream), "TrussProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(unsigned long long) * 8, stream), "TrussProblem memset failed");
        hipLaunchKernelGGL(tc::ValidateCsrKernel, dim3(Grid((n > m ? n : m) + 1)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices,
                           n, m, reinterpret_cast<int *>(ds->d_words));
        GR_CHECK(hipGetLastError(), "ValidateCsrKernel launch failed");
        GR_CHECK(hipMemcpyAsync(&bad, ds->d_words, sizeof(int), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem read-back sync failed");
        if (bad) {
            malformed = 1;
            return hipErrorInvalidValue;
        }
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * (W_COUNT + 4), stream), "TrussProblem memset failed");

        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        for (int i = 0; i < 3; ++i) GR_CHECK(hipEventCreate(&ev[i]), "TrussProblem hipEventCreate failed");
        GR_CHECK(hipEventRecord(ev[0], stream), "TrussProblem hipEventRecord failed");

        GR_CHECK(hipMalloc(&ds->d_nro, sizeof(int) * (n1 + 1)), "TrussProblem hipMalloc d_nro failed");
        GR_CHECK(hipMalloc(&ds->d_vertex, sizeof(int) * n1), "TrussProblem hipMalloc d_vertex failed");
        GR_CHECK(hipMemsetAsync(ds->d_nro, 0, sizeof(int) * (n1 + 1), stream), "TrussProblem memset failed");

        int col_bits = 1;
        while ((1ll << col_bits) < n) ++col_bits;
        const int key_bits = 2 * col_bits;  // <= 62
        const unsigned long long sentinel = (1ull << key_bits) - 1ull;  // min = max = 2^cb - 1: never an edge
        unsigned *d_keep = nullptr, *d_deg = nullptr;
        unsigned long long *d_pos = nullptr, *d_sums = nullptr, *d_ckeys = nullptr;
        int *d_up = nullptr, *d_low = nullptr;
        graphio::DeviceKeySort edge_sort;
        long long M = 0;
        if (m > 0) {
            const long long scan_words = m > n + 1 ? m : n + 1;
            GR_CHECK(hipMalloc(&d_keep, sizeof(unsigned) * static_cast<size_t>(m)), "TrussProblem hipMalloc failed");
            GR_CHECK(hipMalloc(&d_pos, sizeof(unsigned long long) * static_cast<size_t>(m)), "TrussProblem hipMalloc failed");
            GR_CHECK(hipMalloc(&d_sums, sizeof(unsigned long long) * static_cast<size_t>(graphio::ScanScratchWords(scan_words))),
                     "TrussProblem hipMalloc failed");
            GR_CHECK(edge_sort.Reserve(m), "TrussProblem sort scratch failed");
            hipLaunchKernelGGL(tc::EdgeKeysKernel, dim3(Grid(m)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices, static_cast<int>(n),
                               m, col_bits, sentinel, edge_sort.Keys());
            GR_CHECK(hipGetLastError(), "EdgeKeysKernel launch failed");
            unsigned long long *d_sorted = nullptr;
            GR_CHECK(edge_sort.Sort(m, key_bits, stream, &d_sorted), "TrussProblem edge sort failed");
            hipLaunchKernelGGL(graphio::FlagKernel, dim3(Grid(m)), dim3(256), 0, stream, d_sorted, m, sentinel, d_keep);
            GR_CHECK(hipGetLastError(), "FlagKernel launch failed");
            GR_CHECK(graphio::DeviceExclusiveScan<unsigned long long>(d_keep, d_pos, m, d_sums, stream), "TrussProblem flag scan failed");
            unsigned long long last_pos = 0;
            unsigned last_keep = 0;
            GR_CHECK(hipMemcpyAsync(&last_pos, d_pos + (m - 1), sizeof(last_pos), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
            GR_CHECK(hipMemcpyAsync(&last_keep, d_keep + (m - 1), sizeof(last_keep), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
            GR_CHECK(hipStreamSynchronize(stream), "TrussProblem read-back sync failed");
            M = static_cast<long long>(last_pos) + last_keep;
            if (2 * M > 0x7FFFFFFFll) return hipErrorInvalidValue;  // every offset of the 2M entries is an int
            if (M > 0) {
                const size_t ms = static_cast<size_t>(M);
                GR_CHECK(hipMalloc(&d_ckeys, sizeof(unsigned long long) * ms), "TrussProblem hipMalloc failed");
                GR_CHECK(hipMalloc(&ds->d_src, sizeof(int) * ms), "TrussProblem hipMalloc d_src failed");
                GR_CHECK(hipMalloc(&ds->d_dst, sizeof(int) * ms), "TrussProblem hipMalloc d_dst failed");
                GR_CHECK(hipMalloc(&ds->d_nci, sizeof(int) * 2 * ms), "TrussProblem hipMalloc d_nci failed");
                GR_CHECK(hipMalloc(&ds->d_neid, sizeof(int) * 2 * ms), "TrussProblem hipMalloc d_neid failed");
                GR_CHECK(hipMalloc(&d_up, sizeof(int) * (n1 + 1)), "TrussProblem hipMalloc failed");
                GR_CHECK(hipMalloc(&d_low, sizeof(int) * (n1 + 1)), "TrussProblem hipMalloc failed");
                GR_CHECK(hipMalloc(&d_deg, sizeof(unsigned) * (n1 + 1)), "TrussProblem hipMalloc failed");
                hipLaunchKernelGGL(CanonicalKernel, dim3(Grid(m)), dim3(256), 0, stream, d_sorted, d_keep, d_pos, m, col_bits, d_ckeys, ds->d_src,
                                   ds->d_dst);
                GR_CHECK(hipGetLastError(), "CanonicalKernel launch failed");
                // (the sort's buffers are free again: the canonical keys are in their own array)
                hipLaunchKernelGGL(SwapKeysKernel, dim3(Grid(M)), dim3(256), 0, stream, d_ckeys, M, col_bits, edge_sort.Keys());
                GR_CHECK(hipGetLastError(), "SwapKeysKernel launch failed");
                unsigned long long *d_skeys = nullptr;
                GR_CHECK(edge_sort.Sort(M, key_bits, stream, &d_skeys), "TrussProblem edge sort failed");
                hipLaunchKernelGGL(RowStartsKernel, dim3(Grid(n + 1)), dim3(256), 0, stream, d_ckeys, d_skeys, M, n, col_bits, d_up, d_low);
                GR_CHECK(hipGetLastError(), "RowStartsKernel launch failed");
                hipLaunchKernelGGL(DegreesKernel, dim3(Grid(n + 1)), dim3(256), 0, stream, d_up, d_low, n, d_deg);
                GR_CHECK(hipGetLastError(), "DegreesKernel launch failed");
                GR_CHECK(graphio::DeviceExclusiveScan<int>(d_deg, ds->d_nro, n + 1, d_sums, stream), "TrussProblem offset scan failed");
                hipLaunchKernelGGL(FillRowsKernel, dim3(Grid(M)), dim3(256), 0, stream, d_ckeys, d_skeys, M, col_bits, d_up, d_low, ds->d_nro,
                                   ds->d_nci, ds->d_neid);
                GR_CHECK(hipGetLastError(), "FillRowsKernel launch failed");
            }
        }
        simple_edges = M;
        const size_t m1 = static_cast<size_t>(M > 0 ? M : 1);
        GR_CHECK(hipMalloc(&ds->d_support, sizeof(int) * m1), "TrussProblem hipMalloc d_support failed");
        GR_CHECK(hipMalloc(&ds->d_val, sizeof(int) * m1), "TrussProblem hipMalloc d_val failed");
        GR_CHECK(hipMalloc(&ds->d_stamp, sizeof(int) * m1), "TrussProblem hipMalloc d_stamp failed");
        GR_CHECK(hipMalloc(&ds->d_truss, sizeof(int) * m1), "TrussProblem hipMalloc d_truss failed");
        GR_CHECK(hipMalloc(&ds->d_queue, sizeof(int) * m1), "TrussProblem hipMalloc d_queue failed");
        GR_CHECK(hipMemsetAsync(ds->d_support, 0, sizeof(int) * m1, stream), "TrussProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_truss, 0, sizeof(int) * m1, stream), "TrussProblem memset failed");
        GR_CHECK(hipEventRecord(ev[1], stream), "TrussProblem hipEventRecord failed");

        unsigned summary[2] = {0u, kNoLevel};
        unsigned *d_out = ds->d_words + W_COUNT;
        GR_CHECK(hipMemcpyAsync(d_out, summary, sizeof(summary), hipMemcpyHostToDevice, stream), "TrussProblem summary init failed");
        if (M > 0) {
            hipLaunchKernelGGL(SupportKernel, dim3(Grid(M)), dim3(kTrussThreads), 0, stream, DeviceGraph(), M, wave_min_row, ds->d_support,
                               ds->d_counters + 4);
            GR_CHECK(hipGetLastError(), "SupportKernel launch failed");
            hipLaunchKernelGGL(SupportSummaryKernel, dim3(Grid(M)), dim3(256), 0, stream, ds->d_support, M, d_out, ds->d_counters + 5);
            GR_CHECK(hipGetLastError(), "SupportSummaryKernel launch failed");
        }
        GR_CHECK(hipEventRecord(ev[2], stream), "TrussProblem hipEventRecord failed");
        unsigned long long sums[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(summary, d_out, sizeof(summary), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
        GR_CHECK(hipMemcpyAsync(sums, ds->d_counters + 4, sizeof(sums), hipMemcpyDeviceToHost, stream), "TrussProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "TrussProblem build sync failed");
        float ms = 0;
        GR_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]), "TrussProblem hipEventElapsedTime failed");
        build_ms = ms;
        GR_CHECK(hipEventElapsedTime(&ms, ev[1], ev[2]), "TrussProblem hipEventElapsedTime failed");
        support_ms = ms;
        for (int i = 0; i < 3; ++i) hipEventDestroy(ev[i]);
        max_support = summary[0];
        min_support = summary[1] == kNoLevel ? 0 : summary[1];
        support_entries = static_cast<long long>(sums[0]);
        triangles = static_cast<long long>(sums[1] / 3);
        trace_capacity = max_support + 2;
        GR_CHECK(hipMalloc(&ds->d_trace_k, sizeof(int) * static_cast<size_t>(trace_capacity)), "TrussProblem hipMalloc failed");
        GR_CHECK(hipMalloc(&ds->d_trace_tail, sizeof(int) * static_cast<size_t>(trace_capacity)), "TrussProblem hipMalloc failed");
        GR_CHECK(hipMalloc(&ds->d_trace_clock, sizeof(unsigned long long) * static_cast<size_t>(trace_capacity)), "TrussProblem hipMalloc failed");
        void *scratch[] = {d_keep, d_pos, d_sums, d_ckeys, d_up, d_low, d_deg};
        for (void *b : scratch)
            if (b) GR_CHECK(hipFree(b), "TrussProblem hipFree failed");
        return retval;
    }

    // One Init per object (grx_truss_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, false))) return retval;
        data_slices = new DataSlice *[1];
        data_slices[0] = new DataSlice();
        return Build();
    }

    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        data_slices = new DataSlice *[1];
        data_slices[0] = new DataSlice();
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
            hipLaunchKernelGGL(SupportSummaryKernel, dim3(Grid(simple_edges)), dim3(256), 0, stream, ds->d_truss, simple_edges, d_out,
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
            if (ds->d_classes) GR_CHECK(hipFree(ds->d_classes), "TrussProblem hipFree failed");
            ds->d_classes = nullptr;
            GR_CHECK(hipMalloc(&ds->d_classes, sizeof(unsigned long long) * static_cast<size_t>(classes)), "TrussProblem hipMalloc d_classes failed");
            class_capacity = classes;
        }
        GR_CHECK(hipMemsetAsync(ds->d_classes, 0, sizeof(unsigned long long) * static_cast<size_t>(classes), stream), "TrussProblem memset failed");
        if (simple_edges > 0) {  // (k-core's kernel: the lanes of a wave that hold the same value add once)
            hipLaunchKernelGGL(kcore::ShellKernel, dim3(Grid(simple_edges)), dim3(256), 0, stream, ds->d_truss, simple_edges, ds->d_classes);
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
        if (!ds->d_mask) GR_CHECK(hipMalloc(&ds->d_mask, M > 0 ? M : 1), "TrussProblem hipMalloc d_mask failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters + 1, 0, sizeof(unsigned long long) * 2, stream), "TrussProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_vertex, 0, sizeof(int) * static_cast<size_t>(this->nodes), stream), "TrussProblem memset failed");
        if (M > 0) {
            hipLaunchKernelGGL(MemberEdgesKernel, dim3(Grid(simple_edges)), dim3(256), 0, stream, DeviceGraph(), ds->d_truss, simple_edges, k,
                               ds->d_mask, ds->d_vertex, ds->d_counters + 1);
            GR_CHECK(hipGetLastError(), "MemberEdgesKernel launch failed");
            hipLaunchKernelGGL(CountFlagsKernel, dim3(Grid(this->nodes)), dim3(256), 0, stream, ds->d_vertex, static_cast<long long>(this->nodes),
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
            hipLaunchKernelGGL(VertexTrussKernel, dim3(Grid(simple_edges)), dim3(256), 0, stream, DeviceGraph(), ds->d_truss, simple_edges,
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
