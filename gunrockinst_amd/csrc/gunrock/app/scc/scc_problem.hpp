// app/scc/scc_problem.hpp -- device data for the strongly connected components.
//
// The reference snapshot has no app/scc; the shape is this tree's Problem (compare app/kcore/kcore_problem.hpp).  The input CSR is
// read as a directed multigraph: duplicates and self-loops allowed (and without effect), rows unsorted, nothing symmetrised.  Init
// validates it as the other families do and builds the transpose on the device (graphio::DeviceTransposeCsr) unless the caller
// lends one.  The per-vertex arrays are scc_functor.hpp's; comp[] holds representatives while Enact runs and the smallest id of
// the component after it.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/scc/scc_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace scc {

template <bool _USE_DOUBLE_BUFFER>
struct SccProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_built_iro, d_built_ici;  // the transpose built here
        int *d_iro = nullptr, *d_ici = nullptr;     // the transpose the kernels read (that one, or the caller's)
        DeviceArray<int> d_region, d_outdeg, d_indeg, d_colour, d_mark, d_comp;
        DeviceArray<int> d_list[2];
        DeviceArray<int> d_queue[2];
        DeviceArray<int> d_size;  // allocated at the first request
        DeviceArray<unsigned> d_words;
        DeviceArray<unsigned long long> d_counters;  // [0] row entries walked, [1] the end of the trace's clock, [2..4] SummaryKernel's
        DeviceArray<State> d_state;  // LoopKernel's state on return
        DeviceArray<int> d_trace_kind;
        DeviceArray<unsigned> d_trace_finished;
        DeviceArray<unsigned long long> d_trace_clock;
    };

    SliceHolder<DataSlice> data_slices;
    bool fresh = false;    // Reset has run and Enact has not
    bool sizes_valid = false;
    double build_ms = 0;   // HIP-event time of the transpose (0 for a borrowed one)

    Ctx DeviceCtx(int wave_min_row) const
    {
        const DataSlice *ds = data_slices[0];
        const GraphSlice<int, int, int> *gs = this->graph_slices[0];
        Ctx c;
        c.ro = gs->d_row_offsets;
        c.ci = gs->d_column_indices;
        c.iro = ds->d_iro;
        c.ici = ds->d_ici;
        c.region = ds->d_region;
        c.outdeg = ds->d_outdeg;
        c.indeg = ds->d_indeg;
        c.colour = ds->d_colour;
        c.mark = ds->d_mark;
        c.comp = ds->d_comp;
        c.list[0] = ds->d_list[0];
        c.list[1] = ds->d_list[1];
        c.queue[0] = ds->d_queue[0];
        c.queue[1] = ds->d_queue[1];
        c.words = ds->d_words;
        c.reads = ds->d_counters;
        c.trace_kind = ds->d_trace_kind;
        c.trace_finished = ds->d_trace_finished;
        c.trace_clock = ds->d_trace_clock;
        c.nodes = this->nodes;
        c.wave_min_row = wave_min_row;
        return c;
    }

    hipError_t Build(int *d_inv_row_offsets, int *d_inv_col_indices)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1), m1 = static_cast<size_t>(m > 0 ? m : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        if ((retval = ds->d_counters.Alloc(5))) return retval;
        if ((retval = ds->d_state.Alloc(1))) return retval;

        // CSRs of `nodes` vertices?  (the kernels index with what they read)
        if ((retval = this->ValidateCsr())) return retval;
        if (d_inv_row_offsets && (retval = this->ValidateCsr(d_inv_row_offsets, d_inv_col_indices))) return retval;

        if (d_inv_row_offsets) {
            ds->d_iro = d_inv_row_offsets;
            ds->d_ici = d_inv_col_indices;
            build_ms = 0;
        } else {
            hipEvent_t ev[2] = {nullptr, nullptr};
            GR_CHECK(hipEventCreate(&ev[0]), "SccProblem hipEventCreate failed");
            GR_CHECK(hipEventCreate(&ev[1]), "SccProblem hipEventCreate failed");
            GR_CHECK(hipEventRecord(ev[0], stream), "SccProblem hipEventRecord failed");
            if ((retval = ds->d_built_iro.Alloc(n1 + 1))) return retval;
            if ((retval = ds->d_built_ici.Alloc(m1))) return retval;
            ds->d_iro = ds->d_built_iro;
            ds->d_ici = ds->d_built_ici;
            GR_CHECK(graphio::DeviceTransposeCsr(static_cast<int>(n), m, gs->d_row_offsets, gs->d_column_indices, ds->d_iro, ds->d_ici, stream),
                     "SccProblem transpose failed");
            GR_CHECK(hipEventRecord(ev[1], stream), "SccProblem hipEventRecord failed");
            GR_CHECK(hipStreamSynchronize(stream), "SccProblem build sync failed");
            float ms = 0;
            GR_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]), "SccProblem hipEventElapsedTime failed");
            build_ms = ms;
            hipEventDestroy(ev[0]);
            hipEventDestroy(ev[1]);
        }

        DeviceArray<int> *arrays[] = {&ds->d_region, &ds->d_outdeg, &ds->d_indeg, &ds->d_colour, &ds->d_mark, &ds->d_comp, &ds->d_list[0], &ds->d_list[1],
                          &ds->d_queue[0], &ds->d_queue[1]};
        for (DeviceArray<int> *a : arrays) if ((retval = a->Alloc(n1))) return retval;
        // no representative yet: a result asked for before the first Enact finds every entry negative, which the result kernels
        // skip, and never an index taken from fresh memory
        GR_CHECK(hipMemsetAsync(ds->d_comp, 0xFF, sizeof(int) * n1, stream), "SccProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "SccProblem build sync failed");
        if ((retval = ds->d_trace_kind.Alloc(kTraceRows))) return retval;
        if ((retval = ds->d_trace_finished.Alloc(kTraceRows))) return retval;
        if ((retval = ds->d_trace_clock.Alloc(kTraceRows))) return retval;
        return retval;
    }

    // One Init per object (grx_scc_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, false))) return retval;
        data_slices.Make();
        return Build(nullptr, nullptr);
    }

    // the inverse arrays: both or neither
    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_inv_row_offsets = nullptr,
                              int *d_inv_col_indices = nullptr)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        data_slices.Make();
        return Build(d_inv_row_offsets, d_inv_col_indices);
    }

    // every vertex live in region 0, no mark, no representative, the words at 0 (the live degrees are the first step of Enact:
    // they are counted within regions, and so again after every split)
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t bytes = sizeof(int) * static_cast<size_t>(this->nodes);
        GR_CHECK(hipMemsetAsync(ds->d_region, 0, bytes, stream), "SccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_mark, 0, bytes, stream), "SccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_outdeg, 0, bytes, stream), "SccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_indeg, 0, bytes, stream), "SccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_comp, 0xFF, bytes, stream), "SccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * W_COUNT, stream), "SccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(unsigned long long) * 5, stream), "SccProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "SccProblem Reset sync failed");
        fresh = true;
        sizes_valid = false;
        return retval;
    }

    // comp[] from representatives to smallest ids (Enact's last step; colour[] is free by then)
    hipError_t Canonical()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        hipLaunchKernelGGL(IotaKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_colour, n);
        GR_CHECK(hipGetLastError(), "IotaKernel launch failed");
        hipLaunchKernelGGL(MergeKernel<false>, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_comp, n, ds->d_colour);
        GR_CHECK(hipGetLastError(), "MergeKernel launch failed");
        hipLaunchKernelGGL(GatherKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_comp, n, ds->d_colour, ds->d_comp);
        GR_CHECK(hipGetLastError(), "GatherKernel launch failed");
        return retval;
    }

    // size[v] on the device (colour[] counts)
    hipError_t DeviceSizes()
    {
        hipError_t retval = hipSuccess;
        if (sizes_valid) return retval;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        if (!ds->d_size && (retval = ds->d_size.Alloc(static_cast<size_t>(n)))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_colour, 0, sizeof(int) * static_cast<size_t>(n), stream), "SccProblem memset failed");
        hipLaunchKernelGGL(MergeKernel<true>, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_comp, n, ds->d_colour);
        GR_CHECK(hipGetLastError(), "MergeKernel launch failed");
        hipLaunchKernelGGL(GatherKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_comp, n, ds->d_colour, ds->d_size);
        GR_CHECK(hipGetLastError(), "GatherKernel launch failed");
        sizes_valid = true;
        return retval;
    }

    hipError_t Sizes(int *h_size)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if ((retval = DeviceSizes())) return retval;
        GR_CHECK(hipMemcpyAsync(h_size, ds->d_size, sizeof(int) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost, stream),
                 "SccProblem read d_size failed");
        GR_CHECK(hipStreamSynchronize(stream), "SccProblem Sizes sync failed");
        return retval;
    }

    // the largest component's root: ties go to the smaller one
    hipError_t Summary(long long *components, long long *trivial, long long *largest, int *largest_root)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if ((retval = DeviceSizes())) return retval;
        unsigned long long out[3] = {0, 0, 0};
        GR_CHECK(hipMemsetAsync(ds->d_counters + 2, 0, sizeof(out), stream), "SccProblem memset failed");
        hipLaunchKernelGGL(SummaryKernel, dim3(graphio::PairGrid(this->nodes)), dim3(256), 0, stream, ds->d_comp, ds->d_size, static_cast<long long>(this->nodes),
                           ds->d_counters + 2);
        GR_CHECK(hipGetLastError(), "SummaryKernel launch failed");
        GR_CHECK(hipMemcpyAsync(out, ds->d_counters + 2, sizeof(out), hipMemcpyDeviceToHost, stream), "SccProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "SccProblem Summary sync failed");
        if (components) *components = static_cast<long long>(out[0]);
        if (trivial) *trivial = static_cast<long long>(out[1]);
        if (largest) *largest = static_cast<long long>(out[2] >> 32);
        if (largest_root) *largest_root = static_cast<int>(0xFFFFFFFFu - static_cast<unsigned>(out[2] & 0xFFFFFFFFull));
        return retval;
    }

    // h_comp may be NULL: then only the number of components is read
    hipError_t Extract(int *h_comp, long long *components)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if ((retval = Summary(components, nullptr, nullptr, nullptr))) return retval;
        if (h_comp) {
            GR_CHECK(hipMemcpyAsync(h_comp, ds->d_comp, sizeof(int) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost, stream),
                     "SccProblem read d_comp failed");
            GR_CHECK(hipStreamSynchronize(stream), "SccProblem Extract sync failed");
        }
        return retval;
    }

    // the distinct pairs (comp[u], comp[v]) of the edges between components, sorted by (from, to); the first max_edges of them
    // go to h_from / h_to, *count is how many there are
    hipError_t Condensation(long long max_edges, int *h_from, int *h_to, long long *count)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        *count = 0;
        if (m == 0) return retval;
        int col_bits = 1;
        while ((1ll << col_bits) < n) ++col_bits;
        const int key_bits = 2 * col_bits;  // <= 62
        const unsigned long long sentinel = (1ull << key_bits) - 1ull;  // from = to = 2^cb - 1: never a pair
        graphio::DeviceKeySort sort;
        graphio::DeviceScratch<unsigned> d_keep;
        graphio::DeviceScratch<unsigned long long> d_pos, d_sums;
        graphio::DeviceScratch<int> d_from, d_to;
        GR_CHECK(sort.Reserve(m), "SccProblem sort scratch failed");
        if ((retval = d_keep.Alloc(static_cast<size_t>(m)))) return retval;
        if ((retval = d_pos.Alloc(static_cast<size_t>(m)))) return retval;
        if ((retval = d_sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(m))))) return retval;
        hipLaunchKernelGGL(CondensationKeysKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices, ds->d_comp,
                           static_cast<int>(n), m, col_bits, sentinel, sort.Keys());
        GR_CHECK(hipGetLastError(), "CondensationKeysKernel launch failed");
        unsigned long long *d_sorted = nullptr;
        GR_CHECK(sort.Sort(m, key_bits, stream, &d_sorted), "SccProblem key sort failed");
        hipLaunchKernelGGL(graphio::FlagKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, d_sorted, m, sentinel, d_keep);
        GR_CHECK(hipGetLastError(), "FlagKernel launch failed");
        GR_CHECK(graphio::DeviceExclusiveScan<unsigned long long>(d_keep.p, d_pos.p, m, d_sums.p, stream), "SccProblem flag scan failed");
        // the total is behind the tile offsets (DeviceCooToCsr reads it from there too)
        const long long scan_tiles = (m + graphio::kScanTile - 1) / graphio::kScanTile;
        unsigned long long total = 0;
        GR_CHECK(hipMemcpyAsync(&total, d_sums + scan_tiles, sizeof(total), hipMemcpyDeviceToHost, stream), "SccProblem read total failed");
        GR_CHECK(hipStreamSynchronize(stream), "SccProblem Condensation sync failed");
        *count = static_cast<long long>(total);
        const long long take = *count < max_edges ? *count : max_edges;
        if (take < 1 || !h_from || !h_to) return retval;
        if ((retval = d_from.Alloc(static_cast<size_t>(take)))) return retval;
        if ((retval = d_to.Alloc(static_cast<size_t>(take)))) return retval;
        hipLaunchKernelGGL(CondensationEmitKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, d_sorted, d_keep, d_pos, m, col_bits, take, d_from, d_to);
        GR_CHECK(hipGetLastError(), "CondensationEmitKernel launch failed");
        GR_CHECK(hipMemcpyAsync(h_from, d_from, sizeof(int) * static_cast<size_t>(take), hipMemcpyDeviceToHost, stream), "SccProblem read failed");
        GR_CHECK(hipMemcpyAsync(h_to, d_to, sizeof(int) * static_cast<size_t>(take), hipMemcpyDeviceToHost, stream), "SccProblem read failed");
        GR_CHECK(hipStreamSynchronize(stream), "SccProblem Condensation sync failed");
        return retval;
    }
};

}  // namespace scc
}  // namespace app
}  // namespace gunrock
