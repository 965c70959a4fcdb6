// app/wl/wl_problem.hpp -- device data for colour refinement.
//
// The reference snapshot has no app/wl; the shape is app/lp/lp_problem.hpp's.  The input CSR is taken as given and read by every
// round (a CSR given in device memory is borrowed for the life of the handle).  Init validates it and allocates the per-vertex arrays
// and the grouping table of at least 2 n slots.  Reset takes the start labels, any int32 values (NULL: one class).  Finish turns the
// working colours -- the smallest member of every class -- into the dense ids by ascending smallest member with the device scan, and
// fills the class sizes and the representatives; History does the same for a round the Enact kept.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/wl/wl_functor.hpp>
#include <gunrock/graphio/device_csr.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace wl {

template <bool _USE_DOUBLE_BUFFER>
struct WlProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_start;  // the labels of the last Reset
        DeviceArray<int> d_colour[3];  // c, c' and a refused attempt at c' (the enactor rotates them)
        DeviceArray<Sig> d_sig;
        DeviceArray<unsigned long long> d_slot;
        DeviceArray<int> d_owner;
        DeviceArray<unsigned> d_smallest;
        DeviceArray<int> d_waves, d_hubs, d_block_list, d_global_list;
        DeviceArray<int> d_dense, d_representative;
        DeviceArray<unsigned long long> d_size;
        DeviceArray<unsigned long long> d_words;
        Grown<int> history;  // (rounds + 1) x n working colours, when asked for
        Grown<int> rows;     // the GLOBAL rung's counter rows, all 0 between launches
    };

    SliceHolder<DataSlice> data_slices;
    int longest_row = 0;
    unsigned long long table_slots = 0;  // a power of two, at least 2 n
    bool labelled = false;               // the last Reset gave labels
    bool enacted = false;                // the arrays hold a result
    int current = 0;                     // d_colour[current] is c
    long long classes = 0;               // of the last Enact
    int history_rounds = -1;             // history[0 .. history_rounds] is kept, or -1

    // the slots of the grouping table of n vertices: the smallest power of two that is at least 2 n (at least 64)
    static unsigned long long TableSlots(long long n)
    {
        unsigned long long slots = 64;
        while (slots < 2ull * static_cast<unsigned long long>(n)) slots <<= 1;
        return slots;
    }

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "WlProblem memset failed");

        if ((retval = this->ValidateCsr())) return retval;
        unsigned long long longest = 0;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long), stream), "WlProblem memset failed");
        hipLaunchKernelGGL(LongestKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, gs->d_row_offsets, n, ds->d_words);
        GR_CHECK(hipGetLastError(), "LongestKernel launch failed");
        GR_CHECK(hipMemcpyAsync(&longest, ds->d_words, sizeof(longest), hipMemcpyDeviceToHost, stream), "WlProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "WlProblem build sync failed");
        longest_row = static_cast<int>(longest);

        table_slots = TableSlots(n);
        DeviceArray<int> *vertex_arrays[] = {&ds->d_start, &ds->d_colour[0], &ds->d_colour[1], &ds->d_colour[2], &ds->d_waves, &ds->d_hubs, &ds->d_block_list, &ds->d_global_list,
                                 &ds->d_dense, &ds->d_representative};
        for (DeviceArray<int> *a : vertex_arrays) if ((retval = a->Alloc(n1))) return retval;
        if ((retval = ds->d_sig.Alloc(n1))) return retval;
        if ((retval = ds->d_slot.Alloc(n1))) return retval;
        if ((retval = ds->d_size.Alloc(n1))) return retval;
        if ((retval = ds->d_owner.Alloc(static_cast<size_t>(table_slots)))) return retval;
        if ((retval = ds->d_smallest.Alloc(static_cast<size_t>(table_slots)))) return retval;
        return retval;
    }

    // One Init per object (grx_wl_init refuses a second one)
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

    // h_labels: any int32 per vertex, or NULL for one class
    hipError_t Reset(const int *h_labels = nullptr)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if (h_labels) {
            GR_CHECK(hipMemcpyAsync(ds->d_start, h_labels, sizeof(int) * static_cast<size_t>(this->nodes), hipMemcpyHostToDevice, stream),
                     "WlProblem upload failed");
            GR_CHECK(hipStreamSynchronize(stream), "WlProblem Reset sync failed");  // (h_labels is the caller's again)
        }
        labelled = h_labels != nullptr;
        enacted = false;
        classes = 0;
        history_rounds = -1;
        return retval;
    }

    // the grouping table empty
    hipError_t ClearTable(hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GR_CHECK(hipMemsetAsync(ds->d_owner, 0xFF, sizeof(int) * static_cast<size_t>(table_slots), stream), "WlProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_smallest, 0xFF, sizeof(unsigned) * static_cast<size_t>(table_slots), stream), "WlProblem memset failed");
        return retval;
    }

    // dense[] (and with `full` d_size[], d_representative[]) from the working colours `colour`; *count: the classes
    hipError_t Densify(const int *colour, int *dense, bool full, long long *count)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        const long long tiles = (n + graphio::kScanTile - 1) / graphio::kScanTile;
        graphio::DeviceScratch<unsigned> flag;
        graphio::DeviceScratch<unsigned long long> sums;
        graphio::DeviceScratch<int> rank;
        if ((retval = flag.Alloc(static_cast<size_t>(n)))) return retval;
        if ((retval = rank.Alloc(static_cast<size_t>(n)))) return retval;
        if ((retval = sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(n))))) return retval;
        hipLaunchKernelGGL(LeaderFlagKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, colour, n, flag.p);
        GR_CHECK(hipGetLastError(), "LeaderFlagKernel launch failed");
        GR_CHECK(graphio::DeviceExclusiveScan<int>(flag.p, rank.p, n, sums.p, stream), "WlProblem rank scan failed");
        if (full) GR_CHECK(hipMemsetAsync(ds->d_size, 0, sizeof(unsigned long long) * static_cast<size_t>(n), stream), "WlProblem memset failed");
        hipLaunchKernelGGL(DenseKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, colour, rank.p, n, dense, full ? ds->d_size : nullptr,
                           full ? ds->d_representative : nullptr);
        GR_CHECK(hipGetLastError(), "DenseKernel launch failed");
        unsigned long long total = 0;
        GR_CHECK(hipMemcpyAsync(&total, sums.p + tiles, sizeof(total), hipMemcpyDeviceToHost, stream), "WlProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "WlProblem Densify sync failed");  // (the scratch goes with this scope)
        *count = static_cast<long long>(total);
        return retval;
    }

    hipError_t Finish() { return Densify(data_slices[0]->d_colour[current], data_slices[0]->d_dense, true, &classes); }

    // every pointer may be NULL
    hipError_t Extract(int *h_colour, long long *h_size, int *h_representative)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if ((retval = this->Read(h_colour, ds->d_dense.p, static_cast<size_t>(this->nodes)))) return retval;
        if ((retval = this->Read(reinterpret_cast<unsigned long long *>(h_size), ds->d_size.p, static_cast<size_t>(classes)))) return retval;
        return this->Read(h_representative, ds->d_representative.p, static_cast<size_t>(classes));
    }

    // the dense colouring behind round h of the last Enact, h in 0 .. history_rounds (checked by the caller)
    hipError_t History(int h, int *h_colour, long long *count)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        long long c = 0;
        graphio::DeviceScratch<int> dense;
        if ((retval = dense.Alloc(static_cast<size_t>(this->nodes)))) return retval;
        if ((retval = Densify(ds->history.p + static_cast<size_t>(h) * static_cast<size_t>(this->nodes), dense.p, false, &c))) return retval;
        if (count) *count = c;
        return this->Read(h_colour, dense.p, static_cast<size_t>(this->nodes));
    }
};

}  // namespace wl
}  // namespace app
}  // namespace gunrock
