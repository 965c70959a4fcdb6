// app/mis/mis_problem.hpp -- device data for the maximal independent set / greedy colourings.
//
// Stands for the reference's MISProblem (gunrock/app/mis/mis_problem.cuh:41-360):
//   DataSlice { d_labels (the random permutation), d_mis_ids (the colours), d_values_to_reduce, d_reduced_values }   (:64-78)
//   Init(stream_from_host, graph, num_gpus)                                                                          (:145-310)
//   Reset(frontier_type): ids = -1, labels shuffled                                                                  (:320-346)
//   Extract(h_mis_ids)                                                                                               (:106-140)
// Differences: the input is read as an undirected simple graph of any shape (u and v are neighbours when either row holds
// the other; self-loops ignored; unsorted rows and duplicates allowed): Init runs the exact symmetry test and builds the
// in-neighbour CSR when the answer is no.  The order is key(v) = (prio(v), v), prio the caller's int32 array or a seeded hash
// (mis_functor.hpp), so ties cannot occur and every result is unique.  Enact runs to completion: no -1 remains.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/mis/mis_functor.hpp>
#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/pair_graph.hpp>
#include <gunrock/graphio/symmetry.hpp>

namespace gunrock {
namespace app {
namespace mis {

template <bool _USE_DOUBLE_BUFFER>
struct MISProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;
    typedef int VertexId;
    typedef int SizeT;
    typedef int Value;

    struct DataSlice {
        DeviceArray<int> d_mis_ids;  // the result (reference d_mis_ids); the colourings' state table
        DeviceArray<unsigned char> d_state;  // the set's state table: 0 undecided, 1 in, 2 out
        DeviceArray<int> d_own_priorities;  // the copy of the priorities a host Init gave
        int *d_priorities = nullptr;             // caller priorities (that copy, or borrowed with the device CSR), or NULL: hashed
        DeviceArray<int> d_pos;  // cursors (mis_functor.hpp State)
        DeviceArray<int> d_acc;
        DeviceArray<unsigned long long> d_mask;
        DeviceArray<int> d_list[2];  // the worklist of undecided vertices, double-buffered
        DeviceArray<int> d_words;  // [0], [1] worklist lengths
        DeviceArray<int> d_tail_words;  // [0] undecided after a tail pass; per window [1 + 2w] its undecided, [2 + 2w] its sweeps
        DeviceArray<unsigned long long> d_reads; // [0] row entries walked; [1], [2] Extract's sum and maximum of ids; [3] polls
        DeviceArray<int> d_inv_row_offsets;  // in-neighbour CSR of an asymmetric input (owned)
        DeviceArray<int> d_inv_column_indices;
    };

    SliceHolder<DataSlice> data_slices;
    int symmetric = 0;      // every edge has its mirror (sorted duplicate-free rows): a row is the whole neighbourhood
    unsigned seed = 0;
    int mode = MIS_SET;     // of the last Enact: Extract's summary is the set size or the number of colours
    long long summary = 0;
    util::PinnedArray<int> h_words;        // pinned read-back words
    util::PinnedArray<int> h_tail_words;   // pinned copy of d_tail_words
    long long tail_windows = 0;            // windows d_tail_words has room for
    graphio::DeviceKeySort order_sort;     // orders the tail's worklist by key (scratch allocated at the first use)

    // `count` device words read back (pinned), count <= 4
    hipError_t ReadWords(const int *d_from, int count, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(hipMemcpyAsync(h_words, d_from, sizeof(int) * count, hipMemcpyDeviceToHost, stream), "MISProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "MISProblem read-back sync failed");
        return retval;
    }

    // room for the counters of `windows` tail windows
    hipError_t ReserveTail(long long windows)
    {
        hipError_t retval = hipSuccess;
        if (windows <= tail_windows) return retval;
        DataSlice *ds = data_slices[0];
        h_tail_words.Free();
        tail_windows = 0;
        const size_t words = static_cast<size_t>(2 * windows + 1);
        if ((retval = ds->d_tail_words.Alloc(words))) return retval;
        if ((retval = h_tail_words.Alloc(words))) return retval;
        tail_windows = windows;
        return retval;
    }

    Graph DeviceGraph() const
    {
        const GraphSlice<int, int, int> *gs = this->graph_slices[0];
        const DataSlice *ds = data_slices[0];
        return Graph{gs->d_row_offsets, gs->d_column_indices, ds->d_inv_row_offsets, ds->d_inv_column_indices};
    }
    Keys DeviceKeys() const { return Keys{data_slices[0]->d_priorities, seed * 0x9E3779B9u}; }
    State DeviceState() const
    {
        const DataSlice *ds = data_slices[0];
        return State{ds->d_state, ds->d_mis_ids, ds->d_pos, ds->d_acc, ds->d_mask};
    }

    hipError_t AllocData()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = h_words.Alloc(4))) return retval;
        if ((retval = ds->d_words.Alloc(4))) return retval;
        if ((retval = ds->d_reads.Alloc(4))) return retval;

        // 1. the CSR must be one: nothing in the sweeps indexes with an unchecked value
        if ((retval = this->ValidateCsr())) return retval;

        // 2. is a row the whole neighbourhood?  (exact test, graphio/symmetry.hpp; "no" for unsorted rows and duplicates too)
        symmetric = 0;
        if (m > 0) {
            bool yes = false;
            GR_CHECK(graphio::DeviceIsSymmetric(static_cast<int>(n), m, gs->d_row_offsets, gs->d_column_indices, stream, yes),
                     "MISProblem symmetry test failed");
            symmetric = yes ? 1 : 0;
            if (!yes) {
                if ((retval = ds->d_inv_row_offsets.Alloc(n1 + 1))) return retval;
                if ((retval = ds->d_inv_column_indices.Alloc(static_cast<size_t>(m)))) return retval;
                GR_CHECK(graphio::DeviceTransposeCsr(static_cast<int>(n), m, gs->d_row_offsets, gs->d_column_indices, ds->d_inv_row_offsets,
                                                     ds->d_inv_column_indices, stream),
                         "MISProblem transpose failed");
            }
        }

        if ((retval = ds->d_mis_ids.Alloc(n1))) return retval;
        if ((retval = ds->d_state.Alloc(n1))) return retval;
        if ((retval = ds->d_pos.Alloc(n1))) return retval;
        if ((retval = ds->d_acc.Alloc(n1))) return retval;
        if ((retval = ds->d_mask.Alloc(n1))) return retval;
        if ((retval = ds->d_list[0].Alloc(n1))) return retval;
        if ((retval = ds->d_list[1].Alloc(n1))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "MISProblem AllocData failed");
        return retval;
    }

    // One Init per object (grx_mis_init refuses a second one: the buffers of the first would be lost).
    // h_priorities may be NULL: then prio(v) = fmix32(v + seed * 0x9E3779B9), compared as unsigned
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, const int *h_priorities, unsigned seed_, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, false))) return retval;
        seed = seed_;
        data_slices.Make();
        if (h_priorities) {
            DataSlice *ds = data_slices[0];
            if ((retval = ds->d_own_priorities.Alloc(static_cast<size_t>(graph.nodes)))) return retval;
            ds->d_priorities = ds->d_own_priorities;
            GR_CHECK(hipMemcpy(ds->d_priorities, h_priorities, sizeof(int) * static_cast<size_t>(graph.nodes), hipMemcpyHostToDevice),
                     "MISProblem hipMemcpy d_priorities failed");
        }
        return AllocData();
    }

    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_priorities, unsigned seed_)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        seed = seed_;
        data_slices.Make();
        data_slices[0]->d_priorities = d_priorities;
        return AllocData();
    }

    // every vertex undecided (the reference sets ids to -1 and reshuffles the labels; here the order is part of the input)
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t n = static_cast<size_t>(this->nodes);
        GR_CHECK(hipMemsetAsync(ds->d_mis_ids, 0, sizeof(int) * n, stream), "MISProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_state, 0, n, stream), "MISProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(int) * 4, stream), "MISProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_reads, 0, sizeof(unsigned long long) * 4, stream), "MISProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "MISProblem Reset sync failed");
        summary = 0;
        return retval;
    }

    // h_mis_ids may be NULL: then only the summary (size of the set, or number of colours) is computed
    hipError_t Extract(int *h_mis_ids)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        unsigned long long out[2] = {0, 0};
        GR_CHECK(hipMemsetAsync(ds->d_reads + 1, 0, sizeof(unsigned long long) * 2, stream), "MISProblem memset failed");
        hipLaunchKernelGGL(SummaryKernel, dim3(graphio::PairGrid(this->nodes)), dim3(256), 0, stream, ds->d_mis_ids, static_cast<long long>(this->nodes),
                           ds->d_reads + 1);
        GR_CHECK(hipGetLastError(), "SummaryKernel launch failed");
        GR_CHECK(hipMemcpyAsync(out, ds->d_reads + 1, sizeof(out), hipMemcpyDeviceToHost, stream), "MISProblem read summary failed");
        if (h_mis_ids)
            GR_CHECK(hipMemcpyAsync(h_mis_ids, ds->d_mis_ids, sizeof(int) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost, stream),
                     "MISProblem read d_mis_ids failed");
        GR_CHECK(hipStreamSynchronize(stream), "MISProblem Extract sync failed");
        summary = static_cast<long long>(mode == MIS_SET ? out[0] : out[1]);
        return retval;
    }
};

}  // namespace mis
}  // namespace app
}  // namespace gunrock
