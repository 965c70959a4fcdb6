// app/lp/lp_problem.hpp -- device data for label propagation: the pairs and the neighbour CSR, the labels, the class lists.
//
// The reference snapshot has no label propagation; the shape is this tree's Problem (compare app/matching/matching_problem.hpp, whose
// weight kernels are used as they are).  The input CSR is read as matching reads it: the simple undirected graph G with int weights in
// edge_values (NULL: 1 each); Init validates it, builds the canonical pairs and the neighbour CSR with graphio::PairGraph, gives a
// pair the largest weight of its entries and refuses a pair weight below 1.  SetClasses validates a proper colouring over the pairs
// and builds the class lists (the vertex ids grouped by class) with the in-tree sort.  Finish ranks the labels in use into the dense
// community ids; Summary adds up sizes, internal weights and volumes per community on demand.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/app/lp/lp_functor.hpp>
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // (only matching's weight kernels are used here)
#include <gunrock/app/matching/matching_functor.hpp>
#pragma clang diagnostic pop
#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace lp {

constexpr int kBadClasses = -8;  // GRX_LP_BAD_CLASSES

template <bool _USE_DOUBLE_BUFFER>
struct LpProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_src, d_dst, d_pw;  // the canonical pairs and their weights
        DeviceArray<int> d_nro, d_nci, d_ew;  // the neighbour CSR and the weight of every entry (NULL: 1 each)
        DeviceArray<int> d_labels, d_fresh, d_prev, d_chround, d_dirty, d_hubs;  // per vertex
        DeviceArray<int> d_list[2], d_start, d_community;
        DeviceArray<int> d_class, d_class_list;
        DeviceArray<unsigned long long> d_words;
    };

    SliceHolder<DataSlice> data_slices;
    long long pairs = 0;     // M
    int longest_row = 0;
    bool fresh = false;      // Reset has run and Enact has not
    bool enacted = false;    // the arrays hold a result
    double build_ms = 0;     // HIP-event time of the build of the pairs and the neighbour CSR
    long long communities = 0;  // of the last Enact
    // the classes (SetClasses): vertices [class_off[k], class_off[k + 1]) of d_class_list are class k
    int classes = 0;
    std::vector<int> class_off, class_longest;

    Ctx DeviceCtx(int strategy, int lane_max_row, int wave_max_row, int table_slots) const
    {
        const DataSlice *ds = data_slices[0];
        Ctx c;
        c.ro = ds->d_nro;
        c.ci = ds->d_nci;
        c.ew = ds->d_ew;
        c.labels = ds->d_labels;
        c.fresh = ds->d_fresh;
        c.prev = ds->d_prev;
        c.chround = ds->d_chround;
        c.dirty = ds->d_dirty;
        c.hubs = ds->d_hubs;
        c.words = ds->d_words;
        c.nodes = this->nodes;
        c.strategy = strategy;
        c.lane_max_row = lane_max_row;
        c.wave_max_row = wave_max_row;
        c.table_slots = table_slots;
        return c;
    }

    hipError_t ReadWord(int word, unsigned long long *out)
    {
        hipError_t retval = hipSuccess;
        hipStream_t stream = this->graph_slices[0]->stream;
        GR_CHECK(hipMemcpyAsync(out, data_slices[0]->d_words + word, sizeof(*out), hipMemcpyDeviceToHost, stream), "LpProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "LpProblem read-back sync failed");
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
        const bool weighted = gs->d_edge_values != nullptr;
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "LpProblem memset failed");

        // the CSR must be one: the build indexes with what it reads
        if ((retval = this->ValidateCsr())) return retval;

        long long M = 0;
        {  // (the build's scratch goes with this scope)
            graphio::BuildEvents ev;
            if ((retval = ev.Create(2))) return retval;
            if ((retval = ev.Record(0, stream))) return retval;
            graphio::PairGraph pg(n);
            if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
            if ((retval = pg.Pairs(stream))) return retval;
            if ((retval = pg.Rows(stream))) return retval;
            ds->d_src.Adopt(graphio::Take(pg.d_src));
            ds->d_dst.Adopt(graphio::Take(pg.d_dst));
            ds->d_nro.Adopt(graphio::Take(pg.d_ro));
            ds->d_nci.Adopt(graphio::Take(pg.d_ci));
            pairs = M = pg.pairs;
            if (M > 0) {
                // the weights as matching builds them: every input entry raises its pair's weight to its own
                const size_t ms = static_cast<size_t>(M);
                if ((retval = ds->d_pw.Alloc(ms))) return retval;
                hipLaunchKernelGGL(oprtr::FillKernel<int>, dim3(graphio::PairGrid(M)), dim3(256), 0, stream, ds->d_pw, M, weighted ? INT_MIN : 1);
                GR_CHECK(hipGetLastError(), "FillKernel launch failed");
                if (weighted) {
                    if ((retval = ds->d_ew.Alloc(2 * ms))) return retval;
                    hipLaunchKernelGGL(matching::PairWeightKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices,
                                       gs->d_edge_values, static_cast<int>(n), m, ds->d_nro, ds->d_nci, pg.d_eid, ds->d_pw);
                    GR_CHECK(hipGetLastError(), "PairWeightKernel launch failed");
                    hipLaunchKernelGGL(matching::EntryWeightKernel, dim3(graphio::PairGrid(2 * M)), dim3(256), 0, stream, pg.d_eid, ds->d_pw, 2 * M, ds->d_ew);
                    GR_CHECK(hipGetLastError(), "EntryWeightKernel launch failed");
                    hipLaunchKernelGGL(MinWeightKernel, dim3(graphio::PairGrid(M)), dim3(256), 0, stream, ds->d_pw, M, ds->d_words + W_FLAG);
                    GR_CHECK(hipGetLastError(), "MinWeightKernel launch failed");
                }
            }
            hipLaunchKernelGGL(LongestRowKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_nro, n, ds->d_words + W_HUBS);
            GR_CHECK(hipGetLastError(), "LongestRowKernel launch failed");
            if ((retval = ev.Record(1, stream))) return retval;
            GR_CHECK(hipStreamSynchronize(stream), "LpProblem build sync failed");
            if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        }
        unsigned long long flag = 0, longest = 0;
        if ((retval = ReadWord(W_HUBS, &longest))) return retval;  // (the word is the enactor's from the first Reset on)
        longest_row = static_cast<int>(longest);
        if ((retval = ReadWord(W_FLAG, &flag))) return retval;
        if (flag) return this->Malformed();  // a pair weight below 1

        DeviceArray<int> *vertex_arrays[] = {&ds->d_labels, &ds->d_fresh, &ds->d_prev, &ds->d_chround, &ds->d_dirty, &ds->d_hubs, &ds->d_list[0],
                                 &ds->d_list[1], &ds->d_start, &ds->d_community, &ds->d_class, &ds->d_class_list};
        for (DeviceArray<int> *a : vertex_arrays) if ((retval = a->Alloc(n1))) return retval;
        return retval;
    }

    // One Init per object (grx_lp_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, true))) return retval;
        data_slices.Make();
        return Build();
    }

    // (the CSR and the weights are borrowed and read by the build only)
    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_weights)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices, d_weights))) return retval;
        data_slices.Make();
        return Build();
    }

    // classes[v] in [0, count), count <= nodes (checked by the caller).  *improper: a pair has both ends in one class; then
    // nothing is installed, and what was installed before is gone too.
    hipError_t SetClasses(const int *h_classes, int count, bool *improper)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        *improper = false;
        classes = 0;
        GR_CHECK(hipMemcpyAsync(ds->d_class, h_classes, sizeof(int) * static_cast<size_t>(n), hipMemcpyHostToDevice, stream), "LpProblem upload failed");
        GR_CHECK(hipMemsetAsync(ds->d_words + W_FLAG, 0, sizeof(unsigned long long), stream), "LpProblem memset failed");
        if (pairs > 0) {
            hipLaunchKernelGGL(ClassCheckKernel, dim3(graphio::PairGrid(pairs)), dim3(256), 0, stream, ds->d_src, ds->d_dst, ds->d_class, pairs, ds->d_words + W_FLAG);
            GR_CHECK(hipGetLastError(), "ClassCheckKernel launch failed");
        }
        unsigned long long flag = 0;
        if ((retval = ReadWord(W_FLAG, &flag))) return retval;
        if (flag) {
            *improper = true;
            return retval;
        }
        // the lists: the keys (class, id) sorted; the offsets by bisection; the longest row of every class
        int class_bits = 1, col_bits = 1;
        while ((1ll << class_bits) < count) ++class_bits;
        while ((1ll << col_bits) < n) ++col_bits;
        graphio::DeviceKeySort sort;
        graphio::DeviceScratch<int> off, longest;
        GR_CHECK(sort.Reserve(n), "LpProblem sort scratch failed");
        if ((retval = off.Alloc(static_cast<size_t>(count) + 1))) return retval;
        if ((retval = longest.Alloc(static_cast<size_t>(count)))) return retval;
        GR_CHECK(hipMemsetAsync(longest.p, 0, sizeof(int) * static_cast<size_t>(count), stream), "LpProblem memset failed");
        hipLaunchKernelGGL(ClassKeysKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_class, ds->d_nro, n, col_bits, sort.Keys(), longest.p);
        GR_CHECK(hipGetLastError(), "ClassKeysKernel launch failed");
        unsigned long long *d_sorted = nullptr;
        GR_CHECK(sort.Sort(n, class_bits + col_bits, stream, &d_sorted), "LpProblem class sort failed");
        hipLaunchKernelGGL(ClassListKernel, dim3(graphio::PairGrid(n > count ? n : count + 1)), dim3(256), 0, stream, d_sorted, n, count, col_bits,
                           ds->d_class_list, off.p);
        GR_CHECK(hipGetLastError(), "ClassListKernel launch failed");
        class_off.assign(static_cast<size_t>(count) + 1, 0);
        class_longest.assign(static_cast<size_t>(count), 0);
        GR_CHECK(hipMemcpyAsync(class_off.data(), off.p, sizeof(int) * (static_cast<size_t>(count) + 1), hipMemcpyDeviceToHost, stream),
                 "LpProblem read-back failed");
        GR_CHECK(hipMemcpyAsync(class_longest.data(), longest.p, sizeof(int) * static_cast<size_t>(count), hipMemcpyDeviceToHost, stream),
                 "LpProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "LpProblem SetClasses sync failed");
        classes = count;
        return retval;
    }

    // h_start: the caller's labels, validated by the caller (NULL: L[v] = v); every vertex dirty and in list 0, the counters at 0
    hipError_t Reset(const int *h_start = nullptr)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        if (h_start)
            GR_CHECK(hipMemcpyAsync(ds->d_start, h_start, sizeof(int) * static_cast<size_t>(n), hipMemcpyHostToDevice, stream), "LpProblem upload failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "LpProblem memset failed");
        hipLaunchKernelGGL(ResetKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, DeviceCtx(LP_AUTO, kLaneMaxRow, kWaveMaxRow, kTableSlots),
                           h_start ? ds->d_start : nullptr, ds->d_list[0]);
        GR_CHECK(hipGetLastError(), "ResetKernel launch failed");
        GR_CHECK(hipStreamSynchronize(stream), "LpProblem Reset sync failed");  // (h_start is the caller's again)
        fresh = true;
        enacted = false;
        communities = 0;
        return retval;
    }

    // community[] from the labels of the finished Enact; the count lands in W_COMMUNITIES (the enactor's last read-back brings it)
    hipError_t Finish()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        const long long tiles = (n + graphio::kScanTile - 1) / graphio::kScanTile;
        graphio::DeviceScratch<unsigned> used;
        graphio::DeviceScratch<unsigned long long> sums;
        graphio::DeviceScratch<int> rank;
        if ((retval = used.Alloc(static_cast<size_t>(n)))) return retval;
        if ((retval = rank.Alloc(static_cast<size_t>(n)))) return retval;
        if ((retval = sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(n))))) return retval;
        GR_CHECK(hipMemsetAsync(used.p, 0, sizeof(unsigned) * static_cast<size_t>(n), stream), "LpProblem memset failed");
        hipLaunchKernelGGL(UsedKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_labels, n, used.p);
        GR_CHECK(hipGetLastError(), "UsedKernel launch failed");
        GR_CHECK(graphio::DeviceExclusiveScan<int>(used.p, rank.p, n, sums.p, stream), "LpProblem rank scan failed");
        hipLaunchKernelGGL(CommunityKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_labels, rank.p, n, ds->d_community);
        GR_CHECK(hipGetLastError(), "CommunityKernel launch failed");
        GR_CHECK(hipMemcpyAsync(ds->d_words + W_COMMUNITIES, sums.p + tiles, sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream),
                 "LpProblem copy failed");
        GR_CHECK(hipStreamSynchronize(stream), "LpProblem Finish sync failed");  // (the scratch goes with this scope)
        return retval;
    }

    // every pointer may be NULL
    hipError_t Extract(int *h_labels, int *h_community)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t n = static_cast<size_t>(this->nodes);
        if ((retval = this->Read(h_labels, ds->d_labels.p, n))) return retval;
        return this->Read(h_community, ds->d_community.p, n);
    }

    // int64 per community: size, internal weight, volume; *total = W.  Every pointer may be NULL.
    hipError_t Summary(long long *h_size, long long *h_internal, long long *h_volume, long long *total)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        const size_t k = static_cast<size_t>(communities);
        graphio::DeviceScratch<unsigned long long> sums;  // size, internal, volume, W
        if ((retval = sums.Alloc(3 * k + 1))) return retval;
        GR_CHECK(hipMemsetAsync(sums.p, 0, sizeof(unsigned long long) * (3 * k + 1), stream), "LpProblem memset failed");
        hipLaunchKernelGGL(SizeVolumeKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_community, ds->d_nro, ds->d_ew, n, sums.p, sums.p + 2 * k);
        GR_CHECK(hipGetLastError(), "SizeVolumeKernel launch failed");
        if (pairs > 0) {
            hipLaunchKernelGGL(InternalKernel, dim3(graphio::PairGrid(pairs)), dim3(256), 0, stream, ds->d_src, ds->d_dst, ds->d_pw, ds->d_community, pairs,
                               sums.p + k, sums.p + 3 * k);
            GR_CHECK(hipGetLastError(), "InternalKernel launch failed");
        }
        const unsigned long long *d = sums.p;
        if ((retval = this->Read(reinterpret_cast<unsigned long long *>(h_size), d, k))) return retval;
        if ((retval = this->Read(reinterpret_cast<unsigned long long *>(h_internal), d + k, k))) return retval;
        if ((retval = this->Read(reinterpret_cast<unsigned long long *>(h_volume), d + 2 * k, k))) return retval;
        if ((retval = this->Read(reinterpret_cast<unsigned long long *>(total), d + 3 * k, 1))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "LpProblem Summary sync failed");
        return retval;
    }
};

}  // namespace lp
}  // namespace app
}  // namespace gunrock
