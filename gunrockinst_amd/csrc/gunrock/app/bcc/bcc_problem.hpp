// app/bcc/bcc_problem.hpp -- device data for the biconnected components, articulation points, bridges and 2-edge-connected
// components.
//
// The reference snapshot has no app/bcc; the shape is this tree's Problem (compare app/truss/truss_problem.hpp).  The input CSR is
// read as MIS, TC, k-core and truss read it: the simple undirected graph G.  Init validates it and builds, with graphio::PairGraph
// (graphio/pair_graph.hpp), the M canonical edges src[e] < dst[e] in (src, dst) order and the neighbour CSR with
// the edge id on every entry.  The per-vertex and per-edge arrays are bcc_functor.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/bcc/bcc_functor.hpp>
#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace bcc {

struct Summary {
    long long blocks = 0, bridges = 0, articulation_points = 0, largest_block = 0, tecc_components = 0, largest_tecc = 0;
    int largest_block_id = -1, largest_tecc_root = -1;
};

template <bool _USE_DOUBLE_BUFFER>
struct BccProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_src, d_dst;  // the canonical edges
        DeviceArray<int> d_nro, d_nci, d_neid;  // the neighbour CSR, rows ascending, and the edge of every entry
        // per vertex
        DeviceArray<int> d_comp, d_parent, d_level, d_pedge, d_size, d_pre, d_low, d_high, d_queue, d_uf, d_set, d_first, d_tecc, d_tsize, d_min_of, d_cnt_of;
        DeviceArray<int> d_bounds;  // nodes + 2
        DeviceArray<unsigned> d_ents;  // nodes + 2
        // per edge
        DeviceArray<int> d_bcc, d_bsize;
        DeviceArray<unsigned char> d_bridge, d_art;
        DeviceArray<int> d_cut_vertex, d_cut_block;  // the block-cut tree of the last Enact, built at the first request
        DeviceArray<unsigned> d_words;
        DeviceArray<unsigned long long> d_counters;  // [0] row entries walked, [1] articulation points, [2..4] and [5..7] SummaryKernel's
        DeviceArray<unsigned long long> d_clock;  // PHASE_COUNT + 1 stamps
        DeviceArray<Front> d_front;
    };

    SliceHolder<DataSlice> data_slices;
    long long simple_edges = 0;  // M
    bool fresh = false;          // Reset has run and Enact has not
    bool enacted = false;        // the arrays hold a result
    double build_ms = 0;         // HIP-event time of the build of the edges and the neighbour CSR
    Summary summary;             // of the last Enact
    long long cut_pairs = -1;    // the pairs in d_cut_vertex / d_cut_block (-1: not built)

    Ctx DeviceCtx(int wave_min_row) const
    {
        const DataSlice *ds = data_slices[0];
        Ctx c;
        c.ro = ds->d_nro;
        c.ci = ds->d_nci;
        c.eid = ds->d_neid;
        c.parent = ds->d_parent;
        c.level = ds->d_level;
        c.pedge = ds->d_pedge;
        c.size = ds->d_size;
        c.pre = ds->d_pre;
        c.low = ds->d_low;
        c.high = ds->d_high;
        c.queue = ds->d_queue;
        c.bounds = ds->d_bounds;
        c.ents = ds->d_ents;
        c.words = ds->d_words;
        c.reads = ds->d_counters;
        c.nodes = this->nodes;
        c.wave_min_row = wave_min_row;
        return c;
    }

    Tree DeviceTree() const
    {
        const DataSlice *ds = data_slices[0];
        return Tree{ds->d_parent, ds->d_pedge, ds->d_size, ds->d_pre, ds->d_low, ds->d_high};
    }

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        if ((retval = ds->d_counters.Alloc(8))) return retval;
        if ((retval = ds->d_clock.Alloc(PHASE_COUNT + 1))) return retval;
        if ((retval = ds->d_front.Alloc(1))) return retval;

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
            ds->d_neid.Adopt(graphio::Take(pg.d_eid));
            simple_edges = M = pg.pairs;
            if ((retval = ev.Record(1, stream))) return retval;
            GR_CHECK(hipStreamSynchronize(stream), "BccProblem build sync failed");
            if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        }

        const size_t m1 = static_cast<size_t>(M > 0 ? M : 1);
        DeviceArray<int> *vertex_arrays[] = {&ds->d_comp, &ds->d_parent, &ds->d_level, &ds->d_pedge, &ds->d_size, &ds->d_pre, &ds->d_low, &ds->d_high, &ds->d_queue,
                                 &ds->d_uf, &ds->d_set, &ds->d_first, &ds->d_tecc, &ds->d_tsize, &ds->d_min_of, &ds->d_cnt_of};
        for (DeviceArray<int> *a : vertex_arrays) if ((retval = a->Alloc(n1))) return retval;
        if ((retval = ds->d_bounds.Alloc(n1 + 2))) return retval;
        if ((retval = ds->d_ents.Alloc(n1 + 2))) return retval;
        if ((retval = ds->d_bcc.Alloc(m1))) return retval;
        if ((retval = ds->d_bsize.Alloc(m1))) return retval;
        if ((retval = ds->d_bridge.Alloc(m1))) return retval;
        if ((retval = ds->d_art.Alloc(n1))) return retval;
        return retval;
    }

    // One Init per object (grx_bcc_init refuses a second one)
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

    // the words, the counters, the two masks and the level table at 0 (everything else is written before it is read)
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t n = static_cast<size_t>(this->nodes), M = static_cast<size_t>(simple_edges);
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * W_COUNT, stream), "BccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(unsigned long long) * 8, stream), "BccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_clock, 0, sizeof(unsigned long long) * (PHASE_COUNT + 1), stream), "BccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_bounds, 0, sizeof(int) * (n + 2), stream), "BccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_ents, 0, sizeof(unsigned) * (n + 2), stream), "BccProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_art, 0, n, stream), "BccProblem memset failed");
        if (M) GR_CHECK(hipMemsetAsync(ds->d_bridge, 0, M, stream), "BccProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "BccProblem Reset sync failed");
        fresh = true;
        enacted = false;
        summary = Summary();
        DropBlockCut();
        return retval;
    }

    hipError_t Edges(int *h_src, int *h_dst)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t M = static_cast<size_t>(simple_edges);
        if ((retval = this->Read(h_src, ds->d_src.p, M))) return retval;
        return this->Read(h_dst, ds->d_dst.p, M);
    }

    // every pointer may be NULL
    hipError_t Extract(int *h_bcc, unsigned char *h_bridge, unsigned char *h_art, int *h_tecc, int *h_block_size)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t n = static_cast<size_t>(this->nodes), M = static_cast<size_t>(simple_edges);
        if ((retval = this->Read(h_bcc, ds->d_bcc.p, M))) return retval;
        if ((retval = this->Read(h_bridge, ds->d_bridge.p, M))) return retval;
        if ((retval = this->Read(h_art, ds->d_art.p, n))) return retval;
        if ((retval = this->Read(h_tecc, ds->d_tecc.p, n))) return retval;
        return this->Read(h_block_size, ds->d_bsize.p, M);
    }

    void DropBlockCut()
    {
        DataSlice *ds = data_slices[0];
        ds->d_cut_vertex.Free();
        ds->d_cut_block.Free();
        cut_pairs = -1;
    }

    // the distinct pairs (v, block) over the articulation points v and the blocks at them, sorted by (v, block), into d_cut_vertex /
    // d_cut_block (SccProblem::Condensation's sequence).  Kept until the next Reset: asking for the count and then for the pairs sorts
    // the 2M keys once.
    hipError_t BuildBlockCut()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes, keys = 2 * simple_edges;
        if (keys == 0 || summary.articulation_points == 0) {
            cut_pairs = 0;
            return retval;
        }
        int col_bits = 1, edge_bits = 1;
        while ((1ll << col_bits) < n + 1) ++col_bits;  // (+ 1: the sentinel's vertex part is no vertex)
        while ((1ll << edge_bits) < simple_edges) ++edge_bits;
        const int key_bits = col_bits + edge_bits;  // <= 63
        const unsigned long long sentinel = (1ull << key_bits) - 1ull;
        graphio::DeviceKeySort sort;
        graphio::DeviceScratch<unsigned> d_keep;
        graphio::DeviceScratch<unsigned long long> d_pos, d_sums;
        auto run = [&]() -> hipError_t {
            hipError_t retval = hipSuccess;
            GR_CHECK(sort.Reserve(keys), "BccProblem sort scratch failed");
            if ((retval = d_keep.Alloc(static_cast<size_t>(keys)))) return retval;
            if ((retval = d_pos.Alloc(static_cast<size_t>(keys)))) return retval;
            if ((retval = d_sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(keys))))) return retval;
            hipLaunchKernelGGL(BlockCutKeysKernel, dim3(graphio::PairGrid(simple_edges)), dim3(256), 0, stream, ds->d_src, ds->d_dst, ds->d_bcc, ds->d_art, simple_edges,
                               edge_bits, sentinel, sort.Keys());
            GR_CHECK(hipGetLastError(), "BlockCutKeysKernel launch failed");
            unsigned long long *d_sorted = nullptr;
            GR_CHECK(sort.Sort(keys, key_bits, stream, &d_sorted), "BccProblem key sort failed");
            hipLaunchKernelGGL(graphio::FlagKernel, dim3(graphio::PairGrid(keys)), dim3(256), 0, stream, d_sorted, keys, sentinel, d_keep);
            GR_CHECK(hipGetLastError(), "FlagKernel launch failed");
            GR_CHECK(graphio::DeviceExclusiveScan<unsigned long long>(d_keep.p, d_pos.p, keys, d_sums.p, stream), "BccProblem flag scan failed");
            const long long scan_tiles = (keys + graphio::kScanTile - 1) / graphio::kScanTile;  // (the total is behind the tile offsets)
            unsigned long long total = 0;
            GR_CHECK(hipMemcpyAsync(&total, d_sums + scan_tiles, sizeof(total), hipMemcpyDeviceToHost, stream), "BccProblem read total failed");
            GR_CHECK(hipStreamSynchronize(stream), "BccProblem BlockCut sync failed");
            const long long pairs = static_cast<long long>(total);
            if (pairs > 0) {
                if ((retval = ds->d_cut_vertex.Alloc(static_cast<size_t>(pairs)))) return retval;
                if ((retval = ds->d_cut_block.Alloc(static_cast<size_t>(pairs)))) return retval;
                hipLaunchKernelGGL(scc::CondensationEmitKernel, dim3(graphio::PairGrid(keys)), dim3(256), 0, stream, d_sorted, d_keep, d_pos, keys, edge_bits, pairs,
                                   ds->d_cut_vertex, ds->d_cut_block);
                GR_CHECK(hipGetLastError(), "CondensationEmitKernel launch failed");
                GR_CHECK(hipStreamSynchronize(stream), "BccProblem BlockCut sync failed");
            }
            cut_pairs = pairs;
            return retval;
        };
        retval = run();
        if (retval) DropBlockCut();
        return retval;
    }

    // the first max_edges pairs go to h_vertex / h_block, *count is how many there are
    hipError_t BlockCut(long long max_edges, int *h_vertex, int *h_block, long long *count)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        *count = 0;
        if (cut_pairs < 0 && (retval = BuildBlockCut())) return retval;
        *count = cut_pairs;
        const long long take = cut_pairs < max_edges ? cut_pairs : max_edges;
        if (take < 1 || !h_vertex || !h_block) return retval;
        if ((retval = this->Read(h_vertex, ds->d_cut_vertex.p, static_cast<size_t>(take)))) return retval;
        return this->Read(h_block, ds->d_cut_block.p, static_cast<size_t>(take));
    }
};

}  // namespace bcc
}  // namespace app
}  // namespace gunrock
