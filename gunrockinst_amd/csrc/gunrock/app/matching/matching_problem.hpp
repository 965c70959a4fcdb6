// app/matching/matching_problem.hpp -- device data for the heavy-edge matching and its contraction into the coarse graph.
//
// The reference snapshot has no matching; the shape is this tree's Problem (compare app/maxflow/maxflow_problem.hpp).  The input CSR
// is read as BCC and truss read it: the simple undirected graph G, with int weights in edge_values (NULL: 1 each).  Init validates
// it and builds, with graphio::PairGraph (graphio/pair_graph.hpp), the M canonical pairs src[e] < dst[e] in
// (src, dst) order and the neighbour CSR with the pair id on every entry; a pair's weight is the largest of its input entries.
// Contract builds the coarse graph of the last Enact on the device and keeps it until the next Reset.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/matching/matching_functor.hpp>
#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace matching {

struct Summary {
    long long pairs = 0, matched = 0, weight = 0, unmatched = 0, unmatched_with_neighbours = 0;
};

constexpr int kOverflow = -5;  // GRX_MATCHING_OVERFLOW

template <bool _USE_DOUBLE_BUFFER>
struct MatchingProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_src, d_dst, d_pw;  // the canonical pairs and their weights
        DeviceArray<int> d_nro, d_nci, d_neid, d_ew;  // the neighbour CSR; the pair and the weight of every entry
        DeviceArray<int> d_mate, d_tgt, d_pp, d_cur, d_list[2];  // per vertex
        DeviceArray<unsigned char> d_in;  // per pair
        DeviceArray<unsigned> d_words;
        DeviceArray<unsigned long long> d_counters;
        DeviceArray<Active> d_active;
        // the coarse graph of the last Contract
        DeviceArray<int> d_map, d_vweight, d_cro, d_cci, d_cw;
    };

    SliceHolder<DataSlice> data_slices;
    long long pairs = 0;     // M
    long long with_neighbours = 0;  // vertices of degree > 0 (the first live list of the last Reset)
    unsigned seed = 0;
    bool weighted = false;
    bool fresh = false;      // Reset has run and Enact has not
    bool enacted = false;    // the arrays hold a result
    double build_ms = 0;     // HIP-event time of the build of the pairs and the neighbour CSR
    Summary summary;         // of the last Enact
    long long coarse_nodes = -1, coarse_entries = 0;  // of the last Contract (-1: none)

    Ctx DeviceCtx(int wave_min_row) const
    {
        const DataSlice *ds = data_slices[0];
        Ctx c;
        c.ro = ds->d_nro;
        c.ci = ds->d_nci;
        c.eid = ds->d_neid;
        c.ew = ds->d_ew;
        c.pw = ds->d_pw;
        c.mate = ds->d_mate;
        c.tgt = ds->d_tgt;
        c.pp = ds->d_pp;
        c.cur = ds->d_cur;
        c.in_matching = ds->d_in;
        c.words = ds->d_words;
        c.counters = ds->d_counters;
        c.nodes = this->nodes;
        c.seed_mul = seed * 0x9E3779B9u;
        c.wave_min_row = wave_min_row;
        return c;
    }

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        weighted = gs->d_edge_values != nullptr;
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        if ((retval = ds->d_counters.Alloc(C_COUNT))) return retval;
        if ((retval = ds->d_active.Alloc(1))) return retval;

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
            pairs = M = pg.pairs;
            if (M > 0) {
                // the weights: every input entry finds its pair by bisecting the sorted row (the key sort carries no payload) and
                // raises the pair's weight to its own, as max-flow's build adds its capacities up
                const size_t ms = static_cast<size_t>(M);
                if ((retval = ds->d_pw.Alloc(ms))) return retval;
                hipLaunchKernelGGL(oprtr::FillKernel<int>, dim3(graphio::PairGrid(M)), dim3(256), 0, stream, ds->d_pw, M, weighted ? INT_MIN : 1);
                GR_CHECK(hipGetLastError(), "FillKernel launch failed");
                if (weighted) {
                    if ((retval = ds->d_ew.Alloc(2 * ms))) return retval;
                    hipLaunchKernelGGL(PairWeightKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices,
                                       gs->d_edge_values, static_cast<int>(n), m, ds->d_nro, ds->d_nci, ds->d_neid, ds->d_pw);
                    GR_CHECK(hipGetLastError(), "PairWeightKernel launch failed");
                    hipLaunchKernelGGL(EntryWeightKernel, dim3(graphio::PairGrid(2 * M)), dim3(256), 0, stream, ds->d_neid, ds->d_pw, 2 * M, ds->d_ew);
                    GR_CHECK(hipGetLastError(), "EntryWeightKernel launch failed");
                }
            }
            if ((retval = ev.Record(1, stream))) return retval;
            GR_CHECK(hipStreamSynchronize(stream), "MatchingProblem build sync failed");
            if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        }

        const size_t m1 = static_cast<size_t>(M > 0 ? M : 1);
        DeviceArray<int> *vertex_arrays[] = {&ds->d_mate, &ds->d_tgt, &ds->d_pp, &ds->d_cur, &ds->d_list[0], &ds->d_list[1]};
        for (DeviceArray<int> *a : vertex_arrays) if ((retval = a->Alloc(n1))) return retval;
        if ((retval = ds->d_in.Alloc(m1))) return retval;
        return retval;
    }

    // One Init per object (grx_matching_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, unsigned new_seed, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        seed = new_seed;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, true))) return retval;
        data_slices.Make();
        return Build();
    }

    // (the CSR and the weights are borrowed and read by the build only)
    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_weights, unsigned new_seed)
    {
        hipError_t retval = hipSuccess;
        seed = new_seed;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices, d_weights))) return retval;
        data_slices.Make();
        return Build();
    }

    // nobody matched, every pointer and cursor at its start, the vertices with a neighbour in list 0; the coarse graph goes
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned) * W_COUNT, stream), "MatchingProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_counters, 0, sizeof(unsigned long long) * C_COUNT, stream), "MatchingProblem memset failed");
        if (pairs) GR_CHECK(hipMemsetAsync(ds->d_in, 0, static_cast<size_t>(pairs), stream), "MatchingProblem memset failed");
        hipLaunchKernelGGL(SeedKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, DeviceCtx(kWaveMinRow), ds->d_list[0]);
        GR_CHECK(hipGetLastError(), "SeedKernel launch failed");
        unsigned first = 0;
        GR_CHECK(hipMemcpyAsync(&first, ds->d_words + W_NEXT, sizeof(first), hipMemcpyDeviceToHost, stream), "MatchingProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "MatchingProblem Reset sync failed");
        with_neighbours = first;
        fresh = true;
        enacted = false;
        summary = Summary();
        DropCoarse();
        return retval;
    }

    // every pointer may be NULL
    hipError_t Pairs(int *h_src, int *h_dst, int *h_weight)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t M = static_cast<size_t>(pairs);
        if ((retval = this->Read(h_src, ds->d_src.p, M))) return retval;
        if ((retval = this->Read(h_dst, ds->d_dst.p, M))) return retval;
        return this->Read(h_weight, ds->d_pw.p, M);
    }

    hipError_t Extract(unsigned char *h_in, int *h_mate, int *h_medge)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t n = static_cast<size_t>(this->nodes), M = static_cast<size_t>(pairs);
        if ((retval = this->Read(h_in, ds->d_in.p, M))) return retval;
        if ((retval = this->Read(h_mate, ds->d_mate.p, n))) return retval;
        return this->Read(h_medge, ds->d_pp.p, n);
    }

    void DropCoarse()
    {
        DataSlice *ds = data_slices[0];
        for (DeviceArray<int> *a : {&ds->d_map, &ds->d_vweight, &ds->d_cro, &ds->d_cci, &ds->d_cw}) a->Free();
        coarse_nodes = -1;
        coarse_entries = 0;
    }

    // The coarse graph of the matching, kept until the next Reset.  d_vertex_weights is on the device (NULL: 1 each).  *overflow is
    // set when a sum left int32: then nothing is kept.
    hipError_t Contract(const int *d_vertex_weights, bool *overflow)
    {
        *overflow = false;
        DropCoarse();
        const hipError_t retval = BuildCoarse(d_vertex_weights, overflow);
        if (retval || *overflow) DropCoarse();
        return retval;
    }

    // map[] from a flag and a scan over the representatives, the coarse pairs and their mirrored CSR by graphio::PairGraph from the
    // fine pairs' images, their weights by bisection and a 64-bit atomic add
    hipError_t BuildCoarse(const int *d_vertex_weights, bool *overflow)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const long long n = this->nodes, M = pairs;
        const long long scan_tiles_n = (n + graphio::kScanTile - 1) / graphio::kScanTile;
        graphio::DeviceScratch<unsigned> rep;
        graphio::DeviceScratch<unsigned long long> sums, w64;
        graphio::DeviceScratch<int> rank;
        if ((retval = rep.Alloc(static_cast<size_t>(n)))) return retval;
        if ((retval = sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(n))))) return retval;
        if ((retval = rank.Alloc(static_cast<size_t>(n)))) return retval;
        if ((retval = ds->d_map.Alloc(static_cast<size_t>(n)))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_words + W_FLAG, 0, sizeof(unsigned), stream), "MatchingProblem memset failed");

        // the representatives and their ranks (the total is behind the scan's tile offsets)
        hipLaunchKernelGGL(RepFlagKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_mate, n, rep.p);
        GR_CHECK(hipGetLastError(), "RepFlagKernel launch failed");
        GR_CHECK(graphio::DeviceExclusiveScan<int>(rep.p, rank.p, n, sums.p, stream), "MatchingProblem rank scan failed");
        unsigned long long total = 0;
        GR_CHECK(hipMemcpyAsync(&total, sums.p + scan_tiles_n, sizeof(total), hipMemcpyDeviceToHost, stream), "MatchingProblem read total failed");
        GR_CHECK(hipStreamSynchronize(stream), "MatchingProblem Contract sync failed");
        const long long nc = static_cast<long long>(total);
        if ((retval = ds->d_vweight.Alloc(static_cast<size_t>(nc)))) return retval;
        hipLaunchKernelGGL(MapKernel, dim3(graphio::PairGrid(n)), dim3(256), 0, stream, ds->d_mate, rank.p, d_vertex_weights, n, ds->d_map, ds->d_vweight,
                           ds->d_words + W_FLAG);
        GR_CHECK(hipGetLastError(), "MapKernel launch failed");

        // the coarse pairs: the fine pairs' images as keys, then the build's steps on them
        graphio::PairGraph pg(nc);
        if (M > 0) {
            if ((retval = pg.Reserve(M))) return retval;
            hipLaunchKernelGGL(CoarseKeysKernel, dim3(graphio::PairGrid(M)), dim3(256), 0, stream, ds->d_src, ds->d_dst, ds->d_map, M, pg.col_bits, pg.sentinel,
                               pg.sort.Keys());
            GR_CHECK(hipGetLastError(), "CoarseKeysKernel launch failed");
            if ((retval = pg.SortKeys(stream))) return retval;
            if ((retval = pg.Pairs(stream))) return retval;
        }
        const long long Mc = pg.pairs;
        if (Mc > 0) {
            if ((retval = w64.Alloc(static_cast<size_t>(Mc)))) return retval;
            GR_CHECK(hipMemsetAsync(w64.p, 0, sizeof(unsigned long long) * static_cast<size_t>(Mc), stream), "MatchingProblem memset failed");
            hipLaunchKernelGGL(CoarseWeightKernel, dim3(graphio::PairGrid(M)), dim3(256), 0, stream, ds->d_src, ds->d_dst, ds->d_pw, ds->d_map, M, pg.col_bits,
                               pg.sentinel, pg.d_ckeys, Mc, w64.p);
            GR_CHECK(hipGetLastError(), "CoarseWeightKernel launch failed");
        }
        if ((retval = pg.Rows(stream))) return retval;
        ds->d_cro.Adopt(graphio::Take(pg.d_ro));
        ds->d_cci.Adopt(graphio::Take(pg.d_ci));
        if (Mc > 0) {
            if ((retval = ds->d_cw.Alloc(2 * static_cast<size_t>(Mc)))) return retval;
            hipLaunchKernelGGL(CoarseEntriesKernel, dim3(graphio::PairGrid(2 * Mc)), dim3(256), 0, stream, pg.d_eid, w64.p, 2 * Mc, ds->d_cw, ds->d_words + W_FLAG);
            GR_CHECK(hipGetLastError(), "CoarseEntriesKernel launch failed");
        }
        unsigned flag = 0;
        GR_CHECK(hipMemcpyAsync(&flag, ds->d_words + W_FLAG, sizeof(flag), hipMemcpyDeviceToHost, stream), "MatchingProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "MatchingProblem Contract sync failed");
        *overflow = flag != 0;
        coarse_nodes = nc;
        coarse_entries = 2 * Mc;
        return retval;
    }

    // every pointer may be NULL
    hipError_t CoarseExtract(int *h_map, int *h_ro, int *h_ci, int *h_w, int *h_vweight)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t nc = static_cast<size_t>(coarse_nodes), entries = static_cast<size_t>(coarse_entries);
        if ((retval = this->Read(h_map, ds->d_map.p, static_cast<size_t>(this->nodes)))) return retval;
        if ((retval = this->Read(h_ro, ds->d_cro.p, nc + 1))) return retval;
        if ((retval = this->Read(h_ci, ds->d_cci.p, entries))) return retval;
        if ((retval = this->Read(h_w, ds->d_cw.p, entries))) return retval;
        return this->Read(h_vweight, ds->d_vweight.p, nc);
    }
};

}  // namespace matching
}  // namespace app
}  // namespace gunrock
