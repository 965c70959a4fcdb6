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
        int *d_src = nullptr, *d_dst = nullptr, *d_pw = nullptr;                     // the canonical pairs and their weights
        int *d_nro = nullptr, *d_nci = nullptr, *d_neid = nullptr, *d_ew = nullptr;  // the neighbour CSR; the pair and the weight of every entry
        int *d_mate = nullptr, *d_tgt = nullptr, *d_pp = nullptr, *d_cur = nullptr, *d_list[2] = {nullptr, nullptr};  // per vertex
        unsigned char *d_in = nullptr;                                               // per pair
        unsigned *d_words = nullptr;
        unsigned long long *d_counters = nullptr;
        Active *d_active = nullptr;
        // the coarse graph of the last Contract
        int *d_map = nullptr, *d_vweight = nullptr, *d_cro = nullptr, *d_cci = nullptr, *d_cw = nullptr;
    };

    DataSlice **data_slices = nullptr;
    int malformed = 0;
    long long pairs = 0;     // M
    long long with_neighbours = 0;  // vertices of degree > 0 (the first live list of the last Reset)
    unsigned seed = 0;
    bool weighted = false;
    bool fresh = false;      // Reset has run and Enact has not
    bool enacted = false;    // the arrays hold a result
    double build_ms = 0;     // HIP-event time of the build of the pairs and the neighbour CSR
    Summary summary;         // of the last Enact
    long long coarse_nodes = -1, coarse_entries = 0;  // of the last Contract (-1: none)

    ~MatchingProblem() override
    {
        if (data_slices) {
            DataSlice *ds = data_slices[0];
            if (ds) {
                DropCoarse();
                void *bufs[] = {ds->d_src, ds->d_dst, ds->d_pw, ds->d_nro, ds->d_nci, ds->d_neid, ds->d_ew, ds->d_mate, ds->d_tgt, ds->d_pp, ds->d_cur,
                                ds->d_list[0], ds->d_list[1], ds->d_in, ds->d_words, ds->d_counters, ds->d_active};
                for (void *b : bufs)
                    if (b) util::GRError(hipFree(b), "MatchingProblem hipFree failed", __FILE__, __LINE__);
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
        GR_CHECK(hipMalloc(&ds->d_words, sizeof(unsigned) * W_COUNT), "MatchingProblem hipMalloc failed");
        GR_CHECK(hipMalloc(&ds->d_counters, sizeof(unsigned long long) * C_COUNT), "MatchingProblem hipMalloc failed");
        GR_CHECK(hipMalloc(&ds->d_active, sizeof(Active)), "MatchingProblem hipMalloc failed");

        // the CSR must be one: the build indexes with what it reads
        bool bad = false;
        if ((retval = graphio::DeviceValidateCsr(gs->d_row_offsets, gs->d_column_indices, n, m, reinterpret_cast<int *>(ds->d_words), stream, &bad)))
            return retval;
        if (bad) {
            malformed = 1;
            return hipErrorInvalidValue;
        }

        long long M = 0;
        {  // (the build's scratch goes with this scope)
            graphio::BuildEvents ev;
            if ((retval = ev.Create(2))) return retval;
            if ((retval = ev.Record(0, stream))) return retval;
            graphio::PairGraph pg(n);
            if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
            if ((retval = pg.Pairs(stream))) return retval;
            if ((retval = pg.Rows(stream))) return retval;
            ds->d_src = graphio::Take(pg.d_src);
            ds->d_dst = graphio::Take(pg.d_dst);
            ds->d_nro = graphio::Take(pg.d_ro);
            ds->d_nci = graphio::Take(pg.d_ci);
            ds->d_neid = graphio::Take(pg.d_eid);
            pairs = M = pg.pairs;
            if (M > 0) {
                // the weights: every input entry finds its pair by bisecting the sorted row (the key sort carries no payload) and
                // raises the pair's weight to its own, as max-flow's build adds its capacities up
                const size_t ms = static_cast<size_t>(M);
                GR_CHECK(hipMalloc(&ds->d_pw, sizeof(int) * ms), "MatchingProblem hipMalloc d_pw failed");
                hipLaunchKernelGGL(oprtr::FillKernel<int>, dim3(Grid(M)), dim3(256), 0, stream, ds->d_pw, M, weighted ? INT_MIN : 1);
                GR_CHECK(hipGetLastError(), "FillKernel launch failed");
                if (weighted) {
                    GR_CHECK(hipMalloc(&ds->d_ew, sizeof(int) * 2 * ms), "MatchingProblem hipMalloc d_ew failed");
                    hipLaunchKernelGGL(PairWeightKernel, dim3(Grid(m)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices,
                                       gs->d_edge_values, static_cast<int>(n), m, ds->d_nro, ds->d_nci, ds->d_neid, ds->d_pw);
                    GR_CHECK(hipGetLastError(), "PairWeightKernel launch failed");
                    hipLaunchKernelGGL(EntryWeightKernel, dim3(Grid(2 * M)), dim3(256), 0, stream, ds->d_neid, ds->d_pw, 2 * M, ds->d_ew);
                    GR_CHECK(hipGetLastError(), "EntryWeightKernel launch failed");
                }
            }
            if ((retval = ev.Record(1, stream))) return retval;
            GR_CHECK(hipStreamSynchronize(stream), "MatchingProblem build sync failed");
            if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        }

        const size_t m1 = static_cast<size_t>(M > 0 ? M : 1);
        int **vertex_arrays[] = {&ds->d_mate, &ds->d_tgt, &ds->d_pp, &ds->d_cur, &ds->d_list[0], &ds->d_list[1]};
        for (int **a : vertex_arrays) GR_CHECK(hipMalloc(a, sizeof(int) * n1), "MatchingProblem hipMalloc failed");
        GR_CHECK(hipMalloc(&ds->d_in, m1), "MatchingProblem hipMalloc failed");
        return retval;
    }

    // One Init per object (grx_matching_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, unsigned new_seed, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        seed = new_seed;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, true))) return retval;
        data_slices = new DataSlice *[1];
        data_slices[0] = new DataSlice();
        return Build();
    }

    // (the CSR and the weights are borrowed and read by the build only)
    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_weights, unsigned new_seed)
    {
        hipError_t retval = hipSuccess;
        seed = new_seed;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices, d_weights))) return retval;
        data_slices = new DataSlice *[1];
        data_slices[0] = new DataSlice();
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
        hipLaunchKernelGGL(SeedKernel, dim3(Grid(n)), dim3(256), 0, stream, DeviceCtx(kWaveMinRow), ds->d_list[0]);
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

    template <typename T>
    hipError_t Read(T *h_out, const T *d_in, size_t count)
    {
        hipError_t retval = hipSuccess;
        hipStream_t stream = this->graph_slices[0]->stream;
        if (h_out && count) {
            GR_CHECK(hipMemcpyAsync(h_out, d_in, sizeof(T) * count, hipMemcpyDeviceToHost, stream), "MatchingProblem read failed");
            GR_CHECK(hipStreamSynchronize(stream), "MatchingProblem read sync failed");
        }
        return retval;
    }

    // every pointer may be NULL
    hipError_t Pairs(int *h_src, int *h_dst, int *h_weight)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t M = static_cast<size_t>(pairs);
        if ((retval = Read(h_src, ds->d_src, M))) return retval;
        if ((retval = Read(h_dst, ds->d_dst, M))) return retval;
        return Read(h_weight, ds->d_pw, M);
    }

    hipError_t Extract(unsigned char *h_in, int *h_mate, int *h_medge)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t n = static_cast<size_t>(this->nodes), M = static_cast<size_t>(pairs);
        if ((retval = Read(h_in, ds->d_in, M))) return retval;
        if ((retval = Read(h_mate, ds->d_mate, n))) return retval;
        return Read(h_medge, ds->d_pp, n);
    }

    void DropCoarse()
    {
        DataSlice *ds = data_slices[0];
        int **bufs[] = {&ds->d_map, &ds->d_vweight, &ds->d_cro, &ds->d_cci, &ds->d_cw};
        for (int **b : bufs) {
            if (*b) util::GRError(hipFree(*b), "MatchingProblem hipFree failed", __FILE__, __LINE__);
            *b = nullptr;
        }
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
        GR_CHECK(hipMalloc(&ds->d_map, sizeof(int) * static_cast<size_t>(n)), "MatchingProblem hipMalloc failed");
        GR_CHECK(hipMemsetAsync(ds->d_words + W_FLAG, 0, sizeof(unsigned), stream), "MatchingProblem memset failed");

        // the representatives and their ranks (the total is behind the scan's tile offsets)
        hipLaunchKernelGGL(RepFlagKernel, dim3(Grid(n)), dim3(256), 0, stream, ds->d_mate, n, rep.p);
        GR_CHECK(hipGetLastError(), "RepFlagKernel launch failed");
        GR_CHECK(graphio::DeviceExclusiveScan<int>(rep.p, rank.p, n, sums.p, stream), "MatchingProblem rank scan failed");
        unsigned long long total = 0;
        GR_CHECK(hipMemcpyAsync(&total, sums.p + scan_tiles_n, sizeof(total), hipMemcpyDeviceToHost, stream), "MatchingProblem read total failed");
        GR_CHECK(hipStreamSynchronize(stream), "MatchingProblem Contract sync failed");
        const long long nc = static_cast<long long>(total);
        GR_CHECK(hipMalloc(&ds->d_vweight, sizeof(int) * static_cast<size_t>(nc)), "MatchingProblem hipMalloc failed");
        hipLaunchKernelGGL(MapKernel, dim3(Grid(n)), dim3(256), 0, stream, ds->d_mate, rank.p, d_vertex_weights, n, ds->d_map, ds->d_vweight,
                           ds->d_words + W_FLAG);
        GR_CHECK(hipGetLastError(), "MapKernel launch failed");

        // the coarse pairs: the fine pairs' images as keys, then the build's steps on them
        graphio::PairGraph pg(nc);
        if (M > 0) {
            if ((retval = pg.Reserve(M))) return retval;
            hipLaunchKernelGGL(CoarseKeysKernel, dim3(Grid(M)), dim3(256), 0, stream, ds->d_src, ds->d_dst, ds->d_map, M, pg.col_bits, pg.sentinel,
                               pg.sort.Keys());
            GR_CHECK(hipGetLastError(), "CoarseKeysKernel launch failed");
            if ((retval = pg.SortKeys(stream))) return retval;
            if ((retval = pg.Pairs(stream))) return retval;
        }
        const long long Mc = pg.pairs;
        if (Mc > 0) {
            if ((retval = w64.Alloc(static_cast<size_t>(Mc)))) return retval;
            GR_CHECK(hipMemsetAsync(w64.p, 0, sizeof(unsigned long long) * static_cast<size_t>(Mc), stream), "MatchingProblem memset failed");
            hipLaunchKernelGGL(CoarseWeightKernel, dim3(Grid(M)), dim3(256), 0, stream, ds->d_src, ds->d_dst, ds->d_pw, ds->d_map, M, pg.col_bits,
                               pg.sentinel, pg.d_ckeys, Mc, w64.p);
            GR_CHECK(hipGetLastError(), "CoarseWeightKernel launch failed");
        }
        if ((retval = pg.Rows(stream))) return retval;
        ds->d_cro = graphio::Take(pg.d_ro);
        ds->d_cci = graphio::Take(pg.d_ci);
        if (Mc > 0) {
            GR_CHECK(hipMalloc(&ds->d_cw, sizeof(int) * 2 * static_cast<size_t>(Mc)), "MatchingProblem hipMalloc failed");
            hipLaunchKernelGGL(CoarseEntriesKernel, dim3(Grid(2 * Mc)), dim3(256), 0, stream, pg.d_eid, w64.p, 2 * Mc, ds->d_cw, ds->d_words + W_FLAG);
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
        if ((retval = Read(h_map, ds->d_map, static_cast<size_t>(this->nodes)))) return retval;
        if ((retval = Read(h_ro, ds->d_cro, nc + 1))) return retval;
        if ((retval = Read(h_ci, ds->d_cci, entries))) return retval;
        if ((retval = Read(h_w, ds->d_cw, entries))) return retval;
        return Read(h_vweight, ds->d_vweight, nc);
    }
};

}  // namespace matching
}  // namespace app
}  // namespace gunrock
