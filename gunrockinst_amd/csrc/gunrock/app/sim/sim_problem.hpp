// app/sim/sim_problem.hpp -- device data for vertex similarity.
//
// The reference snapshot has no app/sim; the shape is app/c4/c4_problem.hpp's.  The input CSR is read as TC reads it: an undirected
// simple graph G in which u and v are neighbours when either row holds the other, self-loops ignored, unsorted rows, duplicates and
// one-way edges allowed.  Init:
//   1. graphio::PairGraph up to Rows: the neighbour CSR of G, rows ascending by id, which stays resident
//   2. Wd(u) = the sum of d(v) over row u, their sum and the largest (WedgeKernel)
// The queries of an Enact -- pairs or sources -- that come from the host are staged in arrays of the problem; the result arrays grow
// with the largest query so far and are kept between Enacts.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/sim/sim_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace sim {

template <bool _USE_DOUBLE_BUFFER>
struct SimProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_ro;  // the neighbour CSR of G
        DeviceArray<int> d_ci;
        DeviceArray<int> d_wd;  // Wd per vertex
        DeviceArray<unsigned long long> d_words;  // W_COUNT words of the kernels, then [0] the sum of Wd, [1] the largest
        Grown<int> staged_u, staged_v;          // queries given on the host
        Grown<int> pair_common;                 // pair mode's result
        Grown<long long> pair_num, pair_den;
        Grown<int> ids, common, count, candidates, lists;  // top-k mode's result: S x k, S x k, S, S; 2 S of row lists
        Grown<long long> num, den;
        Grown<int> rows;  // the GLOBAL regime's counter rows, grown by Enact, all 0 between launches
    };

    SliceHolder<DataSlice> data_slices;
    long long simple_edges = 0;  // M
    long long wedges = 0;        // the sum of Wd
    long long max_wedges = 0;    // the largest Wd
    long long pairs = -1;        // of the last finished pair Enact, or -1
    long long sources = -1;      // of the last finished top-k Enact, or -1
    int k = 0;                   // ... and its k
    double build_ms = 0;         // HIP-event time of the build

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT + 2))) return retval;

        // 1. the CSR must be one: the build indexes with what it reads
        if ((retval = this->ValidateCsr())) return retval;

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;

        if ((retval = ds->d_wd.Alloc(n1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_wd, 0, sizeof(int) * n1, stream), "SimProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * (W_COUNT + 2), stream), "SimProblem memset failed");

        // 2. the rows
        graphio::PairGraph pg(n);
        if ((retval = pg.Keys(gs->d_row_offsets, gs->d_column_indices, m, stream))) return retval;
        if ((retval = pg.Pairs(stream))) return retval;
        if ((retval = pg.Rows(stream))) return retval;
        simple_edges = pg.pairs;
        // 3. Wd
        if (simple_edges > 0) {
            const long long blocks = (n + kSimWaves - 1) / kSimWaves;
            hipLaunchKernelGGL(WedgeKernel, dim3(static_cast<unsigned>(blocks < 4096 ? blocks : 4096)), dim3(kSimThreads), 0, stream, pg.d_ro, pg.d_ci,
                               static_cast<int>(n), ds->d_wd, ds->d_words + W_COUNT);
            GR_CHECK(hipGetLastError(), "WedgeKernel launch failed");
        }
        unsigned long long summary[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(summary, ds->d_words + W_COUNT, sizeof(summary), hipMemcpyDeviceToHost, stream), "SimProblem read-back failed");
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "SimProblem build sync failed");  // (the sorts' buffers go behind this)
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        ds->d_ro.Adopt(graphio::Take(pg.d_ro));
        ds->d_ci.Adopt(graphio::Take(pg.d_ci));
        wedges = static_cast<long long>(summary[0]);
        max_wedges = static_cast<long long>(summary[1]);
        return retval;
    }

    // One Init per object (grx_sim_init refuses a second one)
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

    // no result
    hipError_t Reset(FrontierType /*frontier_type*/ = VERTEX_FRONTIERS)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "SimProblem memset failed");
        GR_CHECK(hipStreamSynchronize(stream), "SimProblem Reset sync failed");
        pairs = sources = -1;
        k = 0;
        return retval;
    }

    // count > 0 ids of the host into the staging arrays (h_v may be NULL)
    hipError_t Stage(long long count, const int *h_u, const int *h_v)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t bytes = sizeof(int) * static_cast<size_t>(count);
        if ((retval = ds->staged_u.Need(static_cast<size_t>(count)))) return retval;
        GR_CHECK(hipMemcpyAsync(ds->staged_u.p, h_u, bytes, hipMemcpyHostToDevice, stream), "SimProblem stage failed");
        if (h_v) {
            if ((retval = ds->staged_v.Need(static_cast<size_t>(count)))) return retval;
            GR_CHECK(hipMemcpyAsync(ds->staged_v.p, h_v, bytes, hipMemcpyHostToDevice, stream), "SimProblem stage failed");
        }
        GR_CHECK(hipStreamSynchronize(stream), "SimProblem stage sync failed");  // (the host arrays are the caller's again)
        return retval;
    }

    // Any may be NULL.  The score is one IEEE division of the two integers (both below 2^53), on the host; 0 / 0 is 0.
    static void Scores(size_t count, const long long *num, const long long *den, double *score)
    {
        for (size_t i = 0; i < count; ++i) score[i] = den[i] ? static_cast<double>(num[i]) / static_cast<double>(den[i]) : 0.0;
    }

    hipError_t ExtractPairs(int *h_common, long long *h_num, long long *h_den, double *h_score)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t count = static_cast<size_t>(pairs > 0 ? pairs : 0);
        std::vector<long long> num, den;
        if (h_score && !h_num) num.resize(count), h_num = num.data();
        if (h_score && !h_den) den.resize(count), h_den = den.data();
        if ((retval = this->Read(h_common, ds->pair_common.p, count))) return retval;
        if ((retval = this->Read(h_num, ds->pair_num.p, count))) return retval;
        if ((retval = this->Read(h_den, ds->pair_den.p, count))) return retval;
        if (h_score) Scores(count, h_num, h_den, h_score);
        return retval;
    }

    hipError_t ExtractTopk(int *h_ids, int *h_common, long long *h_num, long long *h_den, double *h_score, int *h_count, int *h_candidates)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t rows = static_cast<size_t>(sources > 0 ? sources : 0), count = rows * static_cast<size_t>(k);
        std::vector<long long> num, den;
        if (h_score && !h_num) num.resize(count), h_num = num.data();
        if (h_score && !h_den) den.resize(count), h_den = den.data();
        if ((retval = this->Read(h_ids, ds->ids.p, count))) return retval;
        if ((retval = this->Read(h_common, ds->common.p, count))) return retval;
        if ((retval = this->Read(h_num, ds->num.p, count))) return retval;
        if ((retval = this->Read(h_den, ds->den.p, count))) return retval;
        if ((retval = this->Read(h_count, ds->count.p, rows))) return retval;
        if ((retval = this->Read(h_candidates, ds->candidates.p, rows))) return retval;
        if (h_score) Scores(count, h_num, h_den, h_score);
        return retval;
    }
};

}  // namespace sim
}  // namespace app
}  // namespace gunrock
