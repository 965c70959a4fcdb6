// app/rw/rw_problem.hpp -- device data for random walks.
//
// The reference snapshot has no app/rw; the shape is app/c4/c4_problem.hpp's.  The input CSR is taken as given: directed, self-loops
// and duplicates kept.  Init validates it (a negative weight is malformed too) and builds the copy the walks read:
//   unweighted  the keys (row << cb | column) sorted once: the rows in order, ascending columns
//   weighted    three sorts of (field << eb | rank), each ranking the entries by one more field: by (weight, entry), then by
//               (column, that rank), then by (row, that rank).  The last is the order of the copy -- rows by (column, weight) -- and
//               the sorted arrays of the first two give the column and the weight of every position back.  No key holds more than
//               31 + 31 bits, whatever the graph.
//   prefix[]    per entry, the inclusive int64 sum of the weights of its row up to it (one wave a row)
// The caller's CSR is read by the build alone.  Reset takes the start vertices, Enact (re)allocates the pitched walks.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/rw/rw_build.hpp>
#include <gunrock/app/rw/rw_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace rw {

// ---------------- build kernels (the ones of the weighted order: rw_build.hpp) ----------------

static __global__ void RowColumnKeysKernel(const int *ro, const int *ci, int nodes, long long m, int cb, unsigned long long *keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride)
        keys[i] = (static_cast<unsigned long long>(RowOf(ro, nodes, i)) << cb) | static_cast<unsigned long long>(ci[i]);
}

static __global__ void ColumnsOfKeysKernel(const unsigned long long *keys, long long m, int cb, int *ci)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride)
        ci[i] = static_cast<int>(keys[i] & ((1ull << cb) - 1));
}

template <bool _USE_DOUBLE_BUFFER>
struct RwProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_ro;  // the sorted copy
        DeviceArray<int> d_ci;
        DeviceArray<int> d_w;
        DeviceArray<long long> d_prefix;
        DeviceArray<int> d_starts;
        DeviceArray<int> d_lengths;
        DeviceArray<int> d_walks;  // num_walks x pitch, (re)allocated by Enact
        size_t walk_ints = 0;
        DeviceArray<unsigned long long> d_visits;  // allocated by the first Enact that counts them
        DeviceArray<unsigned long long> d_words;
    };

    SliceHolder<DataSlice> data_slices;
    bool weights = false;      // Init had weights
    long long num_walks = 0;   // of the last Reset
    long long pitch = 0;       // of the last Enact
    double build_ms = 0;

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GraphSlice<int, int, int> *gs = this->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = this->nodes, m = this->edges;
        const size_t n1 = static_cast<size_t>(n > 0 ? n : 1), m1 = static_cast<size_t>(m > 0 ? m : 1);
        weights = gs->d_edge_values != nullptr;

        if ((retval = this->ValidateCsr())) return retval;
        if (weights && m > 0) {
            int negative = 0;
            graphio::DeviceScratch<int> flag;
            if ((retval = flag.Alloc(1))) return retval;
            GR_CHECK(hipMemsetAsync(flag.p, 0, sizeof(int), stream), "RwProblem memset failed");
            hipLaunchKernelGGL(NegativeWeightKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, gs->d_edge_values, m, flag.p);
            GR_CHECK(hipGetLastError(), "NegativeWeightKernel launch failed");
            GR_CHECK(hipMemcpyAsync(&negative, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream), "RwProblem read-back failed");
            GR_CHECK(hipStreamSynchronize(stream), "RwProblem read-back sync failed");
            if (negative) return this->Malformed();
        }

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;

        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        if ((retval = ds->d_ro.Alloc(n1 + 1))) return retval;
        if ((retval = ds->d_ci.Alloc(m1))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "RwProblem memset failed");
        GR_CHECK(hipMemcpyAsync(ds->d_ro, gs->d_row_offsets, sizeof(int) * (n1 + 1), hipMemcpyDeviceToDevice, stream), "RwProblem copy failed");
        if (weights) {
            if ((retval = ds->d_w.Alloc(m1))) return retval;
            if ((retval = ds->d_prefix.Alloc(m1))) return retval;
        }
        graphio::DeviceKeySort sort_a, sort_b, sort_c;  // (their buffers go behind the sync below)
        if (m > 0) {
            const int grid_m = graphio::PairGrid(m);
            const int nodes = static_cast<int>(n), cb = BitsFor(n), eb = BitsFor(m);
            unsigned long long *a = nullptr, *b = nullptr, *c = nullptr;
            if (!weights) {
                GR_CHECK(sort_c.Reserve(m), "RwProblem sort scratch failed");
                hipLaunchKernelGGL(RowColumnKeysKernel, dim3(grid_m), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices, nodes, m, cb,
                                   sort_c.Keys());
                GR_CHECK(hipGetLastError(), "RowColumnKeysKernel launch failed");
                GR_CHECK(sort_c.Sort(m, 2 * cb, stream, &c), "RwProblem sort failed");
                hipLaunchKernelGGL(ColumnsOfKeysKernel, dim3(grid_m), dim3(256), 0, stream, c, m, cb, ds->d_ci);
                GR_CHECK(hipGetLastError(), "ColumnsOfKeysKernel launch failed");
            } else {
                GR_CHECK(sort_a.Reserve(m), "RwProblem sort scratch failed");
                GR_CHECK(sort_b.Reserve(m), "RwProblem sort scratch failed");
                GR_CHECK(sort_c.Reserve(m), "RwProblem sort scratch failed");
                hipLaunchKernelGGL(WeightKeysKernel, dim3(grid_m), dim3(256), 0, stream, gs->d_edge_values, m, eb, sort_a.Keys());
                GR_CHECK(hipGetLastError(), "WeightKeysKernel launch failed");
                GR_CHECK(sort_a.Sort(m, 31 + eb, stream, &a), "RwProblem sort failed");
                hipLaunchKernelGGL(ColumnKeysKernel, dim3(grid_m), dim3(256), 0, stream, a, gs->d_column_indices, m, eb, sort_b.Keys());
                GR_CHECK(hipGetLastError(), "ColumnKeysKernel launch failed");
                GR_CHECK(sort_b.Sort(m, cb + eb, stream, &b), "RwProblem sort failed");
                hipLaunchKernelGGL(RowKeysKernel, dim3(grid_m), dim3(256), 0, stream, a, b, gs->d_row_offsets, nodes, m, eb, sort_c.Keys());
                GR_CHECK(hipGetLastError(), "RowKeysKernel launch failed");
                GR_CHECK(sort_c.Sort(m, cb + eb, stream, &c), "RwProblem sort failed");
                hipLaunchKernelGGL(SortedEntriesKernel, dim3(grid_m), dim3(256), 0, stream, a, b, c, m, eb, ds->d_ci, ds->d_w);
                GR_CHECK(hipGetLastError(), "SortedEntriesKernel launch failed");
                hipLaunchKernelGGL(RowPrefixKernel, dim3(graphio::PairGrid(n * 64)), dim3(256), 0, stream, ds->d_ro, ds->d_w, nodes, ds->d_prefix);
                GR_CHECK(hipGetLastError(), "RowPrefixKernel launch failed");
            }
        }
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "RwProblem build sync failed");
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        return retval;
    }

    // One Init per object (grx_rw_init refuses a second one)
    hipError_t Init(bool stream_from_host, const Csr<int, int, int> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus, true))) return retval;
        data_slices.Make();
        return Build();
    }

    hipError_t InitFromDevice(int nodes, int edges, int *d_row_offsets, int *d_column_indices, int *d_weights)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices, d_weights))) return retval;
        data_slices.Make();
        return Build();
    }

    // the start vertices (checked by the caller against the vertex range)
    hipError_t Reset(long long walks, const int *h_starts)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if (walks != num_walks) {
            num_walks = 0;
            if ((retval = ds->d_starts.Alloc(static_cast<size_t>(walks)))) return retval;
            if ((retval = ds->d_lengths.Alloc(static_cast<size_t>(walks)))) return retval;
            num_walks = walks;
        }
        GR_CHECK(hipMemcpyAsync(ds->d_starts, h_starts, sizeof(int) * static_cast<size_t>(walks), hipMemcpyHostToDevice, stream),
                 "RwProblem copy of the start vertices failed");
        GR_CHECK(hipStreamSynchronize(stream), "RwProblem Reset sync failed");
        return retval;
    }

    // room for num_walks rows of `row_pitch` entries
    hipError_t NeedWalks(long long row_pitch)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t need = static_cast<size_t>(num_walks) * static_cast<size_t>(row_pitch);
        if (need > ds->walk_ints) {
            ds->walk_ints = 0;
            if ((retval = ds->d_walks.Alloc(need))) return retval;
            ds->walk_ints = need;
        }
        pitch = row_pitch;
        return retval;
    }

    hipError_t NeedVisits()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if (!ds->d_visits && (retval = ds->d_visits.Alloc(static_cast<size_t>(this->nodes)))) return retval;
        return retval;
    }

    // any pointer may be NULL; `length` is the last Enact's
    hipError_t Extract(int length, int *h_walks, int *h_lengths, long long *h_visits)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t row_bytes = sizeof(int) * static_cast<size_t>(length + 1);
        if (h_walks)
            GR_CHECK(hipMemcpy2DAsync(h_walks, row_bytes, ds->d_walks, sizeof(int) * static_cast<size_t>(pitch), row_bytes, static_cast<size_t>(num_walks),
                                      hipMemcpyDeviceToHost, stream),
                     "RwProblem read d_walks failed");
        if (h_lengths)
            GR_CHECK(hipMemcpyAsync(h_lengths, ds->d_lengths, sizeof(int) * static_cast<size_t>(num_walks), hipMemcpyDeviceToHost, stream),
                     "RwProblem read d_lengths failed");
        if (h_visits)
            GR_CHECK(hipMemcpyAsync(h_visits, ds->d_visits, sizeof(long long) * static_cast<size_t>(this->nodes), hipMemcpyDeviceToHost, stream),
                     "RwProblem read d_visits failed");
        GR_CHECK(hipStreamSynchronize(stream), "RwProblem Extract sync failed");
        return retval;
    }
};

}  // namespace rw
}  // namespace app
}  // namespace gunrock
