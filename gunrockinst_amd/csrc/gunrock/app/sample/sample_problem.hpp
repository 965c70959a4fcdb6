// app/sample/sample_problem.hpp -- device data for neighbourhood sampling.
//
// The reference snapshot has no app/sample; the shape is app/rw/rw_problem.hpp's, and the build is its build with the entry kept.
// The input CSR is taken as given.  Init validates it (a negative weight is malformed too) and builds the copy the sampler reads,
// every row sorted by (column, weight, entry), with rw's rank sorts of (field << eb | rank):
//   unweighted  by (column, entry), then by (row, that rank): two sorts
//   weighted    rw's three: by (weight, entry), by (column, that rank), by (row, that rank)
// The sorted arrays of the earlier sorts give the column, the weight and the caller's entry of every position back: ci[], w[], ent[].
// prefix[] is rw's inclusive int64 weight prefix per row.  local[] holds the local id of every vertex, -1 without one; a bitmap of
// `nodes` bits marks the new vertices of a hop.  Reset takes the seeds and clears local[] by walking the vertices of the sample
// before, never the whole array.  The result arrays grow as the hops find out how much they hold.
#pragma once

#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/rw/rw_build.hpp>
#include <gunrock/app/sample/sample_functor.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace sample {

// ---------------- build kernels (next to rw_problem.hpp's) ----------------

// B: (column << eb | entry)
static __global__ void ColumnEntryKeysKernel(const int *ci, long long m, int eb, unsigned long long *keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride)
        keys[i] = (static_cast<unsigned long long>(ci[i]) << eb) | static_cast<unsigned long long>(i);
}

// C: (row << eb | rank in B)
static __global__ void RowRankKeysKernel(const unsigned long long *b, const int *ro, int nodes, long long m, int eb, unsigned long long *keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << eb) - 1;
    for (long long q = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; q < m; q += stride)
        keys[q] = (static_cast<unsigned long long>(rw::RowOf(ro, nodes, static_cast<long long>(b[q] & mask))) << eb) | static_cast<unsigned long long>(q);
}

static __global__ void SortedColumnEntryKernel(const unsigned long long *b, const unsigned long long *c, long long m, int eb, int *ci, int *ent)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << eb) - 1;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride) {
        const unsigned long long kb = b[c[i] & mask];
        ci[i] = static_cast<int>(kb >> eb);
        ent[i] = static_cast<int>(kb & mask);
    }
}

// the entry rw's SortedEntriesKernel drops: behind the three sorts, position i holds entry a[b[c[i]]]
static __global__ void SortedEntryKernel(const unsigned long long *a, const unsigned long long *b, const unsigned long long *c, long long m, int eb,
                                         int *ent)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << eb) - 1;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride)
        ent[i] = static_cast<int>(a[b[c[i] & mask] & mask] & mask);
}

template <bool _USE_DOUBLE_BUFFER>
struct SampleProblem : ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> {
    typedef ProblemBase<int, int, int, _USE_DOUBLE_BUFFER> Base;

    struct DataSlice {
        DeviceArray<int> d_ro;  // the sorted copy
        DeviceArray<int> d_ci;
        DeviceArray<int> d_ent;
        DeviceArray<int> d_w;
        DeviceArray<long long> d_prefix;
        DeviceArray<int> d_local;
        DeviceArray<unsigned> d_bitmap;  // words32 words
        DeviceArray<unsigned> d_bit_counts;
        DeviceArray<unsigned long long> d_bit_base;
        DeviceArray<unsigned long long> d_bit_sums;  // the new vertices of a hop behind its tile offsets
        DeviceArray<unsigned long long> d_words;
        // per frontier row (NeedFrontier)
        DeviceArray<unsigned> d_counts;
        DeviceArray<unsigned long long> d_row_base;
        DeviceArray<unsigned long long> d_count_sums;  // the edges of a hop behind its tile offsets
        DeviceArray<int> d_long_rows;
        size_t frontier_cap = 0;
        // the sample (NeedVertices / NeedEdges)
        DeviceArray<int> d_vertices;
        DeviceArray<long long> d_offsets;
        DeviceArray<int> d_cols;
        DeviceArray<int> d_eids;
        size_t vertex_cap = 0, offset_cap = 0, col_cap = 0, eid_cap = 0;
    };

    SliceHolder<DataSlice> data_slices;
    bool weights = false;  // Init had weights
    long long words32 = 0;
    long long num_seeds = 0;  // of the last Reset
    // of the last Enact (the seeds alone behind a Reset)
    long long num_vertices = 0, num_edges = 0;
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
            GR_CHECK(hipMemsetAsync(flag.p, 0, sizeof(int), stream), "SampleProblem memset failed");
            hipLaunchKernelGGL(rw::NegativeWeightKernel, dim3(graphio::PairGrid(m)), dim3(256), 0, stream, gs->d_edge_values, m, flag.p);
            GR_CHECK(hipGetLastError(), "NegativeWeightKernel launch failed");
            GR_CHECK(hipMemcpyAsync(&negative, flag.p, sizeof(int), hipMemcpyDeviceToHost, stream), "SampleProblem read-back failed");
            GR_CHECK(hipStreamSynchronize(stream), "SampleProblem read-back sync failed");
            if (negative) return this->Malformed();
        }

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;

        words32 = (n + 31) / 32;
        const size_t w1 = static_cast<size_t>(words32 > 0 ? words32 : 1);
        if ((retval = ds->d_words.Alloc(W_COUNT))) return retval;
        if ((retval = ds->d_ro.Alloc(n1 + 1))) return retval;
        if ((retval = ds->d_ci.Alloc(m1))) return retval;
        if ((retval = ds->d_ent.Alloc(m1))) return retval;
        if ((retval = ds->d_local.Alloc(n1))) return retval;
        if ((retval = ds->d_bitmap.Alloc(w1))) return retval;
        if ((retval = ds->d_bit_counts.Alloc(w1))) return retval;
        if ((retval = ds->d_bit_base.Alloc(w1))) return retval;
        if ((retval = ds->d_bit_sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(words32))))) return retval;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "SampleProblem memset failed");
        GR_CHECK(hipMemsetAsync(ds->d_local, 0xff, sizeof(int) * n1, stream), "SampleProblem memset failed");  // the one whole-array clear
        GR_CHECK(hipMemsetAsync(ds->d_bitmap, 0, sizeof(unsigned) * w1, stream), "SampleProblem memset failed");
        GR_CHECK(hipMemcpyAsync(ds->d_ro, gs->d_row_offsets, sizeof(int) * (n1 + 1), hipMemcpyDeviceToDevice, stream), "SampleProblem copy failed");
        if (weights) {
            if ((retval = ds->d_w.Alloc(m1))) return retval;
            if ((retval = ds->d_prefix.Alloc(m1))) return retval;
        }
        graphio::DeviceKeySort sort_a, sort_b, sort_c;  // (their buffers go behind the sync below)
        if (m > 0) {
            const int grid_m = graphio::PairGrid(m);
            const int nodes = static_cast<int>(n), cb = rw::BitsFor(n), eb = rw::BitsFor(m);
            unsigned long long *a = nullptr, *b = nullptr, *c = nullptr;
            GR_CHECK(sort_b.Reserve(m), "SampleProblem sort scratch failed");
            GR_CHECK(sort_c.Reserve(m), "SampleProblem sort scratch failed");
            if (!weights) {
                hipLaunchKernelGGL(ColumnEntryKeysKernel, dim3(grid_m), dim3(256), 0, stream, gs->d_column_indices, m, eb, sort_b.Keys());
                GR_CHECK(hipGetLastError(), "ColumnEntryKeysKernel launch failed");
                GR_CHECK(sort_b.Sort(m, cb + eb, stream, &b), "SampleProblem sort failed");
                hipLaunchKernelGGL(RowRankKeysKernel, dim3(grid_m), dim3(256), 0, stream, b, gs->d_row_offsets, nodes, m, eb, sort_c.Keys());
                GR_CHECK(hipGetLastError(), "RowRankKeysKernel launch failed");
                GR_CHECK(sort_c.Sort(m, cb + eb, stream, &c), "SampleProblem sort failed");
                hipLaunchKernelGGL(SortedColumnEntryKernel, dim3(grid_m), dim3(256), 0, stream, b, c, m, eb, ds->d_ci, ds->d_ent);
                GR_CHECK(hipGetLastError(), "SortedColumnEntryKernel launch failed");
            } else {
                GR_CHECK(sort_a.Reserve(m), "SampleProblem sort scratch failed");
                hipLaunchKernelGGL(rw::WeightKeysKernel, dim3(grid_m), dim3(256), 0, stream, gs->d_edge_values, m, eb, sort_a.Keys());
                GR_CHECK(hipGetLastError(), "WeightKeysKernel launch failed");
                GR_CHECK(sort_a.Sort(m, 31 + eb, stream, &a), "SampleProblem sort failed");
                hipLaunchKernelGGL(rw::ColumnKeysKernel, dim3(grid_m), dim3(256), 0, stream, a, gs->d_column_indices, m, eb, sort_b.Keys());
                GR_CHECK(hipGetLastError(), "ColumnKeysKernel launch failed");
                GR_CHECK(sort_b.Sort(m, cb + eb, stream, &b), "SampleProblem sort failed");
                hipLaunchKernelGGL(rw::RowKeysKernel, dim3(grid_m), dim3(256), 0, stream, a, b, gs->d_row_offsets, nodes, m, eb, sort_c.Keys());
                GR_CHECK(hipGetLastError(), "RowKeysKernel launch failed");
                GR_CHECK(sort_c.Sort(m, cb + eb, stream, &c), "SampleProblem sort failed");
                hipLaunchKernelGGL(rw::SortedEntriesKernel, dim3(grid_m), dim3(256), 0, stream, a, b, c, m, eb, ds->d_ci, ds->d_w);
                GR_CHECK(hipGetLastError(), "SortedEntriesKernel launch failed");
                hipLaunchKernelGGL(SortedEntryKernel, dim3(grid_m), dim3(256), 0, stream, a, b, c, m, eb, ds->d_ent);
                GR_CHECK(hipGetLastError(), "SortedEntryKernel launch failed");
                hipLaunchKernelGGL(rw::RowPrefixKernel, dim3(graphio::PairGrid(n * 64)), dim3(256), 0, stream, ds->d_ro, ds->d_w, nodes, ds->d_prefix);
                GR_CHECK(hipGetLastError(), "RowPrefixKernel launch failed");
            }
        }
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "SampleProblem build sync failed");
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;
        return retval;
    }

    // One Init per object (grx_sample_init refuses a second one)
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

    // room for `need` entries behind the `keep` that stay
    template <typename T>
    hipError_t Grow(DeviceArray<T> &p, size_t &cap, size_t need, size_t keep)
    {
        hipError_t retval = hipSuccess;
        if (need <= cap) return retval;
        hipStream_t stream = this->graph_slices[0]->stream;
        size_t room = cap * 2 > need ? cap * 2 : need;
        if (room < 1024) room = 1024;
        DeviceArray<T> q;
        if ((retval = q.Alloc(room))) return retval;
        if (p) {
            // the copy, and whatever queued kernel still reads the old array, are done before it goes
            if (keep) GR_CHECK(hipMemcpyAsync(q.p, p.p, sizeof(T) * keep, hipMemcpyDeviceToDevice, stream), "SampleProblem copy failed");
            GR_CHECK(hipStreamSynchronize(stream), "SampleProblem copy failed");
        }
        p = std::move(q);
        cap = room;
        return retval;
    }

    // room for `vertices` local ids (and one more offset), the first `keep` kept
    hipError_t NeedVertices(long long vertices, long long keep)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if ((retval = Grow(ds->d_vertices, ds->vertex_cap, static_cast<size_t>(vertices), static_cast<size_t>(keep)))) return retval;
        return Grow(ds->d_offsets, ds->offset_cap, static_cast<size_t>(vertices) + 1, static_cast<size_t>(keep) + 1);
    }

    // room for `edges` sampled edges, the first `keep` kept
    hipError_t NeedEdges(long long edges, long long keep, bool with_eids)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        if ((retval = Grow(ds->d_cols, ds->col_cap, static_cast<size_t>(edges), static_cast<size_t>(keep)))) return retval;
        if (with_eids) retval = Grow(ds->d_eids, ds->eid_cap, static_cast<size_t>(edges), static_cast<size_t>(keep));
        return retval;
    }

    // room for a frontier of `rows` vertices: the counts and the row bases hold one entry more
    hipError_t NeedFrontier(long long rows)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        const size_t need = static_cast<size_t>(rows) + 1;
        if (need <= ds->frontier_cap) return retval;
        // (the sampler of the hop before may still be reading the row bases)
        GR_CHECK(hipStreamSynchronize(this->graph_slices[0]->stream), "SampleProblem NeedFrontier sync failed");
        ds->frontier_cap = 0;
        const size_t room = need < 1024 ? 1024 : need + need / 2;
        if ((retval = ds->d_counts.Alloc(room))) return retval;
        if ((retval = ds->d_row_base.Alloc(room))) return retval;
        if ((retval = ds->d_count_sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(static_cast<long long>(room)))))) return retval;
        if ((retval = ds->d_long_rows.Alloc(room))) return retval;
        ds->frontier_cap = room;
        return retval;
    }

    // local[] of the sample's vertices from local id `from` on back to -1
    hipError_t ClearLocal(long long from)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if (num_vertices > from) {
            hipLaunchKernelGGL(ClearLocalKernel, dim3(graphio::PairGrid(num_vertices - from)), dim3(256), 0, stream, ds->d_vertices + from,
                               num_vertices - from, ds->d_local);
            GR_CHECK(hipGetLastError(), "ClearLocalKernel launch failed");
        }
        num_vertices = from < num_vertices ? from : num_vertices;
        num_edges = 0;
        return retval;
    }

    // the seeds: distinct vertices of the graph (checked by the caller), local ids 0 .. seeds - 1 in the given order
    hipError_t Reset(long long seeds, const int *h_seeds)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        if ((retval = ClearLocal(0))) return retval;
        num_seeds = 0;
        if ((retval = NeedVertices(seeds, 0))) return retval;
        GR_CHECK(hipMemcpyAsync(ds->d_vertices, h_seeds, sizeof(int) * static_cast<size_t>(seeds), hipMemcpyHostToDevice, stream),
                 "SampleProblem copy of the seeds failed");
        hipLaunchKernelGGL(SeedLocalKernel, dim3(graphio::PairGrid(seeds)), dim3(256), 0, stream, ds->d_vertices, seeds, ds->d_local);
        GR_CHECK(hipGetLastError(), "SeedLocalKernel launch failed");
        GR_CHECK(hipStreamSynchronize(stream), "SampleProblem Reset sync failed");
        num_seeds = num_vertices = seeds;
        return retval;
    }

    // any pointer may be NULL
    hipError_t Extract(int *h_vertices, long long *h_offsets, int *h_cols, int *h_eids)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        hipStream_t stream = this->graph_slices[0]->stream;
        const size_t v = static_cast<size_t>(num_vertices), e = static_cast<size_t>(num_edges);
        if (h_vertices) GR_CHECK(hipMemcpyAsync(h_vertices, ds->d_vertices, sizeof(int) * v, hipMemcpyDeviceToHost, stream), "SampleProblem read d_vertices failed");
        if (h_offsets)
            GR_CHECK(hipMemcpyAsync(h_offsets, ds->d_offsets, sizeof(long long) * (v + 1), hipMemcpyDeviceToHost, stream), "SampleProblem read d_offsets failed");
        if (h_cols && e) GR_CHECK(hipMemcpyAsync(h_cols, ds->d_cols, sizeof(int) * e, hipMemcpyDeviceToHost, stream), "SampleProblem read d_cols failed");
        if (h_eids && e) GR_CHECK(hipMemcpyAsync(h_eids, ds->d_eids, sizeof(int) * e, hipMemcpyDeviceToHost, stream), "SampleProblem read d_eids failed");
        GR_CHECK(hipStreamSynchronize(stream), "SampleProblem Extract sync failed");
        return retval;
    }
};

}  // namespace sample
}  // namespace app
}  // namespace gunrock
