// app/pr/pr_problem.hpp -- device data for PageRank.
//
// Contract of the reference's PRProblem (gunrock/app/pr/pr_problem.cuh:36-467):
//   DataSlice { d_rank_curr, d_rank_next, d_degrees, d_degrees_pong, d_node_ids, delta, threshold, src_node }   (:57-68)
//   Init(stream_from_host, graph, num_gpus)                                                                  (:186-307)
//   Reset(src, delta, threshold, frontier_type): rank_curr = 1 - delta, degrees = out-degrees, node_ids = iota,
//        queue = every vertex                                                                                (:316-457)
//   Extract(h_rank, h_node_id): ranks sorted descending with their vertex ids                                (:139-175)
// Differences: delta / threshold / src_node travel by value inside the DataSlice kernel argument (the reference keeps
// one-element device arrays for them); contrib[v] = rank[v] / degree[v] is kept next to the ranks because ranks are pulled
// over the IN-neighbour lists (pr_functor.hpp), which needs the inverse graph: the caller's CSC, the CSR itself when the
// graph is symmetric, or a transpose built on the device.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/graphio/device_sort.hpp>
#include <gunrock/util/memset_kernel.hpp>

namespace gunrock {
namespace app {
namespace pr {

template <typename SizeT>
__global__ void OutDegreeKernel(const SizeT *d_row_offsets, long long nodes, SizeT *d_degrees, SizeT *d_degrees_pong)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const SizeT d = d_row_offsets[v + 1] - d_row_offsets[v];
        d_degrees[v] = d;
        d_degrees_pong[v] = d;
    }
}

template <typename _VertexId, typename _SizeT, typename _Value>
struct PRProblem : ProblemBase<_VertexId, _SizeT, _Value, false> {
    typedef ProblemBase<_VertexId, _SizeT, _Value, false> Base;
    typedef _VertexId VertexId;
    typedef _SizeT SizeT;
    typedef _Value Value;
    static constexpr bool MARK_PREDECESSORS = false;
    static constexpr bool ENABLE_IDEMPOTENCE = false;

    struct DataSlice {
        Value *d_rank_curr = nullptr;     // rank per vertex
        Value *d_rank_next = nullptr;     // sum of the in-neighbours' contributions (the reducing advance writes it)
        Value *d_contrib = nullptr;       // rank_curr / degree of the vertices that still have out-edges
        SizeT *d_degrees = nullptr;       // out-degree after peeling (-1: peeled off)
        SizeT *d_degrees_pong = nullptr;
        int *d_zero_flag = nullptr;       // peeling round: 1 = lost its last out-edge in the previous round
        int *d_zero_count = nullptr;      // peeling round: per queue position, out-neighbours with the flag set
        VertexId *d_node_ids = nullptr;   // vertex ids by descending rank (after Enact)
        Value *d_rank_sorted = nullptr;   // their ranks
        Value delta = 0;
        Value threshold = 0;
        VertexId src_node = -1;
    };
    static_assert(std::is_trivially_copyable<DataSlice>::value,
                  "the DataSlice is copied into kernel arguments and functors: views only, the owners sit in the problem");

    SliceHolder<DataSlice> data_slices;
    DataSlice **d_data_slices = nullptr;  // kept for source compatibility; unused
    // what the slice views, under the slice's names
    DeviceArray<Value> d_rank_curr, d_rank_next, d_contrib, d_rank_sorted;
    DeviceArray<SizeT> d_degrees, d_degrees_pong;
    DeviceArray<int> d_zero_flag, d_zero_count;
    DeviceArray<VertexId> d_node_ids;
    const SizeT *d_inv_row_offsets = nullptr;  // in-neighbour lists
    const VertexId *d_inv_column_indices = nullptr;
    DeviceArray<SizeT> d_own_inv_row_offsets;  // the transpose when BuildInverse made it
    DeviceArray<VertexId> d_own_inv_column_indices;
    util::Frontier<VertexId, SizeT> inv_frontier;  // surviving vertices with the degree prefix of their in-lists
    FrontierStorage<VertexId, SizeT> inv_storage;  // (inv_frontier is its view)
    graphio::DeviceKeySort sorter;

    hipError_t AllocData()
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices.Make();
        const size_t n = static_cast<size_t>(this->nodes > 0 ? this->nodes : 1);
        GR_CHECK(d_rank_curr.Alloc(n), "PRProblem d_rank_curr failed");
        GR_CHECK(d_rank_next.Alloc(n), "PRProblem d_rank_next failed");
        GR_CHECK(d_contrib.Alloc(n), "PRProblem d_contrib failed");
        GR_CHECK(d_rank_sorted.Alloc(n), "PRProblem d_rank_sorted failed");
        GR_CHECK(d_degrees.Alloc(n), "PRProblem d_degrees failed");
        GR_CHECK(d_degrees_pong.Alloc(n), "PRProblem d_degrees_pong failed");
        GR_CHECK(d_zero_flag.Alloc(n), "PRProblem d_zero_flag failed");
        GR_CHECK(d_zero_count.Alloc(n), "PRProblem d_zero_count failed");
        GR_CHECK(d_node_ids.Alloc(n), "PRProblem d_node_ids failed");
        ds->d_rank_curr = d_rank_curr;
        ds->d_rank_next = d_rank_next;
        ds->d_contrib = d_contrib;
        ds->d_rank_sorted = d_rank_sorted;
        ds->d_degrees = d_degrees;
        ds->d_degrees_pong = d_degrees_pong;
        ds->d_zero_flag = d_zero_flag;
        ds->d_zero_count = d_zero_count;
        ds->d_node_ids = d_node_ids;
        retval = inv_storage.Grow(static_cast<SizeT>(n + 1));
        inv_frontier = inv_storage.view;
        if (retval) return util::GRError(retval, "PRProblem inverse frontier failed", __FILE__, __LINE__);
        return retval;
    }

    hipError_t Init(bool stream_from_host, const Csr<VertexId, Value, SizeT> &graph, int num_gpus = 1)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Init(stream_from_host, graph, num_gpus))) return retval;
        return AllocData();
    }
    hipError_t InitFromDevice(SizeT nodes, SizeT edges, SizeT *d_row_offsets, VertexId *d_column_indices)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::InitFromDevice(nodes, edges, d_row_offsets, d_column_indices))) return retval;
        return AllocData();
    }

    // In-neighbour lists: borrowed CSC arrays in HBM ...
    void SetInverseGraph(const SizeT *d_iro, const VertexId *d_ici)
    {
        d_inv_row_offsets = d_iro;
        d_inv_column_indices = d_ici;
    }
    // ... the graph's own CSR (symmetric input) ...
    void InverseIsSelf() { SetInverseGraph(this->graph_slices[0]->d_row_offsets, this->graph_slices[0]->d_column_indices); }
    // ... or the transpose, built on the device
    hipError_t BuildInverse()
    {
        hipError_t retval = hipSuccess;
        GraphSlice<VertexId, SizeT, Value> *gs = this->graph_slices[0];
        // (every build: what an earlier one made goes, so the arrays always have this graph's size)
        GR_CHECK(d_own_inv_row_offsets.Alloc(static_cast<size_t>(this->nodes) + 2), "PRProblem inverse offsets failed");
        GR_CHECK(d_own_inv_column_indices.Alloc(static_cast<size_t>(this->edges)), "PRProblem inverse columns failed");
        GR_CHECK(graphio::DeviceTransposeCsr(this->nodes, this->edges, gs->d_row_offsets, gs->d_column_indices, d_own_inv_row_offsets,
                                             d_own_inv_column_indices, gs->stream),
                 "PRProblem transpose failed");
        SetInverseGraph(d_own_inv_row_offsets, d_own_inv_column_indices);
        return retval;
    }

    hipError_t Reset(VertexId src, Value delta, Value threshold, FrontierType frontier_type)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Base::Reset(frontier_type, 1.0))) return retval;  // "Default queue sizing is 1.0" (pr_problem.cuh:326)
        GraphSlice<VertexId, SizeT, Value> *gs = this->graph_slices[0];
        DataSlice *ds = data_slices[0];
        hipStream_t stream = gs->stream;
        ds->delta = delta;
        ds->threshold = threshold;
        ds->src_node = src;
        if (this->nodes > 0) {
            util::Memset(ds->d_rank_curr, static_cast<Value>(1.0 - delta), this->nodes, stream);  // pr_problem.cuh:423
            util::Memset(ds->d_rank_next, static_cast<Value>(0), this->nodes, stream);
            util::Memset(ds->d_contrib, static_cast<Value>(0), this->nodes, stream);
            util::MemsetIdx(ds->d_node_ids, this->nodes, stream);
            hipLaunchKernelGGL((OutDegreeKernel<SizeT>), dim3(1024), dim3(256), 0, stream, gs->d_row_offsets, static_cast<long long>(this->nodes),
                               ds->d_degrees, ds->d_degrees_pong);
            GR_CHECK(hipGetLastError(), "OutDegreeKernel launch failed");
        }
        return retval;
    }

    // ranks in descending order with their vertex ids, as the reference returns them; `count` <= nodes entries
    hipError_t Extract(Value *h_rank, VertexId *h_node_id, SizeT count = -1)
    {
        hipError_t retval = hipSuccess;
        DataSlice *ds = data_slices[0];
        GR_CHECK(hipStreamSynchronize(this->graph_slices[0]->stream), "PRProblem Extract sync failed");
        if (count < 0 || count > this->nodes) count = this->nodes;
        if (count > 0 && h_rank)
            GR_CHECK(hipMemcpy(h_rank, ds->d_rank_sorted, sizeof(Value) * static_cast<size_t>(count), hipMemcpyDeviceToHost), "PRProblem hipMemcpy failed");
        if (count > 0 && h_node_id)
            GR_CHECK(hipMemcpy(h_node_id, ds->d_node_ids, sizeof(VertexId) * static_cast<size_t>(count), hipMemcpyDeviceToHost), "PRProblem hipMemcpy failed");
        return retval;
    }
};

}  // namespace pr
}  // namespace app
}  // namespace gunrock
