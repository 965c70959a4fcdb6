// app/problem_base.hpp -- device graph storage and frontier queues shared by all primitives.
//
// Same roles and names as the reference's ProblemBase / GraphSlice / FrontierType
// (gunrock/app/problem_base.cuh:35-39, 73-140, 226-431):
//   ProblemBase::Init  uploads the CSR once (problem_base.cuh:280-303),
//   ProblemBase::Reset sizes the two ping-pong frontier queues from queue_sizing
//                      (VERTEX_FRONTIERS -> nodes, EDGE_FRONTIERS -> edges, MIXED -> both; :378-382).
// MI355X-first differences: a frontier is (vertex, row start, degree prefix) (util/frontier.hpp); the
// graph may already be resident in HBM (InitFromDevice: 288 GB lets callers keep graphs on the card
// between primitives instead of re-uploading over PCIe per call); one HIP stream per problem.
// Multi-GPU: the reference has only a TODO (problem_base.cuh:336-338); vertex-cut partitioning lives
// in the package's multi_gpu layer and hands each rank's LOCAL CSR to this class unchanged.
#pragma once

#include <hip/hip_runtime.h>

#include <utility>

#include <gunrock/csr.hpp>
#include <gunrock/graphio/pair_graph.hpp>
#include <gunrock/util/device_array.hpp>
#include <gunrock/util/error_utils.hpp>
#include <gunrock/util/frontier.hpp>

namespace gunrock {
namespace app {

using util::DeviceArray;

enum FrontierType {
    VERTEX_FRONTIERS,  // O(n) ping-pong frontier queues
    EDGE_FRONTIERS,    // O(m) ping-pong frontier queues
    MIXED_FRONTIERS    // O(n) + O(m)
};

// A frontier queue and its owner, shaped like oprtr::advance::BinPoolStorage: `view` is what kernels take by value, the three
// arrays beside it are what is freed.  Mem as in DeviceArray.
template <typename VertexId, typename SizeT, typename Mem = util::HipMem>
struct FrontierStorage {
    util::Frontier<VertexId, SizeT> view;
    DeviceArray<VertexId, Mem> v;
    DeviceArray<SizeT, Mem> row_start, scan;

    // Room for `elements` entries; a queue that has it stays.  The new arrays come first and the view and its capacity are
    // published only when all three exist: a grow that fails leaves an empty queue, which the next call grows again.
    hipError_t Grow(SizeT elements)
    {
        hipError_t retval = hipSuccess;
        if (view.capacity >= elements) return retval;
        DeviceArray<VertexId, Mem> new_v;
        DeviceArray<SizeT, Mem> new_row_start, new_scan;
        const size_t count = static_cast<size_t>(elements);
        if ((retval = new_v.Alloc(count)) || (retval = new_row_start.Alloc(count)) || (retval = new_scan.Alloc(count))) {
            Free();
            return retval;
        }
        v = std::move(new_v);
        row_start = std::move(new_row_start);
        scan = std::move(new_scan);
        view.v = v;
        view.row_start = row_start;
        view.scan = scan;
        view.capacity = elements;
        return retval;
    }

    void Free()
    {
        view = util::Frontier<VertexId, SizeT>();
        v.Free();
        row_start.Free();
        scan.Free();
    }
};

template <typename VertexId, typename SizeT, typename Value>
struct GraphSlice {
    int index = 0;
    SizeT nodes = 0;
    SizeT edges = 0;
    // the CSR the kernels read: views of the arrays below (Init uploaded them) or of the caller's (InitFromDevice: borrowed)
    SizeT *d_row_offsets = nullptr;
    VertexId *d_column_indices = nullptr;
    Value *d_edge_values = nullptr;  // only when a primitive asks for weights
    DeviceArray<SizeT> own_row_offsets;
    DeviceArray<VertexId> own_column_indices;
    DeviceArray<Value> own_edge_values;

    util::Frontier<VertexId, SizeT> frontier_queues[2];  // = queue_storage[i].view as of the last Reset: the kernel argument
    FrontierStorage<VertexId, SizeT> queue_storage[2];
    hipStream_t stream = 0;

    GraphSlice() = default;
    GraphSlice(const GraphSlice &) = delete;
    GraphSlice &operator=(const GraphSlice &) = delete;
    ~GraphSlice()
    {
        if (stream) util::GRError(hipStreamDestroy(stream), "GraphSlice hipStreamDestroy failed", __FILE__, __LINE__);
    }
};

// The owner of a problem's slice, spelled as the reference's array of one per GPU: data_slices[0] (graph_slices[0]) is the slice,
// null until Make().  The slice's DeviceArray members free themselves when it goes, however far its build came.
template <typename DataSlice>
struct SliceHolder {
    DataSlice *slice = nullptr;
    SliceHolder() = default;
    SliceHolder(const SliceHolder &) = delete;
    SliceHolder &operator=(const SliceHolder &) = delete;
    ~SliceHolder() { delete slice; }
    DataSlice *operator[](int) const { return slice; }
    explicit operator bool() const { return slice != nullptr; }
    DataSlice *Make()
    {
        delete slice;
        slice = new DataSlice();
        return slice;
    }
};

template <typename _VertexId, typename _SizeT, typename _Value, bool _USE_DOUBLE_BUFFER = false>
struct ProblemBase {
    typedef _VertexId VertexId;
    typedef _SizeT SizeT;
    typedef _Value Value;
    static constexpr bool USE_DOUBLE_BUFFER = _USE_DOUBLE_BUFFER;

    int num_gpus = 1;
    SizeT nodes = 0;
    SizeT edges = 0;
    SliceHolder<GraphSlice<VertexId, SizeT, Value>> graph_slices;
    int malformed = 0;  // ValidateCsr found offsets or columns that are not a CSR of `nodes` vertices

    virtual ~ProblemBase() {}

    hipError_t MakeSlice()
    {
        hipError_t retval = hipSuccess;
        num_gpus = 1;  // one process per GPU; N-GPU runs partition above this class
        GraphSlice<VertexId, SizeT, Value> *gs = graph_slices.Make();  // (a second Init: the first slice goes with all it held)
        gs->nodes = nodes;
        gs->edges = edges;
        GR_CHECK(hipStreamCreateWithFlags(&gs->stream, hipStreamNonBlocking), "ProblemBase hipStreamCreate failed");
        return retval;
    }

    // Host CSR -> HBM (problem_base.cuh:226-342).  `load_edge_values` also uploads graph.edge_values.
    hipError_t Init(bool /*stream_from_host: mapped-host streaming is not offered, HBM holds the graph*/,
                    const Csr<VertexId, Value, SizeT> &graph, int /*_num_gpus*/ = 1, bool load_edge_values = false)
    {
        hipError_t retval = hipSuccess;
        nodes = graph.nodes;
        edges = graph.edges;
        if ((retval = MakeSlice())) return retval;
        GraphSlice<VertexId, SizeT, Value> *gs = graph_slices[0];
        const size_t ro_bytes = sizeof(SizeT) * (static_cast<size_t>(nodes) + 1);
        GR_CHECK(gs->own_row_offsets.Alloc(static_cast<size_t>(nodes) + 1), "ProblemBase d_row_offsets failed");
        GR_CHECK(gs->own_column_indices.Alloc(static_cast<size_t>(edges)), "ProblemBase d_column_indices failed");
        gs->d_row_offsets = gs->own_row_offsets;
        gs->d_column_indices = gs->own_column_indices;
        GR_CHECK(hipMemcpy(gs->d_row_offsets, graph.row_offsets, ro_bytes, hipMemcpyHostToDevice),
                 "ProblemBase hipMemcpy d_row_offsets failed");
        if (edges > 0)
            GR_CHECK(hipMemcpy(gs->d_column_indices, graph.column_indices, sizeof(VertexId) * static_cast<size_t>(edges),
                               hipMemcpyHostToDevice),
                     "ProblemBase hipMemcpy d_column_indices failed");
        if (load_edge_values && graph.edge_values) {
            GR_CHECK(gs->own_edge_values.Alloc(static_cast<size_t>(edges)), "ProblemBase d_edge_values failed");
            gs->d_edge_values = gs->own_edge_values;
            if (edges > 0)
                GR_CHECK(hipMemcpy(gs->d_edge_values, graph.edge_values, sizeof(Value) * static_cast<size_t>(edges),
                                   hipMemcpyHostToDevice),
                         "ProblemBase hipMemcpy d_edge_values failed");
        }
        return retval;
    }

    // CSR already resident in HBM (borrowed, not freed).
    hipError_t InitFromDevice(SizeT nodes_, SizeT edges_, SizeT *d_row_offsets, VertexId *d_column_indices,
                              Value *d_edge_values = nullptr)
    {
        hipError_t retval = hipSuccess;
        nodes = nodes_;
        edges = edges_;
        if ((retval = MakeSlice())) return retval;
        graph_slices[0]->d_row_offsets = d_row_offsets;
        graph_slices[0]->d_column_indices = d_column_indices;
        graph_slices[0]->d_edge_values = d_edge_values;
        return retval;
    }

    // The CSR must be one before a build indexes with what it reads: hipErrorInvalidValue, and `malformed` set, when it is not.
    // Without arguments the problem's own graph; with them another CSR of as many vertices and entries (a caller's transpose).
    hipError_t ValidateCsr(const SizeT *d_row_offsets, const VertexId *d_column_indices)
    {
        hipError_t retval = hipSuccess;
        DeviceArray<int> flag;
        bool bad = false;
        if ((retval = flag.Alloc(1))) return retval;
        if ((retval = graphio::DeviceValidateCsr(d_row_offsets, d_column_indices, nodes, edges, flag.p, graph_slices[0]->stream, &bad))) return retval;
        return bad ? Malformed() : retval;
    }
    hipError_t ValidateCsr() { return ValidateCsr(graph_slices[0]->d_row_offsets, graph_slices[0]->d_column_indices); }

    // what an Init returns when the input is not what the primitive takes
    hipError_t Malformed()
    {
        malformed = 1;
        return hipErrorInvalidValue;
    }

    // count elements of d_in to the host, and the stream drained; h_out may be NULL and count 0: then nothing happens
    template <typename T>
    hipError_t Read(T *h_out, const T *d_in, size_t count)
    {
        hipError_t retval = hipSuccess;
        hipStream_t stream = graph_slices[0]->stream;
        if (h_out && count) {
            GR_CHECK(hipMemcpyAsync(h_out, d_in, sizeof(T) * count, hipMemcpyDeviceToHost, stream), "ProblemBase read failed");
            GR_CHECK(hipStreamSynchronize(stream), "ProblemBase read sync failed");
        }
        return retval;
    }

    // (Re)size the ping-pong queues; memory is reused when large enough (problem_base.cuh:352-431).
    hipError_t Reset(FrontierType frontier_type, double queue_sizing)
    {
        hipError_t retval = hipSuccess;
        GraphSlice<VertexId, SizeT, Value> *gs = graph_slices[0];
        double base = 0;
        switch (frontier_type) {
            case VERTEX_FRONTIERS: base = nodes; break;
            case EDGE_FRONTIERS: base = edges > nodes ? edges : nodes; break;
            case MIXED_FRONTIERS: base = static_cast<double>(nodes) + edges; break;
        }
        double want = base * queue_sizing;
        if (want < 1024) want = 1024;
        if (want > 2147483000.0) want = 2147483000.0;
        const SizeT elements = static_cast<SizeT>(want);
        for (int i = 0; i < 2; ++i) {
            retval = gs->queue_storage[i].Grow(elements);
            gs->frontier_queues[i] = gs->queue_storage[i].view;  // (empty after a grow that failed)
            if (retval) return util::GRError(retval, "ProblemBase frontier queue failed", __FILE__, __LINE__);
        }
        return retval;
    }
};

// One device array of a problem's slice that grows with the largest need so far and keeps nothing when it does.
template <typename T>
struct Grown : util::DeviceArray<T> {
    size_t room = 0;
    hipError_t Need(size_t count)
    {
        hipError_t retval = hipSuccess;
        if (count <= room) return retval;
        room = 0;
        if ((retval = this->Alloc(count))) return retval;
        room = count;
        return retval;
    }
    // ... and is all 0 when it has grown: for scratch that every kernel leaves as it found it, cleared once
    hipError_t NeedZeroed(size_t count, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        if (count <= room) return retval;
        if ((retval = Need(count))) return retval;
        GR_CHECK(hipMemsetAsync(this->p, 0, sizeof(T) * count, stream), "grown array memset failed");
        return retval;
    }
    void Free()
    {
        util::DeviceArray<T>::Free();
        room = 0;
    }
};

}  // namespace app
}  // namespace gunrock
