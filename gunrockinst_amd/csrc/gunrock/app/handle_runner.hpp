// app/handle_runner.hpp -- host-side pieces shared by the handle C ABI (lib/*_app.hip: the grx_<primitive>_* calls).
//
// Every primitive's runner times its Enact between two HIP events, borrows the caller's host CSR for Init, tracks whether
// an init succeeded, copies a per-round trace out and comes in an instrumented and a plain build.  Those blocks live here
// once; what differs per family -- argument rules, signatures, which phases are guarded -- stays in its *_app.hip.  The
// pieces are independent: a runner uses the ones it needs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>

#include <gunrock/csr.hpp>
#include <gunrock/util/error_utils.hpp>

namespace gunrock {
namespace app {

// The ABI's own init codes next to -1, a bad argument (a positive value is a hipError_t).
constexpr int kMalformedGraph = -2;  // Init found offsets or columns that are not a CSR of `nodes` vertices
constexpr int kHandleTaken = -3;     // the handle already took a graph

// The two events a runner times with.  Create() is separate from construction so that a runner calls it after it has
// selected its device.
class EventPair {
    hipEvent_t start = nullptr, stop = nullptr;

   public:
    EventPair() {}
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair()
    {
        if (start) hipEventDestroy(start);
        if (stop) hipEventDestroy(stop);
    }
    void Create()
    {
        util::GRError(hipEventCreate(&start), "hipEventCreate failed", __FILE__, __LINE__);
        util::GRError(hipEventCreate(&stop), "hipEventCreate failed", __FILE__, __LINE__);
    }
    // Device time of run() on `stream` into *ms (when given).  Returns what run() returned, or the error of a failed
    // event call.
    template <typename Run>
    hipError_t Timed(hipStream_t stream, float *ms, Run run)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(hipEventRecord(start, stream), "hipEventRecord failed");
        const hipError_t result = run();
        GR_CHECK(hipEventRecord(stop, stream), "hipEventRecord failed");
        GR_CHECK(hipEventSynchronize(stop), "hipEventSynchronize failed");
        float t = 0;
        GR_CHECK(hipEventElapsedTime(&t, start, stop), "hipEventElapsedTime failed");
        if (ms) *ms = t;
        return result;
    }
    // The same for a run(stop_event) that records the stop event itself, behind the last kernel it queues (recording it again
    // when it queues more: the later record wins), and returns only when the event has completed.  It is neither recorded
    // nor waited for again here (an event that has not completed makes hipEventElapsedTime fail): a run whose last kernel is
    // still executing when it knows its result spares the host calls behind that kernel.
    template <typename Run>
    hipError_t TimedLent(hipStream_t stream, float *ms, Run run)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(hipEventRecord(start, stream), "hipEventRecord failed");
        const hipError_t result = run(stop);
        float t = 0;
        GR_CHECK(hipEventElapsedTime(&t, start, stop), "hipEventElapsedTime failed");
        if (ms) *ms = t;
        return result;
    }
};

// A host Csr over arrays the caller owns (reference bfs_app.cu:256-260).  ~Csr() frees its arrays, so the pointers are
// taken back here, on every path out of the scope (bfs_app.cu:350-351 does it by hand).
template <typename Value = int>
struct BorrowedCsr {
    Csr<int, Value, int> graph;
    BorrowedCsr(int nodes, int edges, const int *row_offsets, const int *col_indices, const Value *edge_values = nullptr) : graph(false)
    {
        graph.nodes = nodes;
        graph.edges = edges;
        graph.row_offsets = const_cast<int *>(row_offsets);
        graph.column_indices = const_cast<int *>(col_indices);
        graph.edge_values = const_cast<Value *>(edge_values);
    }
    BorrowedCsr(const BorrowedCsr &) = delete;
    BorrowedCsr &operator=(const BorrowedCsr &) = delete;
    ~BorrowedCsr()
    {
        graph.row_offsets = nullptr;
        graph.column_indices = nullptr;
        graph.edge_values = nullptr;
    }
};

// What a handle knows about its init.
struct InitState {
    bool ready = false;  // an init succeeded: the other phases may run
    bool used = false;   // an init was called: a handle of a one-graph family takes no second one
    hipError_t Admit(hipError_t rc)
    {
        used = true;
        ready = rc == hipSuccess;
        return rc;
    }
    // Admits `rc` and gives the ABI's code for it; `malformed` is the problem's flag, read after its init returned.
    int AdmitCode(hipError_t rc, bool malformed) { return Admit(rc) != hipSuccess && malformed ? kMalformedGraph : static_cast<int>(rc); }
    // One-graph families refuse a second init: `if (int taken = state.Taken()) return taken;`
    int Taken() const { return used ? kHandleTaken : 0; }
};

// One output array of a trace and where entry i comes from.
template <typename Out, typename Get>
struct TraceColumn {
    Out *out;
    Get get;
};
template <typename Out, typename Get>
TraceColumn<Out, Get> Column(Out *out, Get get)
{
    return {out, get};
}
// Copies the first min(size, max) entries of a trace into its columns' arrays, skipping null ones; returns `size`, so a
// caller can ask with max = 0 how much to allocate.
template <typename... Out, typename... Get>
int CopyTrace(size_t size, int max, TraceColumn<Out, Get>... columns)
{
    const int count = static_cast<int>(size);
    for (int i = 0; i < count && i < max; ++i) ((columns.out ? void(columns.out[i] = columns.get(i)) : void()), ...);
    return count;
}

// The INSTR = true / false pair of a family's runner template behind its abstract base.
template <typename Base, template <bool> class Impl>
std::unique_ptr<Base> MakeRunner(bool instrument, int device)
{
    if (instrument) return std::unique_ptr<Base>(new Impl<true>(device));
    return std::unique_ptr<Base>(new Impl<false>(device));
}

}  // namespace app
}  // namespace gunrock
