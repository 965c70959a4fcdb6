// frontier.hpp -- device frontier queues and the work-progress counters that go with them.
//
// MI355X-first redesign of the reference's ping-pong frontier queues
// (gunrock/app/problem_base.cuh:73-140 GraphSlice::frontier_queues, util/multiple_buffering.cuh:92-131)
// and of CtaWorkProgress (gunrock/util/cta_work_progress.cuh:51-360):
//
//  * A frontier is three parallel arrays: vertex id, the vertex's first edge (row start) and the
//    EXCLUSIVE prefix sum of degrees in queue order.  The prefix is produced by whoever WRITES the
//    frontier (FrontierWriter in oprtr/frontier_writer.hpp) from one packed 64-bit reservation per
//    flushed batch, so the load-balanced advance needs no separate degree-gather, device-wide scan or
//    sorted-search pass per BFS level (reference: GetEdgeCounts + mgpu::Scan + MarkPartitionSizes +
//    mgpu::SortedSearch, oprtr/advance/kernel.cuh:300-368) and no blocking 4-byte length read inside
//    the operator (advance/kernel.cuh:315-317).
//  * One packed counter per BSP step: low 32 bits = queued vertices, high 32 bits = queued edges.
//    Counters form a ring of 4 like the reference's queue-length slots; the kernel of step k writes
//    slot (k+1)&3 and clears slot (k+2)&3 (cta_work_progress.cuh:55-72 protocol).
#pragma once

#include <hip/hip_runtime.h>
#include <set>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include <gunrock/util/device_array.hpp>
#include <gunrock/util/error_utils.hpp>

namespace gunrock {
namespace util {

template <typename VertexId, typename SizeT>
struct Frontier {
    VertexId *v = nullptr;   // vertex ids
    SizeT *row_start = nullptr;  // first edge of each vertex (offset into column_indices)
    SizeT *scan = nullptr;   // exclusive prefix sum of degrees, in queue order
    SizeT capacity = 0;
};
static_assert(std::is_trivially_copyable<Frontier<int, int>>::value,
              "a Frontier is a kernel argument: a view of raw pointers; its owner is app::FrontierStorage (app/problem_base.hpp)");

__host__ __device__ __forceinline__ unsigned long long PackTail(unsigned count, unsigned edges)
{
    return (static_cast<unsigned long long>(edges) << 32) | count;
}
__host__ __device__ __forceinline__ unsigned TailCount(unsigned long long t) { return static_cast<unsigned>(t); }
__host__ __device__ __forceinline__ unsigned TailEdges(unsigned long long t) { return static_cast<unsigned>(t >> 32); }

// Host wait for the stream: spin on hipStreamQuery instead of hipStreamSynchronize.  The BSP loop waits dozens of times
// per search for kernels that run 10-100 us; a blocking wait adds wake-up latency to each of them.
inline hipError_t SpinSync(hipStream_t stream)
{
    hipError_t rc;
    while ((rc = hipStreamQuery(stream)) == hipErrorNotReady) {
    }
    return rc;
}

// The calling workgroup's line of a "wide" tail (see WorkProgress::d_wide); nullptr stays nullptr.
__device__ __forceinline__ unsigned long long *WideTailSlot(unsigned long long *d_wide)
{
    return d_wide ? d_wide + (blockIdx.x & 31u) * 16u : nullptr;
}

// Pinned, device-mapped host block the PublishKernel writes straight into (no copy engine, no blit kernel per word).
struct HostMailbox {
    unsigned long long seq;       // written last, system-scope release
    unsigned long long tail[8];   // WorkProgress::d_tail
    unsigned long long sums[2];   // WorkProgress::d_sums
    unsigned long long wide;      // packed sum of the wide tail lines (which the kernel clears again)
    unsigned long long overflow;  // *d_overflow
    unsigned long long set_value; // staging word of WorkProgress::SetTail (host -> device)
    unsigned long long wide_set[8];  // packed sums of the further wide-counter sets (chained bottom-up sweeps; [0] unused: `wide`)
    int chain_log[8];             // action each sweep of the last chain took (oprtr/advance/bottom_up.hpp SweepAction)
};

// What one publication needs.  A kernel that publishes on behalf of PublishKernel (the BFS label pass, bfs_problem.hpp)
// takes one of these by value and only reads it; box == nullptr means "do not publish".
struct PublishArgs {
    unsigned long long *d_tail = nullptr;
    const unsigned long long *d_sums = nullptr;
    unsigned long long *d_wide = nullptr;
    const int *d_overflow = nullptr;
    HostMailbox *box = nullptr;
    unsigned long long seq = 0;
    // clear_mask / ones_mask: slots to zero / to set to all ones AFTER mirroring -- the re-arming an enactor
    // would otherwise do with one hipMemsetAsync per word before its next kernel
    unsigned clear_mask = 0, ones_mask = 0;
    int wide_sets = 1;
    const int *d_chain_log = nullptr;
};

// One wave (every lane of it, and no other wave of the grid): mirror the enactor's device words into the mailbox, fold +
// re-arm the wide tail, then publish `seq`.  Every word it reads must be final before the calling kernel starts.
__device__ __forceinline__ void PublishBody(const PublishArgs &a)
{
    const unsigned lane = threadIdx.x & 63u;
    HostMailbox *box = a.box;
    if (lane < 8) {
        const unsigned long long v = a.d_tail[lane];
        box->tail[lane] = v;
        if (lane == 7 || ((a.clear_mask >> lane) & 1u)) a.d_tail[lane] = 0ull;  // slot 7: grid barrier of the persistent levels kernel
        else if ((a.ones_mask >> lane) & 1u) a.d_tail[lane] = ~0ull;
    }
    if (lane < 2) box->sums[lane] = a.d_sums[lane];
    unsigned long long w = 0;
    if (lane < 32) {
        w = a.d_wide[lane * 16];
        if (w) a.d_wide[lane * 16] = 0;
    }
    for (int o = 16; o; o >>= 1) w += __shfl_xor(w, o, 64);  // packed halves add independently (counts stay below 2^32)
    if (lane == 0) {
        box->wide = w;
        box->overflow = static_cast<unsigned long long>(*a.d_overflow);
    }
    if (a.wide_sets > 1) {  // (uniform) the sets of a sweep chain: all loads first, then fold, mirror and re-arm each
        unsigned long long ws[7];
#pragma unroll
        for (int k = 1; k < 8; ++k) ws[k - 1] = (k < a.wide_sets && lane < 32) ? a.d_wide[k * 512 + lane * 16] : 0ull;
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            if (k < a.wide_sets) {
                if (ws[k - 1]) a.d_wide[k * 512 + lane * 16] = 0ull;
                unsigned long long t = ws[k - 1];
                for (int o = 16; o; o >>= 1) t += __shfl_xor(t, o, 64);
                if (lane == 0) box->wide_set[k] = t;
            }
        }
        if (lane < 8) box->chain_log[lane] = a.d_chain_log[lane];
    }
    __threadfence_system();  // (one wave: the fence covers the stores of all its lanes)
    if (lane == 0) __hip_atomic_store(&box->seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The publication as a kernel of its own: one workgroup of one wave.
static __global__ void PublishKernel(PublishArgs args) { PublishBody(args); }

// One wave: what WorkProgress::Reset + SetTail do with three fill blits and one copy blit (4-5 us each, serialised at the
// start of every Enact) -- zero the ring, the overflow flag and the wide tail, then seed one ring slot.
static __global__ void ArmKernel(unsigned long long *d_tail, int *d_overflow, unsigned long long *d_wide, int slots, int wide_lines,
                                 int wide_stride, int seed_slot, unsigned long long seed_value, int wide_sets)
{
    const int lane = threadIdx.x;
    if (lane < slots) d_tail[lane] = (lane == seed_slot) ? seed_value : 0ull;
    if (lane < wide_lines)
        for (int k = 0; k < wide_sets; ++k) d_wide[(k * wide_lines + lane) * wide_stride] = 0ull;
    if (lane == 0) *d_overflow = 0;
}

// Device words shared by all kernels of one enactor.  The struct stays on the host (kernels take its words one by one, or a
// PublishArgs), so it owns them.
struct WorkProgress {
    static constexpr int kSlots = 8;       // 0..3: BSP ring, 4: auxiliary tail, 5: SSSP far-min, 6: tail-kernel level count,
                                           // 7: grid barrier (counter | timeout); tail-kernel sums live in d_sums[2]
    static constexpr int kAux = 4;
    DeviceArray<unsigned long long> d_tail;  // [kSlots] packed (edges<<32 | vertices)
    DeviceArray<int> d_overflow;             // set when a writer ran out of queue capacity
    DeviceArray<unsigned long long> d_sums;  // [2] tail kernel: summed frontier lengths / edges
    // "Wide" tail: kWideLines packed counters, 128 bytes apart.  Atomics on ONE address retire at ~80 per microsecond on
    // MI355X (measured: 8192 wave-level adds = 103 us, tools/xcd_store_bench.hip), so kernels whose every workgroup reports
    // a count (bottom-up sweep, fresh-flag pass) spread their adds over these lines; PublishKernel folds and clears them.
    static constexpr int kWideLines = 32;
    static constexpr int kWideStride = 16;  // in 8-byte words
    // kWideSets such sets back to back: set 0 is "the" wide tail; sets 1.. take the finds of the sweeps of a chain (bottom_up.hpp)
    static constexpr int kWideSets = 8;
    static constexpr int kWideSetWords = kWideLines * kWideStride;
    DeviceArray<unsigned long long> d_wide;
    DeviceArray<int> d_chain_log;          // [8] action each sweep of a chain took; [8], [9]: gate words of the kernels queued behind
                                           // a chain (did the closing levels run; how many sweeps ran)
    int publish_sets = 1;                  // wide sets PublishKernel folds (enactors that chain sweeps raise it)
    // Host view.  Every blocking read-back of a BSP step is ONE tiny kernel that writes the mailbox in pinned host memory and
    // a host spin on its sequence word: the previous form (one or two hipMemcpyAsync = blit kernels of 4-5 us each, then a
    // stream query loop) cost ~20 us per level.
    PinnedArray<HostMailbox, hipHostMallocMapped> box;  // pinned + mapped
    unsigned long long *h_sums = nullptr;  // = box->sums
    unsigned long long *h_tail = nullptr;  // = box->tail
    unsigned long long seq = 0;

    // WorkProgress objects whose device words exist.  A problem that arms an enactor's words from its own Reset kernel
    // (BFSProblem) keeps a pointer to them across searches; it asks here whether the enactor is still alive before using it.
    static std::set<const WorkProgress *> &Live()
    {
        static std::set<const WorkProgress *> *live = new std::set<const WorkProgress *>();  // (never destroyed: an enactor may be
                                                                                             //  released during static destruction)
        return *live;
    }
    static bool IsLive(const WorkProgress *p) { return p && Live().count(p) != 0; }

    hipError_t Init()
    {
        hipError_t retval = hipSuccess;
        if (d_tail) return retval;
        Live().insert(this);
        GR_CHECK(d_tail.Alloc(kSlots), "WorkProgress d_tail failed");
        GR_CHECK(d_overflow.Alloc(1), "WorkProgress d_overflow failed");
        GR_CHECK(box.Alloc(1), "WorkProgress mailbox failed");
        std::memset(box.p, 0, sizeof(HostMailbox));
        h_tail = box->tail;
        h_sums = box->sums;
        GR_CHECK(d_sums.Alloc(2), "WorkProgress d_sums failed");
        GR_CHECK(hipMemset(d_sums, 0, sizeof(unsigned long long) * 2), "WorkProgress memset failed");
        GR_CHECK(d_wide.Alloc(kWideSets * kWideSetWords), "WorkProgress d_wide failed");
        GR_CHECK(d_chain_log.Alloc(16), "WorkProgress d_chain_log failed");
        GR_CHECK(hipMemset(d_chain_log, 0, sizeof(int) * 16), "WorkProgress memset failed");
        // Blocking clears: the enactors work on non-blocking streams, which are NOT ordered behind the null stream -- an
        // asynchronous clear issued here could land after the first search's seed (seen: a search that found nothing).
        GR_CHECK(hipMemset(d_tail, 0, sizeof(unsigned long long) * kSlots), "WorkProgress memset failed");
        GR_CHECK(hipMemset(d_overflow, 0, sizeof(int)), "WorkProgress memset failed");
        GR_CHECK(hipMemset(d_wide, 0, sizeof(unsigned long long) * kWideSets * kWideSetWords), "WorkProgress memset failed");
        GR_CHECK(hipDeviceSynchronize(), "WorkProgress init sync failed");
        return retval;
    }

    hipError_t Reset(hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(hipMemsetAsync(d_tail, 0, sizeof(unsigned long long) * kSlots, stream), "WorkProgress memset failed");
        GR_CHECK(hipMemsetAsync(d_overflow, 0, sizeof(int), stream), "WorkProgress memset failed");
        GR_CHECK(hipMemsetAsync(d_wide, 0, sizeof(unsigned long long) * kWideSets * kWideSetWords, stream),
                 "WorkProgress memset failed");
        return retval;
    }

    // Reset + SetTail(slot, count, edges) in one launch
    hipError_t ResetWithTail(int slot, unsigned count, unsigned edges, hipStream_t stream)
    {
        box->overflow = 0;  // (a new search starts: forget the last search's flag)
        hipLaunchKernelGGL(ArmKernel, dim3(1), dim3(64), 0, stream, d_tail, d_overflow, d_wide, kSlots, kWideLines, kWideStride, slot & 3,
                           PackTail(count, edges), kWideSets);
        return GRError(hipGetLastError(), "WorkProgress ArmKernel launch failed", __FILE__, __LINE__);
    }

    hipError_t SetTail(int slot, unsigned count, unsigned edges, hipStream_t stream)
    {
        box->set_value = PackTail(count, edges);
        box->overflow = 0;  // (a new search starts: forget the last search's flag)
        return GRError(hipMemcpyAsync(d_tail + (slot & 3), &box->set_value, sizeof(unsigned long long), hipMemcpyHostToDevice, stream),
                       "WorkProgress SetTail failed", __FILE__, __LINE__);
    }

    // A read-back in two steps.  Post: the next sequence number and the publication that will write it -- PublishKernel on
    // `stream`, or, with `hand_over`, the filled arguments for a kernel the caller queues next and which publishes on its
    // behalf (every word mirrored must be final before that kernel starts).
    hipError_t Post(hipStream_t stream, unsigned clear_mask = 0, unsigned ones_mask = 0, PublishArgs *hand_over = nullptr)
    {
        PublishArgs a;
        a.d_tail = d_tail;
        a.d_sums = d_sums;
        a.d_wide = d_wide;
        a.d_overflow = d_overflow;
        a.box = box;
        a.seq = ++seq;
        a.clear_mask = clear_mask;
        a.ones_mask = ones_mask;
        a.wide_sets = publish_sets;
        a.d_chain_log = d_chain_log;
        if (hand_over) {
            *hand_over = a;
            return hipSuccess;
        }
        hipLaunchKernelGGL(PublishKernel, dim3(1), dim3(64), 0, stream, a);
        return GRError(hipGetLastError(), "WorkProgress PublishKernel launch failed", __FILE__, __LINE__);
    }

    // Wait: host spin on the sequence word of the last Post.
    hipError_t Wait(hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        volatile unsigned long long *flag = &box->seq;
        unsigned spins = 0;
        while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
            if ((++spins & 0x3FFu) == 0) {  // now and then: did the stream fail, or finish without us seeing the flag yet?
                hipError_t rc = hipStreamQuery(stream);
                if (rc == hipSuccess) {
                    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) break;
                    continue;
                }
                if (rc != hipErrorNotReady) return GRError(rc, "WorkProgress Sync: stream failed", __FILE__, __LINE__);
            }
        }
        return retval;
    }

    // Mirror all device words into the mailbox and wait for them (the only host<->device sync of a BSP step).
    hipError_t Sync(hipStream_t stream, unsigned clear_mask = 0, unsigned ones_mask = 0)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(Post(stream, clear_mask, ones_mask), "WorkProgress Post failed");
        return Wait(stream);
    }

    // Blocking read of one slot.
    hipError_t GetTail(int slot, unsigned &count, unsigned &edges, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(Sync(stream), "WorkProgress GetTail sync failed");
        count = TailCount(h_tail[slot & 3]);
        edges = TailEdges(h_tail[slot & 3]);
        return retval;
    }

    // Blocking read of one ring slot plus the wide counters; (count, edges) = their sum.
    hipError_t GetTailWide(int slot, unsigned &count, unsigned &edges, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(Sync(stream), "WorkProgress GetTailWide sync failed");
        count = TailCount(h_tail[slot & 3]) + TailCount(box->wide);
        edges = TailEdges(h_tail[slot & 3]) + TailEdges(box->wide);
        return retval;
    }

    // One blocking read of the whole ring + the tail kernel's outputs.
    hipError_t GetAll(hipStream_t stream) { return Sync(stream); }

    // slot 7: grid-barrier counter (low word) and its timeout flag (high word) of the persistent levels kernel
    unsigned *BarrierCounter() { return reinterpret_cast<unsigned *>(d_tail + 7); }
    int *BarrierTimeout() { return reinterpret_cast<int *>(d_tail + 7) + 1; }
    bool HostBarrierTimedOut() const { return (h_tail[7] >> 32) != 0; }
    int *LevelsDone() { return reinterpret_cast<int *>(d_tail + 6); }
    int HostLevelsDone() const { return *reinterpret_cast<const int *>(h_tail + 6); }

    unsigned long long *AuxTail() { return d_tail + kAux; }
    hipError_t ClearAux(hipStream_t stream)
    {
        return GRError(hipMemsetAsync(d_tail + kAux, 0, sizeof(unsigned long long), stream),
                       "WorkProgress ClearAux failed", __FILE__, __LINE__);
    }
    hipError_t GetAux(unsigned &count, unsigned &edges, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(Sync(stream), "WorkProgress GetAux sync failed");
        count = TailCount(h_tail[kAux]);
        edges = TailEdges(h_tail[kAux]);
        return retval;
    }

    // Overflow flag as of the last read-back.  Every enactor loop ends on a read-back that follows its last kernel; the only
    // kernel that may run behind the last read-back is the BFS label pass that carried it (PublishBody), and that pass writes
    // labels only: it cannot overflow anything.
    bool OverflowAtLastSync() const { return box->overflow != 0; }

    hipError_t CheckOverflow(bool &overflow, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(Sync(stream), "WorkProgress CheckOverflow sync failed");
        overflow = OverflowAtLastSync();
        return retval;
    }

    ~WorkProgress() { Live().erase(this); }  // (the words free themselves)
};

}  // namespace util
}  // namespace gunrock
