// app/truss/truss_functor.hpp -- device kernels of per-edge triangle support and the k-truss decomposition.
//
// The reference snapshot has no app/truss (later Gunrock releases and the GraphChallenge do); the shape follows this tree's
// primitives.  G is the simple undirected graph of the CSR as MIS, TC and k-core read it.  Init (truss_problem.hpp) builds the
// canonical edge arrays src[e] < dst[e], sorted by (src, dst), and the symmetric neighbour CSR with rows ascending by id; beside
// every entry (v, u) sits the id of the edge {v, u}, so an intersection hands back the two other edges of every triangle it finds.
//
// Support: the triangle a < b < c is found once, from its edge (a, b), as a common entry c of the tails above b of N(a) and N(b)
// (rows ascend: a tail is a contiguous range).  The shorter tail is walked and looked up in the longer by bisection; the hits
// credit (a, b) with one store and (a, c), (b, c) with one atomic each.
//
// Peel: one array does the work.  val[e] starts as support[e] and ends as truss[e] - 2.  At level s = k - 2 the frontier F of a
// sub-round is the set of edges at or under s that have not left before; every e1 = (u, v) in F walks the shorter of N(u), N(v)
// and bisects the longer, and for every triangle {e1, e2, e3} whose other edges have not left in an earlier sub-round:
//   neither e2 nor e3 in F   each loses one
//   one of them in F         the other loses one when e1 has the smaller id of the two F edges (the triangle is charged once)
//   both in F                nothing (all three leave together)
// "Loses one" is k-core's returning atomic (kcore_functor.hpp): old == s + 1 appends the edge for the next sub-round (the one
// lane that saw s + 1), old <= s is put back, old > s + 1 leaves old - 1 as a candidate for the next level.
// The states are told apart by one stamp per edge: 0 while the edge is live, the number of the sub-round in which it is in F
// from the moment it is appended.  A sub-round `cur` reads stamp == cur as "in F", 0 < stamp < cur as "left earlier" and
// everything else (0, or cur + 1: appended during this sub-round) as alive and not in F.  A stamp is written once, by the lane
// that appends the edge, and the only value written during sub-round cur is cur + 1: both values a racing reader can see (0 and
// cur + 1) mean the same to it, so every schedule takes the same decisions.  Sub-rounds are numbered through the whole run.
//
// Rows: a lane per intersection whose shorter row has fewer than `wave_min_row` entries, the whole wave for the others; both loops
// are wave-uniform, so the appends of one step are one ballot and one atomic on the tail per wave.  A wave's tile of frontier edges
// is sized by the entries of their shorter rows (oprtr::TileFor), not by their number.
//
// Kernels: ScanKernel / PeelKernel are the wide forms, one launch per step, the host reading the words in between.  LoopKernel is
// one workgroup of 1024 that runs the same steps in a loop on the device (agent-scope accesses on everything a step hands to the
// next, a fence and a barrier between steps) and returns when the work at hand is too wide for one CU, when it is done, or after
// max_steps.
#pragma once

#include <hip/hip_runtime.h>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // (only a few of k-core's and TC's kernels are used here)
#include <gunrock/app/kcore/kcore_functor.hpp>
#include <gunrock/app/tc/tc_functor.hpp>
#pragma clang diagnostic pop
#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace truss {

enum { TRUSS_AUTO = 0, TRUSS_ROUNDS = 1 };

constexpr int kTrussThreads = 256;
constexpr int kWaveMinRow = 32;  // default "wave_min_row", not the shared 16

using kcore::kNoLevel;
using oprtr::kLoopMaxSteps;
using oprtr::kLoopThreads;
using oprtr::Ld;
using oprtr::St;
using oprtr::TileFor;
using tc::LowerBound;

// the words the kernels and the host share
enum {
    W_TAIL = 0,      // queue tail: edges appended so far
    W_LOW,           // smallest live value seen above the current level (UINT_MAX: none)
    W_ENTRIES,       // shorter-row entries of all the edges appended so far, modulo 2^32 (readers take differences)
    W_HEAD,          // LoopKernel's state on return: queue head,
    W_S,             //   current level,
    W_SPREV,         //   the level before it (an edge is live when val > sprev),
    W_STATUS,        //   why it returned,
    W_ROUND,         //   the number of the sub-round [head, tail) is or will be,
    W_SUBROUNDS,     // sub-rounds LoopKernel ran
    W_TRACE,         // trace entries written
    W_ENTRIES_SEEN,  // W_ENTRIES when the range [.., head) was fixed
    W_COUNT = 16
};
enum { LOOP_DONE = 0, LOOP_WIDE_PEEL = 1, LOOP_WIDE_SCAN = 2, LOOP_STEPS = 3, LOOP_LIMIT = 4 };

struct Graph {
    const int *ro;   // [nodes + 1] the symmetric simple neighbour CSR, rows ascending by id
    const int *ci;   // [2M]
    const int *eid;  // [2M] the edge of every entry
    const int *src;  // [M] the canonical edges, src < dst, sorted by (src, dst)
    const int *dst;
};

struct Trace {
    int *k;                     // one entry per level scan: the level (as k = s + 2),
    int *tail;                  // the queue tail when it began,
    unsigned long long *clock;  // the constant-rate counter then
};

struct Tally {
    unsigned low = kNoLevel;  // smallest live value seen above s
    unsigned entries = 0;     // shorter-row entries of the edges this lane appended
    unsigned reads = 0;       // row entries this lane walked
};

__device__ __forceinline__ void Flush(Tally &t, unsigned *d_words)
{
    unsigned low = t.low, entries = t.entries;
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const unsigned other = __shfl_xor(low, o, util::kWaveSize);
        low = other < low ? other : low;
        entries += __shfl_xor(entries, o, util::kWaveSize);
    }
    if (util::LaneId() == 0) {
        if (low != kNoLevel) atomicMin(d_words + W_LOW, low);
        if (entries) atomicAdd(d_words + W_ENTRIES, entries);
    }
    t.low = kNoLevel;
    t.entries = 0;
}

__device__ __forceinline__ void FlushReads(const Tally &t, unsigned long long *d_reads)
{
    const unsigned long long reads = util::WaveSum(static_cast<unsigned long long>(t.reads));
    if (util::LaneId() == 0 && reads) atomicAdd(d_reads, reads);
}

// the two rows of edge e: [sb, se) the shorter, [lb, le) the longer
__device__ __forceinline__ void RowsOf(const Graph &g, int e, int &sb, int &se, int &lb, int &le)
{
    const int u = g.src[e], v = g.dst[e];
    sb = g.ro[u];
    se = g.ro[u + 1];
    lb = g.ro[v];
    le = g.ro[v + 1];
    if (se - sb > le - lb) {
        int t = sb; sb = lb; lb = t;
        t = se; se = le; le = t;
    }
}

// All lanes of the wave call; the lanes with `hit` append e for sub-round `next`: one atomic on the tail per wave.  (An edge is
// appended once in a run, so the tail never passes M, the length of the queue.)
template <bool FRESH>
__device__ __forceinline__ void Append(const Graph &g, bool hit, int e, int next, int *d_stamp, int *d_queue, unsigned *d_words, Tally &t)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned pos = oprtr::WaveTicket(d_words + W_TAIL, mask);
    if (hit) {
        St<FRESH>(d_queue + pos, e);
        St<FRESH>(d_stamp + e, next);
        int sb, se, lb, le;
        RowsOf(g, e, sb, se, lb, le);
        t.entries += static_cast<unsigned>(se - sb);
    }
}

// edge e, alive and not in F (its stamp read as `stamp`: 0, or cur + 1 when it reached the level in this sub-round already),
// loses one; returns whether it reached the level through this lane
__device__ __forceinline__ bool LoseOne(int *d_val, int e, int stamp, int s, Tally &t)
{
    if (stamp != 0) return false;  // at the level already: the decrement would be put back
    const int old = atomicSub(d_val + e, 1);
    if (old == s + 1) return true;
    if (old <= s) atomicAdd(d_val + e, 1);
    else if (static_cast<unsigned>(old - 1) < t.low) t.low = static_cast<unsigned>(old - 1);
    return false;
}

// what a probe hands to the appends: the edges that reached the level through this lane, -1 for none
struct Hits {
    int e2, e3;
};

// entry i of the shorter row of the frontier edge e1, the longer row [lb, le): the triangle through it, if there is a live one
template <bool FRESH>
__device__ __forceinline__ Hits Probe(const Graph &g, int *d_val, const int *d_stamp, int e1, int i, int lb, int le, int s, int cur, Tally &t)
{
    Hits h = {-1, -1};
    ++t.reads;
    const int e2 = g.eid[i];
    if (e2 == e1) return h;  // (the entry of e1's other end)
    const int s2 = Ld<FRESH>(d_stamp + e2);
    if (s2 > 0 && s2 < cur) return h;  // left earlier: no look-up
    const int w = g.ci[i];
    const int at = LowerBound(g.ci, lb, le, w);
    if (at >= le || g.ci[at] != w) return h;
    const int e3 = g.eid[at];
    const int s3 = Ld<FRESH>(d_stamp + e3);
    if (s3 > 0 && s3 < cur) return h;
    const bool f2 = s2 == cur, f3 = s3 == cur;
    // both in F: nothing; one in F: the other loses one when e1 is the smaller of the two F edges; none: both lose one
    const bool take2 = !f2 && (f3 ? e1 < e3 : true), take3 = !f3 && (f2 ? e1 < e2 : true);
    if (take2 && LoseOne(d_val, e2, s2, s, t)) h.e2 = e2;
    if (take3 && LoseOne(d_val, e3, s3, s, t)) h.e3 = e3;
    return h;
}

// 64 queue entries by one wave: lane `lane` holds e1 (or -1).  Short intersections by their lane, the others by the wave.
template <bool FRESH>
__device__ __forceinline__ void PeelTile(const Graph &g, int *d_val, int *d_stamp, int *d_queue, unsigned *d_words, int e1, int s, int cur,
                                         int wave_min_row, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    int sb = 0, se = 0, lb = 0, le = 0;
    if (e1 >= 0) RowsOf(g, e1, sb, se, lb, le);
    const bool wide = se - sb >= wave_min_row && se > sb;
    int longest = wide ? 0 : se - sb;
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const int other = __shfl_xor(longest, o, util::kWaveSize);
        longest = other > longest ? other : longest;
    }
    for (int j = 0; j < longest; ++j) {  // (wave-uniform)
        Hits h = {-1, -1};
        if (!wide && sb + j < se) h = Probe<FRESH>(g, d_val, d_stamp, e1, sb + j, lb, le, s, cur, t);
        Append<FRESH>(g, h.e2 >= 0, h.e2, cur + 1, d_stamp, d_queue, d_words, t);
        Append<FRESH>(g, h.e3 >= 0, h.e3, cur + 1, d_stamp, d_queue, d_words, t);
    }
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const int wsb = __shfl(sb, leader, util::kWaveSize), wse = __shfl(se, leader, util::kWaveSize);
        const int wlb = __shfl(lb, leader, util::kWaveSize), wle = __shfl(le, leader, util::kWaveSize);
        const int we = __shfl(e1, leader, util::kWaveSize);
        for (int base = wsb; base < wse; base += util::kWaveSize) {  // (wave-uniform)
            Hits h = {-1, -1};
            if (base + lane < wse) h = Probe<FRESH>(g, d_val, d_stamp, we, base + lane, wlb, wle, s, cur, t);
            Append<FRESH>(g, h.e2 >= 0, h.e2, cur + 1, d_stamp, d_queue, d_words, t);
            Append<FRESH>(g, h.e3 >= 0, h.e3, cur + 1, d_stamp, d_queue, d_words, t);
        }
        todo &= todo - 1;
    }
}

// the sub-round [head, tail) of level s, numbered cur, by the waves wave0, wave0 + nwaves, ..., `tile` entries each at a time
template <bool FRESH>
__device__ __forceinline__ void PeelRange(const Graph &g, int *d_val, int *d_stamp, int *d_queue, unsigned *d_words, long long head, long long tail,
                                          int s, int cur, int wave_min_row, int tile, long long wave0, long long nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    for (long long base = head + wave0 * tile; base < tail; base += nwaves * tile) {  // (wave-uniform)
        const long long i = base + lane;
        const int e1 = lane < tile && i < tail ? Ld<FRESH>(d_queue + i) : -1;
        PeelTile<FRESH>(g, d_val, d_stamp, d_queue, d_words, e1, s, cur, wave_min_row, t);
    }
}

// the first sub-round of level s, numbered cur: the live edges (val > sprev) with val <= s; the others give the minimum
template <bool FRESH>
__device__ __forceinline__ void ScanRange(const Graph &g, const int *d_val, int *d_stamp, long long count, int sprev, int s, int cur, int *d_queue,
                                          unsigned *d_words, long long wave0, long long nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    for (long long base = wave0 * util::kWaveSize; base < count; base += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = base + lane;
        bool hit = false;
        if (i < count) {
            const int c = Ld<FRESH>(d_val + i);
            hit = c > sprev && c <= s;
            if (c > s && static_cast<unsigned>(c) < t.low) t.low = static_cast<unsigned>(c);
        }
        Append<FRESH>(g, hit, static_cast<int>(i), cur, d_stamp, d_queue, d_words, t);
    }
}

__device__ __forceinline__ void Stamp(const Trace &tr, unsigned *d_words, int s, unsigned tail)
{
    const unsigned at = atomicAdd(d_words + W_TRACE, 1u);  // (levels are distinct values in [0, max support]: the arrays hold them)
    tr.k[at] = s + 2;
    tr.tail[at] = static_cast<int>(tail);
    tr.clock[at] = wall_clock64();
}

// ---------------- the wide forms ----------------

static __global__ __launch_bounds__(kTrussThreads) void ScanKernel(Graph g, const int *d_val, int *d_stamp, long long count, int sprev, int s, int cur,
                                                                    int *d_queue, unsigned *d_words, Trace tr, unsigned tail)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    if (blockIdx.x == 0 && threadIdx.x == 0) Stamp(tr, d_words, s, tail);
    Tally t;
    ScanRange<false>(g, d_val, d_stamp, count, sprev, s, cur, d_queue, d_words, wave0, nwaves, t);
    Flush(t, d_words);
}

static __global__ __launch_bounds__(kTrussThreads) void PeelKernel(Graph g, int *d_val, int *d_stamp, int *d_queue, long long head, long long tail,
                                                                    int s, int cur, int wave_min_row, int tile, unsigned *d_words,
                                                                    unsigned long long *d_reads)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    PeelRange<false>(g, d_val, d_stamp, d_queue, d_words, head, tail, s, cur, wave_min_row, tile, wave0, nwaves, t);
    Flush(t, d_words);
    FlushReads(t, d_reads);
}

// ---------------- the device loop ----------------

struct LoopArgs {
    long long edges;        // M
    long long head;
    unsigned entries_seen;  // W_ENTRIES when `head` was fixed
    int s, sprev;
    int s_limit;            // levels at or above it are not peeled (INT_MAX: none)
    int round;              // the number of the sub-round [head, tail) is (level open) or the next scan opens
    int level_open;         // the scan of level s has run: [head, tail) is a sub-round of it
    int wave_min_row;
    long long max_list;     // return to the host for a scan of more edges, ...
    long long max_entries;  // ... and for a sub-round with more shorter-row entries
    int max_steps;
};

// One workgroup.  Every step ends in a barrier behind a fence; the words and everything a step leaves for the next are read with
// agent-scope loads.  Uniform control flow: every decision is taken on values all threads read after the same barrier.
static __global__ __launch_bounds__(kLoopThreads) void LoopKernel(Graph g, int *d_val, int *d_stamp, int *d_queue, unsigned *d_words,
                                                                   unsigned long long *d_reads, Trace tr, LoopArgs a)
{
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    const int *w = reinterpret_cast<const int *>(d_words);
    long long head = a.head;
    int s = a.s, sprev = a.sprev, cur = a.round, status = LOOP_STEPS;
    bool open = a.level_open != 0;
    unsigned subrounds = 0, entries_seen = a.entries_seen;
    Tally t;
    for (int step = 0; step < a.max_steps; ++step) {
        const long long tail = static_cast<unsigned>(Ld<true>(w + W_TAIL));
        if (open && head < tail) {  // a sub-round of level s
            const unsigned entries = static_cast<unsigned>(Ld<true>(w + W_ENTRIES));
            if (entries - entries_seen > a.max_entries) { status = LOOP_WIDE_PEEL; break; }
            __syncthreads();  // (everybody has read the words)
            PeelRange<true>(g, d_val, d_stamp, d_queue, d_words, head, tail, s, cur, a.wave_min_row, TileFor(tail - head, nwaves, entries - entries_seen),
                            wave0, nwaves, t);
            Flush(t, d_words);
            head = tail;
            entries_seen = entries;
            ++cur;
            ++subrounds;
            __threadfence();
            __syncthreads();
            continue;
        }
        if (open) {  // level s has run dry: the next one is the smallest live value
            const unsigned low = static_cast<unsigned>(Ld<true>(w + W_LOW));
            sprev = s;
            open = false;
            if (low == kNoLevel || a.edges - tail <= 0) { status = LOOP_DONE; break; }
            s = static_cast<int>(low);
        }
        if (s >= a.s_limit) { status = LOOP_LIMIT; break; }
        if (a.edges > a.max_list) { status = LOOP_WIDE_SCAN; break; }
        __syncthreads();
        if (threadIdx.x == 0) {
            St<true>(reinterpret_cast<int *>(d_words) + W_LOW, static_cast<int>(kNoLevel));
            Stamp(tr, d_words, s, static_cast<unsigned>(tail));
        }
        __threadfence();
        __syncthreads();
        ScanRange<true>(g, d_val, d_stamp, a.edges, sprev, s, cur, d_queue, d_words, wave0, nwaves, t);
        Flush(t, d_words);
        open = true;
        __threadfence();
        __syncthreads();
    }
    FlushReads(t, d_reads);
    __syncthreads();
    if (threadIdx.x == 0) {
        int *out = reinterpret_cast<int *>(d_words);
        out[W_ENTRIES_SEEN] = static_cast<int>(entries_seen);
        out[W_HEAD] = static_cast<int>(head);
        out[W_S] = s;
        out[W_SPREV] = sprev;
        out[W_STATUS] = status | (open ? 0x100 : 0);
        out[W_ROUND] = cur;
        out[W_SUBROUNDS] += static_cast<int>(subrounds);
    }
}

// ---------------- the support pass ----------------

// entry i of the shorter tail of edge e = (a, b): c = ci[i] > b, looked up in the longer tail [lb, le)
__device__ __forceinline__ unsigned SupportProbe(const Graph &g, int i, int lb, int le, int *d_support)
{
    const int c = g.ci[i];
    const int at = LowerBound(g.ci, lb, le, c);
    if (at >= le || g.ci[at] != c) return 0;
    atomicAdd(d_support + g.eid[i], 1);
    atomicAdd(d_support + g.eid[at], 1);
    return 1;
}

// support[e] += the triangles {a, b, c} with a < b < c of every edge e = (a, b); the edges (a, c) and (b, c) are credited by
// atomics, so d_support is zeroed before.  d_reads += the tail entries walked.
static __global__ __launch_bounds__(kTrussThreads) void SupportKernel(Graph g, long long edges, int wave_min_row, int *d_support,
                                                                       unsigned long long *d_reads)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    unsigned long long reads = 0;
    for (long long base = wave0 * util::kWaveSize; base < edges; base += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long e = base + lane;
        int sb = 0, se = 0, lb = 0, le = 0;
        if (e < edges) {
            const int a = g.src[e], b = g.dst[e];
            // the tails above b: in N(b) behind the entries below b (a among them); in N(a) behind the entry b itself
            se = g.ro[a + 1];
            sb = LowerBound(g.ci, g.ro[a], se, b + 1);
            le = g.ro[b + 1];
            lb = LowerBound(g.ci, g.ro[b], le, b + 1);
            if (se - sb > le - lb) {
                int t = sb; sb = lb; lb = t;
                t = se; se = le; le = t;
            }
            if (le == lb) se = sb;  // nothing to find
        }
        const bool wide = se - sb >= wave_min_row && se > sb;
        unsigned c = 0;
        if (!wide) {
            for (int i = sb; i < se; ++i) c += SupportProbe(g, i, lb, le, d_support);
            reads += static_cast<unsigned long long>(se - sb);
            if (c) atomicAdd(d_support + e, static_cast<int>(c));
        }
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int wsb = __shfl(sb, leader, util::kWaveSize), wse = __shfl(se, leader, util::kWaveSize);
            const int wlb = __shfl(lb, leader, util::kWaveSize), wle = __shfl(le, leader, util::kWaveSize);
            unsigned wc = 0;
            for (int i = wsb + lane; i < wse; i += util::kWaveSize) wc += SupportProbe(g, i, wlb, wle, d_support);
            wc = util::WaveSum(wc);
            if (lane == 0) {
                reads += static_cast<unsigned long long>(wse - wsb);
                if (wc) atomicAdd(d_support + base + leader, static_cast<int>(wc));
            }
            todo &= todo - 1;
        }
    }
    reads = util::WaveSum(reads);
    if (lane == 0 && reads) atomicAdd(d_reads, reads);
}

// ---------------- around the peel ----------------

// d_out[0] = the largest value, d_out[1] = the smallest (UINT_MAX: no edges); d_sum += the values
static __global__ void SupportSummaryKernel(const int *d_values, long long count, unsigned *d_out, unsigned long long *d_sum)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned most = 0, least = kNoLevel;
    unsigned long long sum = 0;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < count; e += stride) {
        const unsigned d = static_cast<unsigned>(d_values[e]);
        most = d > most ? d : most;
        least = d < least ? d : least;
        sum += d;
    }
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const unsigned m = __shfl_xor(most, o, util::kWaveSize), l = __shfl_xor(least, o, util::kWaveSize);
        most = m > most ? m : most;
        least = l < least ? l : least;
        sum += __shfl_xor(sum, o, util::kWaveSize);
    }
    if (util::LaneId() == 0) {
        atomicMax(d_out, most);
        atomicMin(d_out + 1, least);
        if (sum) atomicAdd(d_sum, sum);
    }
}

// truss[e] = min(val[e], cap) + 2 (cap: the level a limited run stopped at, minus 2; what is live there has at least that)
static __global__ void FinishKernel(const int *d_val, long long count, int cap, int *d_truss)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < count; e += stride) {
        const int v = d_val[e];
        d_truss[e] = (v < cap ? v : cap) + 2;
    }
}

// mask[e] = truss[e] >= k; d_out[0] += such edges; their ends are flagged
static __global__ void MemberEdgesKernel(Graph g, const int *d_truss, long long count, int k, unsigned char *d_mask, int *d_flag,
                                         unsigned long long *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned long long members = 0;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < count; e += stride) {
        const bool in = d_truss[e] >= k;
        d_mask[e] = in ? 1 : 0;
        if (in) {
            ++members;
            d_flag[g.src[e]] = 1;  // (every writer writes 1)
            d_flag[g.dst[e]] = 1;
        }
    }
    members = util::WaveSum(members);
    if (util::LaneId() == 0 && members) atomicAdd(d_out, members);
}

static __global__ void CountFlagsKernel(const int *d_flag, long long nodes, unsigned long long *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned long long members = 0;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) members += d_flag[v] != 0;
    members = util::WaveSum(members);
    if (util::LaneId() == 0 && members) atomicAdd(d_out, members);
}

// vertex_truss[v] = the largest truss over the edges at v (zeroed before)
static __global__ void VertexTrussKernel(Graph g, const int *d_truss, long long count, int *d_vertex)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < count; e += stride) {
        const int t = d_truss[e], a = g.src[e], b = g.dst[e];
        if (d_vertex[a] < t) atomicMax(d_vertex + a, t);  // (a stale read is only ever low: it costs an atomic)
        if (d_vertex[b] < t) atomicMax(d_vertex + b, t);
    }
}

}  // namespace truss
}  // namespace app
}  // namespace gunrock
