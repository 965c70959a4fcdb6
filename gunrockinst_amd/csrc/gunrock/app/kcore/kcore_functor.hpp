// app/kcore/kcore_functor.hpp -- device kernels of the k-core decomposition (core numbers by peeling).
//
// The reference snapshot has no app/kcore (later Gunrock releases do); the shape follows this tree's primitives.  G is the simple
// undirected graph of the CSR as MIS and TC read it; Init (kcore_problem.hpp) builds its symmetric neighbour CSR and d(v).
//
// One array does the work: core[v] starts as d(v) and ends as the core number.  At level k a vertex with core[v] = k is peeled:
// it walks its row and takes one off every neighbour u with core[u] > k, with a returning atomic:
//   old == k + 1   u has just reached the level: appended to the queue, by the one lane that saw k + 1
//   old <= k       u had reached the level before this lane came: the decrement is put back, so nothing rests below its level
//   old >  k + 1   u lives on; old - 1 is a candidate for the next level
// A vertex peeled at level j keeps core = j <= k for good, so "core[u] > k" is also the liveness test: no alive flags.  The
// unlocked read that guards the atomic may be stale, but only high (a value at or under k is final): a stale read costs an
// atomic pair, never a wrong value.  Every vertex enters the queue exactly once in a whole run, so one queue of `nodes` entries and
// one tail word serve all levels: a sub-round is the range [head, tail) and what it appends is the next one.
//
// The next level is the smallest live value.  Every pass that touches a live value carries the minimum of what it saw above k in a
// register (ScanRange: the values it did not collect; Relax: old - 1), one atomicMin per wave at the end.  That minimum can name a
// value that a later decrement took away (a level nobody is at: one more scan of the live list, no sub-round), never miss one.
//
// Rows: a lane per short row, the whole wave per row of `wave_min_row` entries and more; both loops are wave-uniform, so the
// appends of one step are one ballot and one atomic on the tail per wave.
//
// Kernels: ScanKernel / PeelKernel / CompactKernel are the wide forms, one launch per step, the host reading the words in between.
// LoopKernel is one workgroup of 1024 that runs the same three steps in a loop on the device, with a barrier between steps and
// agent-scope accesses on everything a step hands to the next (its CU's L1 is not refreshed by the atomics that land in L2); it
// returns to the host when the work at hand is too wide for one CU, when it is done, or after max_steps.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace kcore {

using oprtr::kLoopThreads;
using oprtr::Ld;
using oprtr::St;
using oprtr::TileFor;

enum { KCORE_AUTO = 0, KCORE_ROUNDS = 1, KCORE_DEVICE_LOOP = 2 };

constexpr int kKcoreThreads = 256;
constexpr int kWaveUnroll = 4;             // chunks of 64 row entries a wave keeps in flight per step of a long row
constexpr double kCompactBelow = 0.75;     // default "compact_below"

// the words the kernels and the host share
enum {
    W_TAIL = 0,      // queue tail: vertices appended so far
    W_LOW,           // smallest live value seen above the current level (UINT_MAX: none)
    W_ENTRIES,       // row entries of all the vertices appended so far, modulo 2^32 (readers take differences)
    W_HEAD,          // LoopKernel's state on return: queue head,
    W_K,             //   current level,
    W_KPREV,         //   the level before it (a vertex is live when core > kprev),
    W_STATUS,        //   why it returned,
    W_LIST_LEN,      //   length of the live list,
    W_LIST_BUF,      //   which buffer holds it (-1: every vertex),
    W_SUBROUNDS,     // sub-rounds LoopKernel ran
    W_TRACE,         // trace entries written
    W_COMPACTIONS,   // live-list rebuilds LoopKernel made
    W_SCANS,         // level scans LoopKernel made
    W_ENTRIES_SEEN,  // W_ENTRIES when the range [.., head) was fixed: the rest belongs to [head, tail)
    W_SCRATCH,       // CompactKernel's counter
    W_COUNT = 16
};
enum { LOOP_DONE = 0, LOOP_WIDE_PEEL = 1, LOOP_WIDE_SCAN = 2, LOOP_STEPS = 3, LOOP_LIMIT = 4 };

constexpr unsigned kNoLevel = 0xFFFFFFFFu;

struct Graph {
    const int *ro;  // [nodes + 1] the symmetric simple neighbour CSR
    const int *ci;
};

struct Trace {
    int *k;                      // one entry per level scan: the level,
    int *tail;                   // the queue tail when it began,
    unsigned long long *clock;   // the constant-rate counter then
};

// what a lane carries through a pass and leaves in the words at its end
struct Tally {
    unsigned low = kNoLevel;   // smallest live value seen above k
    unsigned entries = 0;      // row entries of the vertices this lane appended
    unsigned reads = 0;        // row entries this lane walked
};

// the minimum and the appended entries of a pass: one atomic each per wave
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

// All lanes of the wave call; the lanes with `hit` append u: one atomic on the tail per wave.  (A vertex is appended once in a
// run, so the tail never passes `nodes`, the length of the queue.)
template <bool FRESH>
__device__ __forceinline__ void Append(const Graph &g, bool hit, int u, int *d_queue, unsigned *d_words, Tally &t)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned pos = oprtr::WaveTicket(d_words + W_TAIL, mask);
    if (hit) {
        St<FRESH>(d_queue + pos, u);
        t.entries += static_cast<unsigned>(g.ro[u + 1] - g.ro[u]);
    }
}

// one entry of a peeled vertex's row; returns whether u reached the level through this lane
template <bool FRESH>
__device__ __forceinline__ bool Relax(int *d_core, int u, int k, Tally &t)
{
    ++t.reads;
    if (Ld<FRESH>(d_core + u) <= k) return false;  // peeled, or at the level already (a stale read is only ever high)
    const int old = atomicSub(d_core + u, 1);
    if (old == k + 1) return true;
    if (old <= k) atomicAdd(d_core + u, 1);
    else if (static_cast<unsigned>(old - 1) < t.low) t.low = static_cast<unsigned>(old - 1);
    return false;
}

// 64 queue entries by one wave: lane `lane` holds v (or -1).  Short rows by their lane, rows of wave_min_row and more by the wave.
template <bool FRESH>
__device__ __forceinline__ void PeelTile(const Graph &g, int *d_core, int *d_queue, unsigned *d_words, int v, int k, int wave_min_row, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    int b = 0, e = 0;
    if (v >= 0) {
        b = g.ro[v];
        e = g.ro[v + 1];
    }
    const bool wide = e - b >= wave_min_row && e > b;
    int longest = wide ? 0 : e - b;
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const int other = __shfl_xor(longest, o, util::kWaveSize);
        longest = other > longest ? other : longest;
    }
    for (int j = 0; j < longest; ++j) {  // (wave-uniform)
        int u = 0;
        bool hit = false;
        if (!wide && b + j < e) {
            u = g.ci[b + j];
            hit = Relax<FRESH>(d_core, u, k, t);
        }
        Append<FRESH>(g, hit, u, d_queue, d_words, t);
    }
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
        for (int base = lb; base < le; base += util::kWaveSize * kWaveUnroll) {  // (wave-uniform)
            // kWaveUnroll chunks of 64 entries, each stage of all chunks before the next: the loads, the guards and the returning
            // atomics of a step are in flight together, and a hub's row is walked at a round trip per 256 entries, not per 64
            int us[kWaveUnroll], ds[kWaveUnroll], olds[kWaveUnroll];
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) {
                const int i = base + j * util::kWaveSize + lane;
                us[j] = i < le ? g.ci[i] : -1;
            }
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) ds[j] = us[j] >= 0 ? Ld<FRESH>(d_core + us[j]) : 0;
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) olds[j] = ds[j] > k ? atomicSub(d_core + us[j], 1) : 0;
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) {
                if (us[j] >= 0) ++t.reads;
                bool hit = false;
                if (ds[j] > k) {
                    const int old = olds[j];
                    hit = old == k + 1;
                    if (old <= k) atomicAdd(d_core + us[j], 1);
                    else if (old > k + 1 && static_cast<unsigned>(old - 1) < t.low) t.low = static_cast<unsigned>(old - 1);
                }
                Append<FRESH>(g, hit, us[j], d_queue, d_words, t);
            }
        }
        todo &= todo - 1;
    }
}

// the sub-round [head, tail) of level k by the waves wave0, wave0 + nwaves, ..., `tile` entries each at a time
template <bool FRESH>
__device__ __forceinline__ void PeelRange(const Graph &g, int *d_core, int *d_queue, unsigned *d_words, long long head, long long tail, int k,
                                          int wave_min_row, int tile, long long wave0, long long nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    for (long long base = head + wave0 * tile; base < tail; base += nwaves * tile) {  // (wave-uniform)
        const long long i = base + lane;
        const int v = lane < tile && i < tail ? Ld<FRESH>(d_queue + i) : -1;
        PeelTile<FRESH>(g, d_core, d_queue, d_words, v, k, wave_min_row, t);
    }
}

// the first sub-round of level k: the live vertices (core > kprev) of the list with core <= k; the others give the minimum
template <bool FRESH>
__device__ __forceinline__ void ScanRange(const Graph &g, const int *d_core, const int *d_list, long long count, int kprev, int k, int *d_queue,
                                          unsigned *d_words, long long wave0, long long nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    for (long long base = wave0 * util::kWaveSize; base < count; base += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = base + lane;
        int v = 0;
        bool hit = false;
        if (i < count) {
            v = d_list ? Ld<FRESH>(d_list + i) : static_cast<int>(i);
            const int c = Ld<FRESH>(d_core + v);
            hit = c > kprev && c <= k;
            if (c > k && static_cast<unsigned>(c) < t.low) t.low = static_cast<unsigned>(c);
        }
        Append<FRESH>(g, hit, v, d_queue, d_words, t);
    }
}

// the live vertices of the list, in any order, to d_out; *d_count of them
template <bool FRESH>
__device__ __forceinline__ void CompactRange(const int *d_core, const int *d_list, long long count, int kprev, int *d_out, unsigned *d_count,
                                             long long wave0, long long nwaves)
{
    const int lane = static_cast<int>(util::LaneId());
    for (long long base = wave0 * util::kWaveSize; base < count; base += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = base + lane;
        int v = 0;
        bool keep = false;
        if (i < count) {
            v = d_list ? Ld<FRESH>(d_list + i) : static_cast<int>(i);
            keep = Ld<FRESH>(d_core + v) > kprev;
        }
        const unsigned long long mask = __ballot(keep);
        if (!mask) continue;
        const unsigned pos = oprtr::WaveTicket(d_count, mask);
        if (keep) St<FRESH>(d_out + pos, v);
    }
}

__device__ __forceinline__ void Stamp(const Trace &tr, unsigned *d_words, int k, unsigned tail)
{
    const unsigned at = atomicAdd(d_words + W_TRACE, 1u);  // (levels are distinct values in [1, max degree]: the arrays hold them)
    tr.k[at] = k;
    tr.tail[at] = static_cast<int>(tail);
    tr.clock[at] = wall_clock64();
}

// ---------------- the wide forms ----------------

static __global__ __launch_bounds__(kKcoreThreads) void ScanKernel(Graph g, const int *d_core, const int *d_list, long long count, int kprev, int k,
                                                                    int *d_queue, unsigned *d_words, unsigned long long *d_reads, Trace tr, unsigned tail)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    if (blockIdx.x == 0 && threadIdx.x == 0) Stamp(tr, d_words, k, tail);
    Tally t;
    ScanRange<false>(g, d_core, d_list, count, kprev, k, d_queue, d_words, wave0, nwaves, t);
    Flush(t, d_words);
    FlushReads(t, d_reads);
}

static __global__ __launch_bounds__(kKcoreThreads) void PeelKernel(Graph g, int *d_core, int *d_queue, long long head, long long tail, int k,
                                                                    int wave_min_row, int tile, unsigned *d_words, unsigned long long *d_reads)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    PeelRange<false>(g, d_core, d_queue, d_words, head, tail, k, wave_min_row, tile, wave0, nwaves, t);
    Flush(t, d_words);
    FlushReads(t, d_reads);
}

static __global__ __launch_bounds__(kKcoreThreads) void CompactKernel(const int *d_core, const int *d_list, long long count, int kprev, int *d_out,
                                                                       unsigned *d_count)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    CompactRange<false>(d_core, d_list, count, kprev, d_out, d_count, wave0, nwaves);
}

// ---------------- the device loop ----------------

struct LoopArgs {
    int *d_list[2];          // the two live-list buffers
    int list_buf;            // which one is current, -1: every vertex
    long long list_len;
    long long nodes, zeros;  // vertices, and those of degree 0 (never live)
    long long head;
    unsigned entries_seen;   // W_ENTRIES when `head` was fixed
    int k, kprev;
    int k_limit;             // < 0: none
    int level_open;          // the scan of level k has run: [head, tail) is a sub-round of it
    int wave_min_row;
    double compact_below;
    long long max_list;      // return to the host for a scan of a longer list, ...
    long long max_entries;   // ... and for a sub-round with more row entries
    int max_steps;
};

// One workgroup.  Every step ends in a barrier behind a fence; the words and everything a step leaves for the next are read with
// agent-scope loads.  Uniform control flow: every decision is taken on values all threads read after the same barrier.
static __global__ __launch_bounds__(kLoopThreads) void LoopKernel(Graph g, int *d_core, int *d_queue, unsigned *d_words, unsigned long long *d_reads,
                                                                   Trace tr, LoopArgs a)
{
    __shared__ unsigned s_count;
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    const int *w = reinterpret_cast<const int *>(d_words);
    long long head = a.head, list_len = a.list_len;
    int k = a.k, kprev = a.kprev, list_buf = a.list_buf, status = LOOP_STEPS;
    bool open = a.level_open != 0;
    unsigned subrounds = 0, compactions = 0, scans = 0, entries_seen = a.entries_seen;
    Tally t;
    for (int step = 0; step < a.max_steps; ++step) {
        const long long tail = static_cast<unsigned>(Ld<true>(w + W_TAIL));
        if (open && head < tail) {  // a sub-round of level k
            const unsigned entries = static_cast<unsigned>(Ld<true>(w + W_ENTRIES));
            if (entries - entries_seen > a.max_entries) { status = LOOP_WIDE_PEEL; break; }
            __syncthreads();  // (everybody has read the words)
            PeelRange<true>(g, d_core, d_queue, d_words, head, tail, k, a.wave_min_row, TileFor(tail - head, nwaves, entries - entries_seen), wave0, nwaves, t);
            Flush(t, d_words);
            head = tail;
            entries_seen = entries;
            ++subrounds;
            __threadfence();
            __syncthreads();
            continue;
        }
        if (open) {  // level k has run dry: the next one is the smallest live value
            const unsigned low = static_cast<unsigned>(Ld<true>(w + W_LOW));
            kprev = k;
            open = false;
            if (low == kNoLevel || a.nodes - a.zeros - tail <= 0) { status = LOOP_DONE; break; }
            k = static_cast<int>(low);
        }
        if (a.k_limit >= 0 && k >= a.k_limit) { status = LOOP_LIMIT; break; }
        const long long alive = a.nodes - a.zeros - tail;
        if (a.compact_below > 0 && static_cast<double>(alive) <= a.compact_below * static_cast<double>(list_len) && list_len <= a.max_list) {
            const int to = list_buf == 0 ? 1 : 0;
            if (threadIdx.x == 0) s_count = 0;
            __syncthreads();
            CompactRange<true>(d_core, list_buf < 0 ? nullptr : a.d_list[list_buf], list_len, kprev, a.d_list[to], &s_count, wave0, nwaves);
            __threadfence();
            __syncthreads();
            list_buf = to;
            list_len = s_count;
            ++compactions;
            __syncthreads();
        }
        if (list_len > a.max_list) { status = LOOP_WIDE_SCAN; break; }
        __syncthreads();
        if (threadIdx.x == 0) {
            St<true>(reinterpret_cast<int *>(d_words) + W_LOW, static_cast<int>(kNoLevel));
            Stamp(tr, d_words, k, static_cast<unsigned>(tail));
        }
        __threadfence();
        __syncthreads();
        ScanRange<true>(g, d_core, list_buf < 0 ? nullptr : a.d_list[list_buf], list_len, kprev, k, d_queue, d_words, wave0, nwaves, t);
        Flush(t, d_words);
        open = true;
        ++scans;
        __threadfence();
        __syncthreads();
    }
    FlushReads(t, d_reads);
    __syncthreads();
    if (threadIdx.x == 0) {
        int *out = reinterpret_cast<int *>(d_words);
        out[W_ENTRIES_SEEN] = static_cast<int>(entries_seen);
        out[W_HEAD] = static_cast<int>(head);
        out[W_K] = k;
        out[W_KPREV] = kprev;
        out[W_STATUS] = status | (open ? 0x100 : 0);
        out[W_LIST_LEN] = static_cast<int>(list_len);
        out[W_LIST_BUF] = list_buf;
        out[W_SUBROUNDS] += static_cast<int>(subrounds);
        out[W_COMPACTIONS] += static_cast<int>(compactions);
        out[W_SCANS] += static_cast<int>(scans);
    }
}

// ---------------- around the peel ----------------

// a limited run: what is still live when level k_limit is reached has a core number of at least k_limit
static __global__ void ClampKernel(int *d_core, long long nodes, int k_limit)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride)
        if (d_core[v] > k_limit) d_core[v] = k_limit;
}

// both directions of every kept edge, each at its row's cursor (the order inside a row is the arrival order: nothing reads it)
static __global__ void NeighbourScatterKernel(const unsigned long long *d_keys, const unsigned *d_keep, long long count, int col_bits,
                                              const int *d_ro, unsigned *d_cursor, int *d_ci)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (!d_keep[i]) continue;
        const unsigned long long key = d_keys[i];
        const unsigned a = static_cast<unsigned>(key >> col_bits), b = static_cast<unsigned>(key & mask);
        d_ci[d_ro[a] + static_cast<int>(atomicAdd(d_cursor + a, 1u))] = static_cast<int>(b);
        d_ci[d_ro[b] + static_cast<int>(atomicAdd(d_cursor + b, 1u))] = static_cast<int>(a);
    }
}

// d_out[0] = the largest value, d_out[1] = the smallest positive one (UINT_MAX: none), d_out[2] = how many are 0
static __global__ void SummaryKernel(const int *d_values, long long nodes, unsigned *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned most = 0, least = kNoLevel, zeros = 0;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const unsigned d = static_cast<unsigned>(d_values[v]);
        most = d > most ? d : most;
        if (d == 0) ++zeros;
        else least = d < least ? d : least;
    }
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const unsigned m = __shfl_xor(most, o, util::kWaveSize), l = __shfl_xor(least, o, util::kWaveSize);
        most = m > most ? m : most;
        least = l < least ? l : least;
        zeros += __shfl_xor(zeros, o, util::kWaveSize);
    }
    if (util::LaneId() == 0) {
        atomicMax(d_out, most);
        atomicMin(d_out + 1, least);
        if (zeros) atomicAdd(d_out + 2, zeros);
    }
}

// shell[c] += the vertices with core c: the lanes of a wave that hold the same value add once (most of an R-MAT graph sits in a
// few shells: one atomic per vertex would queue on a few words)
static __global__ void ShellKernel(const int *d_core, long long nodes, unsigned long long *d_shell)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (long long r = 0; r < rounds; ++r, v += stride) {  // (wave-uniform)
        const int c = v < nodes ? d_core[v] : -1;
        unsigned long long todo = __ballot(c >= 0);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int value = __shfl(c, leader, util::kWaveSize);
            const unsigned long long same = __ballot(c == value);
            if (static_cast<int>(util::LaneId()) == leader) atomicAdd(d_shell + value, static_cast<unsigned long long>(__popcll(same)));
            todo &= ~same;
        }
    }
}

// mask[v] = core[v] >= k; d_out[0] += the members, d_out[1] += the entries (v, u) of the neighbour CSR with v < u and both members
static __global__ __launch_bounds__(kKcoreThreads) void MembersKernel(Graph g, const int *d_core, long long nodes, int k, int wave_min_row,
                                                                       unsigned char *d_mask, unsigned long long *d_out)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    unsigned long long members = 0, edges = 0;
    for (long long base = wave0 * util::kWaveSize; base < nodes; base += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long v = base + lane;
        int b = 0, e = 0;
        if (v < nodes) {
            const bool in = d_core[v] >= k;
            d_mask[v] = in ? 1 : 0;
            if (in) {
                ++members;
                b = g.ro[v];
                e = g.ro[v + 1];
            }
        }
        const bool wide = e - b >= wave_min_row && e > b;
        if (!wide)
            for (int i = b; i < e; ++i) {
                const int u = g.ci[i];
                if (u > v && d_core[u] >= k) ++edges;
            }
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
            const long long lv = base + leader;
            for (int i = lb + lane; i < le; i += util::kWaveSize) {
                const int u = g.ci[i];
                if (u > lv && d_core[u] >= k) ++edges;
            }
            todo &= todo - 1;
        }
    }
    members = util::WaveSum(members);
    edges = util::WaveSum(edges);
    if (lane == 0) {
        if (members) atomicAdd(d_out, members);
        if (edges) atomicAdd(d_out + 1, edges);
    }
}

}  // namespace kcore
}  // namespace app
}  // namespace gunrock
