// app/msbfs/msbfs_functor.hpp -- device kernels of the bit-parallel multi-source BFS (MS-BFS, Then et al., VLDB 2014).
//
// The reference snapshot has no app/msbfs; the shape follows this tree's primitives (app/scc/scc_functor.hpp: the row walk by
// lane or by wave, the ballot append).  The CSR is read as a directed multigraph.  A batch is up to 64 sources; every vertex
// carries one 64-bit word per array and bit b belongs to the batch's source b:
//   seen[v]      the searches that have reached v
//   frontier[v]  the searches that reached v at the previous level (0 outside the frontier)
//   next[v]      a push level's collecting word (0 between levels), a pull level's output
// A level is a PUSH (PushKernel over the queue of frontier vertices, then UpdateKernel over the vertices it reached) or a PULL
// (PullKernel over every vertex that some search of the batch has not reached, on the in-neighbour lists; the host then swaps
// frontier[] and next[]).  The dense frontier[] is valid after either, so a pull can follow a push at once; a push after a pull
// takes CompactKernel for its queue.  Both settle a reached vertex the same way (Settle): the per-vertex sums, the depths when
// stored, and the per-source counts, which are one ballot per source and wave, kept by lane b for source b until the block ends.
// Nothing is exchanged between workgroups inside a launch but atomics whose returned value is all that is used.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace msbfs {

using oprtr::kWaveMinRow;  // default "wave_min_row"
using oprtr::TileFor;

enum { MSBFS_AUTO = 0, MSBFS_PUSH = 1, MSBFS_PULL = 2, MSBFS_ALTERNATE = 3 };
enum { INVERSE_AUTO = 0, INVERSE_NONE = 1, INVERSE_SELF = 2, INVERSE_BUILD = 3 };
enum { LEVEL_PUSH = 0, LEVEL_PULL = 1 };

typedef unsigned long long Word;

constexpr int kThreads = 256;
constexpr int kBatch = 64;        // sources per batch: the bits of a Word, the lanes of a wave
constexpr double kAlpha = 4.0;    // default "alpha": push -> pull when frontier edges * alpha > unexplored edges
constexpr double kBeta = 24.0;    // default "beta": pull -> push when frontier vertices * beta < nodes

// the 64-bit words a level's kernels and the host share: zeroed before every level
enum {
    W_TAIL = 0,        // queue tickets handed out
    W_NEW,             // vertices reached at this level
    W_FRONTIER_EDGES,  // their out-row entries
    W_FULL_EDGES,      // row entries of the vertices that every search of the batch has now reached
    W_READS,           // row entries walked
    W_COUNT = 8
};

struct Ctx {
    const int *ro, *ci;    // G
    const int *iro, *ici;  // the in-neighbour lists (nullptr: none, every level is a push)
    Word *seen, *frontier, *next;
    int *queue_in, *queue_out;
    Word *words;
    unsigned long long *reached, *dist_sum;  // of this batch's source 0 (int64 on the host side)
    int *ecc;
    int *sources_reaching;
    unsigned long long *in_dist_sum;
    int *depth;  // row 0 is this batch's source 0, a row is `nodes` long; nullptr: not stored
    Word mask;   // the batch's sources: the low (k % 64) bits in a partial last batch
    int nodes;
    int level;
    int wave_min_row;
};

struct Tally {
    unsigned long long frontier_edges = 0, full_edges = 0;
    unsigned reads = 0, fresh = 0;
    unsigned mine = 0;  // lane b: vertices that source b reached
};

__device__ __forceinline__ Word WaveOr(Word x)
{
#pragma unroll
    for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) x |= __shfl_xor(x, d, util::kWaveSize);
    return x;
}

// All lanes of the wave call.  `fresh`: the searches that reach v at this level (0: none, or an idle lane), `before`: seen[v] as it
// was.  The caller has written the three state words.
__device__ __forceinline__ void Settle(const Ctx &c, int v, Word fresh, Word before, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    if (fresh) {
        const unsigned count = static_cast<unsigned>(__popcll(fresh));
        c.sources_reaching[v] += static_cast<int>(count);
        c.in_dist_sum[v] += static_cast<unsigned long long>(count) * static_cast<unsigned long long>(c.level);
        if (c.depth) {
            Word todo = fresh & c.mask;  // (rows past the batch's last source do not exist)
            while (todo) {
                const int b = __ffsll(static_cast<long long>(todo)) - 1;
                c.depth[static_cast<size_t>(b) * static_cast<size_t>(c.nodes) + static_cast<size_t>(v)] = c.level;
                todo &= todo - 1;
            }
        }
        ++t.fresh;
        t.frontier_edges += static_cast<unsigned long long>(c.ro[v + 1] - c.ro[v]);
        if (((before | fresh) & c.mask) == c.mask)
            t.full_edges += static_cast<unsigned long long>(c.iro ? c.iro[v + 1] - c.iro[v] : c.ro[v + 1] - c.ro[v]);
    }
#pragma unroll
    for (int b = 0; b < kBatch; ++b) {  // (wave-uniform: one ballot per source)
        const unsigned count = static_cast<unsigned>(__popcll(__ballot((fresh >> b) & 1ull)));
        t.mine += lane == b ? count : 0u;
    }
}

// The end of a settling kernel; every thread of the block calls.  One atomic per workgroup and source; the mask keeps the bits a
// partial batch does not have out of the sums whatever the words held.
__device__ __forceinline__ void Flush(const Ctx &c, Tally &t, unsigned *counts)
{
    const int lane = static_cast<int>(util::LaneId());
    if (threadIdx.x < kBatch) counts[threadIdx.x] = 0;
    __syncthreads();
    if (t.mine) atomicAdd(counts + lane, t.mine);
    __syncthreads();
    if (threadIdx.x < kBatch) {
        const unsigned count = counts[threadIdx.x];
        if (count && ((c.mask >> threadIdx.x) & 1ull)) {
            atomicAdd(c.reached + threadIdx.x, static_cast<unsigned long long>(count));
            atomicAdd(c.dist_sum + threadIdx.x, static_cast<unsigned long long>(count) * static_cast<unsigned long long>(c.level));
            atomicMax(c.ecc + threadIdx.x, c.level);
        }
    }
    const unsigned long long frontier_edges = util::WaveSum(t.frontier_edges), full_edges = util::WaveSum(t.full_edges);
    const unsigned long long reads = util::WaveSum(static_cast<unsigned long long>(t.reads)), fresh = util::WaveSum(static_cast<unsigned long long>(t.fresh));
    if (lane == 0) {
        if (frontier_edges) atomicAdd(c.words + W_FRONTIER_EDGES, frontier_edges);
        if (full_edges) atomicAdd(c.words + W_FULL_EDGES, full_edges);
        if (reads) atomicAdd(c.words + W_READS, reads);
        if (fresh) atomicAdd(c.words + W_NEW, fresh);
    }
}

// All lanes of the wave call; the lanes with `hit` append v: one atomic on the ticket word per wave.  A vertex is appended at most
// once per level, so a position stays under `nodes`, the queue's length; the test keeps a mistake elsewhere inside the buffer.
__device__ __forceinline__ void Append(const Ctx &c, bool hit, int v, int *d_out)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    unsigned long long at = 0;
    if (util::LaneId() == 0) at = atomicAdd(c.words + W_TAIL, static_cast<unsigned long long>(__popcll(mask)));
    at = __shfl(at, 0, util::kWaveSize);
    if (hit) {
        const unsigned long long pos = at + util::RankInMask(mask);
        if (pos < static_cast<unsigned long long>(c.nodes)) d_out[pos] = v;
    }
}

// The searches of `fw` that v has not seen go into next[v]; the one lane that finds the word empty queues v.  seen[] is not written
// during a push, so the screen is exact; the OR is relaxed at agent scope and only its returned value is used.
__device__ __forceinline__ bool Relax(const Ctx &c, Word fw, int v)
{
    const Word d = fw & ~c.seen[v];
    if (!d) return false;
    return __hip_atomic_fetch_or(c.next + v, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
}

// The batch's sources (one wave, lane b holds source b): their bits, the first queue and the first level's words.  Duplicate
// vertices share a word; the lane that finds frontier[] empty owns the vertex.
static __global__ __launch_bounds__(kBatch) void InitKernel(Ctx c, const int *d_sources, int count)
{
    const int lane = static_cast<int>(util::LaneId());
    const int s = lane < count ? d_sources[lane] : -1;
    bool owner = false;
    if (s >= 0) {
        const Word bit = 1ull << lane;
        __hip_atomic_fetch_or(c.seen + s, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        owner = __hip_atomic_fetch_or(c.frontier + s, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
    }
    __syncthreads();
    unsigned long long frontier_edges = 0, full_edges = 0;
    if (owner) {
        frontier_edges = static_cast<unsigned long long>(c.ro[s + 1] - c.ro[s]);
        if ((__hip_atomic_load(c.seen + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & c.mask) == c.mask)
            full_edges = static_cast<unsigned long long>(c.iro ? c.iro[s + 1] - c.iro[s] : c.ro[s + 1] - c.ro[s]);
    }
    const unsigned long long owners = __ballot(owner);
    if (owner) {
        const unsigned pos = util::RankInMask(owners);
        if (pos < static_cast<unsigned>(c.nodes)) c.queue_in[pos] = s;
    }
    frontier_edges = util::WaveSum(frontier_edges);
    full_edges = util::WaveSum(full_edges);
    if (lane == 0) {
        c.words[W_TAIL] = static_cast<unsigned long long>(__popcll(owners));
        c.words[W_NEW] = static_cast<unsigned long long>(__popcll(owners));
        c.words[W_FRONTIER_EDGES] = frontier_edges;
        c.words[W_FULL_EDGES] = full_edges;
    }
}

// A push level over queue_in[0, count), `tile` entries per wave at a time: rows shorter than wave_min_row by their lane, the others
// by the wave; both loops are wave-uniform.  The walker of u is the only reader of frontier[u] and clears it.
static __global__ __launch_bounds__(kThreads) void PushKernel(Ctx c, long long count, int tile)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    unsigned reads = 0;
    for (long long from = wave0 * tile; from < count; from += nwaves * tile) {  // (wave-uniform)
        const long long i = from + lane;
        Word fw = 0;
        int b = 0, e = 0;
        if (lane < tile && i < count) {
            const int u = c.queue_in[i];
            fw = c.frontier[u];
            c.frontier[u] = 0;
            b = c.ro[u];
            e = c.ro[u + 1];
        }
        const bool wide = e - b >= c.wave_min_row && e > b;
        int longest = wide ? 0 : e - b;
        for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
            const int other = __shfl_xor(longest, o, util::kWaveSize);
            longest = other > longest ? other : longest;
        }
        for (int j = 0; j < longest; ++j) {  // (wave-uniform)
            int v = 0;
            bool hit = false;
            if (!wide && b + j < e) {
                v = c.ci[b + j];
                ++reads;
                hit = Relax(c, fw, v);
            }
            Append(c, hit, v, c.queue_out);
        }
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
            const Word lfw = __shfl(fw, leader, util::kWaveSize);
            for (int at = lb; at < le; at += util::kWaveSize) {  // (wave-uniform)
                int v = 0;
                bool hit = false;
                if (at + lane < le) {
                    v = c.ci[at + lane];
                    ++reads;
                    hit = Relax(c, lfw, v);
                }
                Append(c, hit, v, c.queue_out);
            }
            todo &= todo - 1;
        }
    }
    const unsigned long long total = util::WaveSum(static_cast<unsigned long long>(reads));
    if (lane == 0 && total) atomicAdd(c.words + W_READS, total);
}

// After a push: the vertices it queued (W_TAIL of them; next[v] is non-zero by construction) take their new bits.
static __global__ __launch_bounds__(kThreads) void UpdateKernel(Ctx c)
{
    __shared__ unsigned counts[kBatch];
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    unsigned long long tail = c.words[W_TAIL];
    const long long count = tail < static_cast<unsigned long long>(c.nodes) ? static_cast<long long>(tail) : c.nodes;
    Tally t;
    for (long long from = wave0 * util::kWaveSize; from < count; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = from + lane;
        int v = -1;
        Word fresh = 0, before = 0;
        if (i < count) {
            v = c.queue_out[i];
            fresh = c.next[v];
            before = c.seen[v];
            c.seen[v] = before | fresh;
            c.frontier[v] = fresh;
            c.next[v] = 0;
        }
        Settle(c, v, fresh, before, t);
    }
    Flush(c, t, counts);
}

// A pull level: every vertex that some search of the batch has not reached ORs the frontier words of its in-neighbours and stops as
// soon as nothing is missing; next[v] is written for EVERY vertex (the host swaps it with frontier[]).  No atomics on the state: v's
// words are written by the lane that holds v, and frontier[] is only read.
static __global__ __launch_bounds__(kThreads) void PullKernel(Ctx c)
{
    __shared__ unsigned counts[kBatch];
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    for (long long from = wave0 * util::kWaveSize; from < c.nodes; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = from + lane;
        const int v = i < c.nodes ? static_cast<int>(i) : -1;
        const Word before = v >= 0 ? c.seen[v] : c.mask;
        const Word need = ~before & c.mask;
        int b = 0, e = 0;
        if (need) {
            b = c.iro[v];
            e = c.iro[v + 1];
        }
        const bool wide = e - b >= c.wave_min_row && e > b;
        Word acc = 0;
        if (!wide)
            for (int at = b; at < e; ++at) {
                acc |= c.frontier[c.ici[at]];
                ++t.reads;
                if ((acc & need) == need) break;
            }
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
            const Word lneed = __shfl(need, leader, util::kWaveSize);
            Word whole = 0;
            for (int at = lb; at < le; at += util::kWaveSize) {  // (wave-uniform)
                Word part = 0;
                if (at + lane < le) {
                    part = c.frontier[c.ici[at + lane]];
                    ++t.reads;
                }
                whole |= WaveOr(part);
                if ((whole & lneed) == lneed) break;
            }
            if (lane == leader) acc = whole;
            todo &= todo - 1;
        }
        const Word fresh = acc & need;
        if (v >= 0) {
            c.next[v] = fresh;
            if (fresh) c.seen[v] = before | fresh;
        }
        Settle(c, v, fresh, before, t);
    }
    Flush(c, t, counts);
}

// The queue of a push that follows a pull: the vertices with a frontier word
static __global__ __launch_bounds__(kThreads) void CompactKernel(Ctx c)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    for (long long from = wave0 * util::kWaveSize; from < c.nodes; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = from + lane;
        const bool hit = i < c.nodes && c.frontier[i] != 0;
        Append(c, hit, static_cast<int>(i), c.queue_in);
    }
}

// Reset: every source has reached itself at depth 0
static __global__ void ResetKernel(const int *d_sources, long long count, int nodes, unsigned long long *d_reached, unsigned long long *d_dist_sum,
                                   int *d_ecc, int *d_sources_reaching, int *d_depth)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long s = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; s < count; s += stride) {
        const int v = d_sources[s];
        d_reached[s] = 1;
        d_dist_sum[s] = 0;
        d_ecc[s] = 0;
        atomicAdd(d_sources_reaching + v, 1);
        if (d_depth) d_depth[static_cast<size_t>(s) * static_cast<size_t>(nodes) + static_cast<size_t>(v)] = 0;
    }
}

}  // namespace msbfs
}  // namespace app
}  // namespace gunrock
