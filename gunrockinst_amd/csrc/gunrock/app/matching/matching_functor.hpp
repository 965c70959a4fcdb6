// app/matching/matching_functor.hpp -- device kernels of the heavy-edge matching (the locally dominant matching) and its contraction.
//
// The reference snapshot has no matching; the shape follows this tree's primitives: max-flow's lane / wave row balance, its next
// list with one ticket per wave and its one-workgroup device loop (scc_functor.hpp is included for the accessors and the tile rule,
// maxflow_functor.hpp's RowFind is restated because that header brings its own Ctx; neither is changed).
//
// The graph is the neighbour CSR over the canonical pairs: row v holds the distinct neighbours of v ascending, eid[i] is the pair of
// entry i and ew[i] its weight (NULL: every weight is 1).  Pairs are strictly ordered by
//     key(e) = ((uint32)w(e) ^ 0x80000000) << 32 | Fmix32((uint32)e + seed * 0x9E3779B9)
// and the matching is the one solution of  in[e] = no pair f that shares an end with e and has key(f) > key(e) has in[f].
//
//   point   every vertex of the live list names the largest-keyed pair of its row whose other end is unmatched: tgt[v] is that end
//           and pp[v] the pair.  A vertex that named one before asks first whether tgt[v] is still unmatched (one entry: a poll) and
//           keeps its pointer then: nothing that became matched can have raised another key over it.  Otherwise it walks its row
//           from cur[v], the first entry that had an unmatched end at the last walk (matched vertices stay matched, so everything in
//           front of it is out for good).  No unmatched neighbour: pp[v] = -1 and the vertex leaves.  Keys are computed in
//           registers from eid[i] and ew[i]; none is stored.
//   match   a vertex whose pointer is answered (pp[tgt[v]] == pp[v]) writes mate[v]; the smaller end writes in_matching[] and
//           counts the pair.  Everybody else with a pointer enters the next list: one ticket per wave.
// The largest-keyed pair with two unmatched ends is the pointer of both, so every round with such a pair matches one; a round
// without one empties the list.  Nothing in a step reads what the same step writes: point reads mate[] and writes tgt / pp / cur of
// its own vertex, match reads pp[] / tgt[] and writes mate[] of its own vertex.  Between the two, and between rounds, is a kernel
// boundary or, in the device loop, a fence and a barrier; there every read of what an earlier step left is an agent-scope load (a
// CU's L1 is not refreshed by what lands in L2).  In the end medge[v] is pp[v]: -1 for every vertex that left unmatched.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace matching {

enum { MATCHING_AUTO = 0, MATCHING_ROUNDS = 1, MATCHING_DEVICE_LOOP = 2 };
enum { STEP_WIDE = 0, STEP_LOOP = 1 };  // the kinds of the round trace

constexpr int kMatchingThreads = 256;
constexpr long long kLoopMaxEntries = 65536;  // AUTO: the device loop takes a round whose rows hold up to this many entries, not the
                                              // shared 8192: an upper bound of the round's reads that is loose here, most of a list
                                              // polls one entry (by reasoning, not tuned)
constexpr int kWaveUnroll = 4;               // chunks of 64 row entries a wave keeps in flight on a long row (as MIS's sweep does)

using oprtr::kLoopMaxSteps;
using oprtr::kLoopThreads;
using oprtr::kWaveMinRow;
using oprtr::Ld;
using oprtr::Limits;
using oprtr::Narrow;
using oprtr::St;
using oprtr::TileFor;
using util::Fmix32;

// the words the kernels and the host share
enum {
    W_NEXT = 0,      // vertices in the next list
    W_NEXT_ENTRIES,  // their row entries (the word behind W_NEXT: the two are cleared together)
    W_MATCHED,       // pairs matched since Reset
    W_FLAG,          // contract: a sum left int32
    W_COUNT = 8
};

// the 64-bit counters
enum { C_READS = 0, C_POLLS, C_WEIGHT, C_COUNT = 4 };

struct Ctx {
    const int *ro, *ci, *eid, *ew;  // the neighbour CSR, the pair and the weight (or NULL) of every entry
    const int *pw;                  // weight per pair
    int *mate, *tgt, *pp, *cur;     // per vertex
    unsigned char *in_matching;     // per pair
    unsigned *words;
    unsigned long long *counters;
    int nodes;
    unsigned seed_mul;  // seed * 0x9E3779B9
    int wave_min_row;
};

// the next round; the host and LoopKernel carry the same
struct Active {
    unsigned count, entries;  // the current list and its row entries
    int cur;                  // which of the two lists it is
    unsigned matched;         // W_MATCHED behind the last round
    int steps;                // rounds run by the loop launch ...
    int match_steps;          // ... and those of them that matched a pair
};

__host__ __device__ __forceinline__ unsigned long long PairKey(int weight, int pair, unsigned seed_mul)
{
    return (static_cast<unsigned long long>(static_cast<unsigned>(weight) ^ 0x80000000u) << 32) | Fmix32(static_cast<unsigned>(pair) + seed_mul);
}

struct Tally {
    unsigned entries = 0;  // row entries of the vertices this lane listed
    unsigned reads = 0;    // row entries this lane walked
    unsigned polls = 0;
    unsigned matched = 0;
    long long weight = 0;
};

__device__ __forceinline__ void Flush(Tally &t, const Ctx &c)
{
    const unsigned entries = util::WaveSum(t.entries), matched = util::WaveSum(t.matched);
    const unsigned long long reads = util::WaveSum(static_cast<unsigned long long>(t.reads));
    const unsigned long long polls = util::WaveSum(static_cast<unsigned long long>(t.polls));
    const unsigned long long weight = util::WaveSum(static_cast<unsigned long long>(t.weight));  // (two's complement: it may be negative)
    if (util::LaneId() == 0) {
        if (entries) atomicAdd(c.words + W_NEXT_ENTRIES, entries);
        if (matched) {
            atomicAdd(c.words + W_MATCHED, matched);
            atomicAdd(c.counters + C_WEIGHT, weight);
        }
        if (reads) atomicAdd(c.counters + C_READS, reads);
        if (polls) atomicAdd(c.counters + C_POLLS, polls);
    }
    t = Tally();
}

// All lanes of the wave call; the lanes with `hit` append v to list[] through W_NEXT: one atomic per wave.  A vertex enters a list
// once, so a position stays under `nodes`; the test keeps a mistake elsewhere from turning into a store outside the array.
template <bool FRESH>
__device__ __forceinline__ void Append(const Ctx &c, int *list, bool hit, int v, Tally &t)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned pos = oprtr::WaveTicket(c.words + W_NEXT, mask);
    if (hit) {
        if (pos < static_cast<unsigned>(c.nodes)) St<FRESH>(list + pos, v);
        t.entries += static_cast<unsigned>(c.ro[v + 1] - c.ro[v]);
    }
}

// ---------------- the point step ----------------

// what a walk knows: the best entry so far (-1: none), its key, and the first entry with an unmatched end
struct Best {
    unsigned long long key = 0;
    int at = -1;
    int first = INT_MAX;
};

__device__ __forceinline__ void Take(Best &b, unsigned long long key, int at, int first)
{
    if (at >= 0 && (b.at < 0 || key > b.key)) {
        b.key = key;
        b.at = at;
    }
    b.first = first < b.first ? first : b.first;
}

// entry i as a candidate
template <bool FRESH>
__device__ __forceinline__ void Look(const Ctx &c, int i, Best &b, Tally &t)
{
    ++t.reads;
    if (Ld<FRESH>(c.mate + c.ci[i]) >= 0) return;
    Take(b, PairKey(c.ew ? c.ew[i] : 1, c.eid[i], c.seed_mul), i, i);
}

__device__ __forceinline__ Best WaveBest(Best b)
{
#pragma unroll
    for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) {
        const unsigned long long key = __shfl_xor(b.key, d, util::kWaveSize);
        const int at = __shfl_xor(b.at, d, util::kWaveSize), first = __shfl_xor(b.first, d, util::kWaveSize);
        Take(b, key, at, first);
    }
    return b;
}

// 64 list entries by one wave: lane `lane` holds v (or -1).  Rows with fewer than wave_min_row entries left by their lane, the others
// by the whole wave with a wave-wide reduction, one after the other.  Every loop that holds a wave operation is wave-uniform.
template <bool FRESH>
__device__ __forceinline__ void PointTile(const Ctx &c, int v, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    int b = 0, e = 0;
    bool walk = false;
    if (v >= 0) {
        walk = true;
        if (Ld<FRESH>(c.pp + v) >= 0) {  // the poll
            ++t.polls;
            walk = Ld<FRESH>(c.mate + Ld<FRESH>(c.tgt + v)) >= 0;
        }
        if (walk) {
            b = Ld<FRESH>(c.cur + v);
            e = c.ro[v + 1];
        }
    }
    const bool wide = walk && e - b >= c.wave_min_row && e > b;
    Best best;
    if (walk && !wide)
        for (int i = b; i < e; ++i) Look<FRESH>(c, i, best, t);
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
        Best part;
        for (int base = lb; base < le; base += util::kWaveSize * kWaveUnroll) {  // (kWaveUnroll chunks of the row in flight)
            int w[kWaveUnroll], m[kWaveUnroll];
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) {
                const int i = base + j * util::kWaveSize + lane;
                w[j] = i < le ? c.ci[i] : -1;
            }
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) m[j] = w[j] >= 0 ? Ld<FRESH>(c.mate + w[j]) : 0;
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) {
                const int i = base + j * util::kWaveSize + lane;
                if (w[j] < 0) continue;
                ++t.reads;
                if (m[j] < 0) Take(part, PairKey(c.ew ? c.ew[i] : 1, c.eid[i], c.seed_mul), i, i);
            }
        }
        part = WaveBest(part);
        if (lane == leader) best = part;
        todo &= todo - 1;
    }
    if (walk) {
        St<FRESH>(c.cur + v, best.at >= 0 ? best.first : e);
        St<FRESH>(c.pp + v, best.at >= 0 ? c.eid[best.at] : -1);
        if (best.at >= 0) St<FRESH>(c.tgt + v, c.ci[best.at]);
    }
}

// ---------------- the match step ----------------

template <bool FRESH>
__device__ __forceinline__ void MatchTile(const Ctx &c, int v, int *next, Tally &t)
{
    bool again = false;
    if (v >= 0) {
        const int pair = Ld<FRESH>(c.pp + v);
        if (pair >= 0) {
            const int w = Ld<FRESH>(c.tgt + v);
            if (Ld<FRESH>(c.pp + w) == pair) {
                St<FRESH>(c.mate + v, w);
                if (v < w) {
                    c.in_matching[pair] = 1;
                    ++t.matched;
                    t.weight += c.pw[pair];
                }
            } else {
                again = true;
            }
        }
    }
    Append<FRESH>(c, next, again, v, t);
}

template <bool FRESH, bool MATCH>
__device__ __forceinline__ void StepList(const Ctx &c, const int *cur, int *next, long long count, int tile, long long wave0, long long nwaves,
                                         Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    if (count > c.nodes) count = c.nodes;
    for (long long from = wave0 * tile; from < count; from += nwaves * tile) {  // (wave-uniform)
        const long long i = from + lane;
        int v = -1;
        if (lane < tile && i < count) v = Ld<FRESH>(cur + i);
        if (MATCH) MatchTile<FRESH>(c, v, next, t);
        else PointTile<FRESH>(c, v, t);
    }
}

static __global__ __launch_bounds__(kMatchingThreads) void PointKernel(Ctx c, const int *cur, unsigned count, int tile)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    StepList<false, false>(c, cur, nullptr, count, tile, wave0, nwaves, t);
    Flush(t, c);
}

static __global__ __launch_bounds__(kMatchingThreads) void MatchKernel(Ctx c, const int *cur, int *next, unsigned count)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    StepList<false, true>(c, cur, next, count, util::kWaveSize, wave0, nwaves, t);
    Flush(t, c);
}

// One workgroup runs round after round while the list is narrow and not empty; at most lim.max_steps rounds per launch.  Every step
// ends in a barrier behind a fence, the words are read with agent-scope loads by every thread, and a further barrier keeps the next
// step's atomics behind those reads.  Uniform control flow: every thread carries the same Active.  W_NEXT and W_NEXT_ENTRIES are 0
// at entry and at exit.
static __global__ __launch_bounds__(kLoopThreads) void LoopKernel(Ctx c, int *list0, int *list1, Active a, Limits lim, Active *d_active)
{
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    const int *words = reinterpret_cast<const int *>(c.words);
    Tally t;
    a.steps = a.match_steps = 0;
    while (a.steps < lim.max_steps && a.count > 0 && Narrow(a.count, a.entries, lim)) {
        const int *cur = a.cur ? list1 : list0;
        int *next = a.cur ? list0 : list1;
        const int tile = TileFor(static_cast<long long>(a.count), nwaves, a.entries);
        StepList<true, false>(c, cur, next, a.count, tile, wave0, nwaves, t);
        __threadfence();
        __syncthreads();
        StepList<true, true>(c, cur, next, a.count, util::kWaveSize, wave0, nwaves, t);
        Flush(t, c);
        __threadfence();
        __syncthreads();
        const unsigned count = static_cast<unsigned>(Ld<true>(words + W_NEXT));
        const unsigned matched = static_cast<unsigned>(Ld<true>(words + W_MATCHED));
        a.entries = static_cast<unsigned>(Ld<true>(words + W_NEXT_ENTRIES));
        a.count = count < static_cast<unsigned>(c.nodes) ? count : static_cast<unsigned>(c.nodes);
        a.cur ^= 1;
        ++a.steps;
        if (matched != a.matched) ++a.match_steps;
        a.matched = matched;
        __syncthreads();
        if (threadIdx.x == 0) {
            St<true>(reinterpret_cast<int *>(c.words) + W_NEXT, 0);
            St<true>(reinterpret_cast<int *>(c.words) + W_NEXT_ENTRIES, 0);
        }
        __threadfence();
        __syncthreads();
    }
    if (threadIdx.x == 0) *d_active = a;
}

// Reset: nobody is matched or points anywhere, every walk starts at the head of its row, and the vertices with a neighbour are the
// first list
static __global__ void SeedKernel(Ctx c, int *list)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (c.nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    Tally t;
    for (long long r = 0; r < rounds; ++r, v += stride) {  // (wave-uniform)
        bool hit = false;
        if (v < c.nodes) {
            c.mate[v] = c.pp[v] = c.tgt[v] = -1;
            c.cur[v] = c.ro[v];
            hit = c.ro[v + 1] > c.ro[v];
        }
        Append<false>(c, list, hit, static_cast<int>(v), t);
    }
    Flush(t, c);
}

// ---------------- the build ----------------

// the entry of row u that holds w (it is there: rows are ascending and distinct)
__device__ __forceinline__ int RowFind(const int *ro, const int *ci, int u, int w)
{
    int lo = ro[u], hi = ro[u + 1];
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (ci[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// every entry of the input raises the weight of its pair to its own (the pair's weight is the largest of its entries, either way).
// The row of input entry e is found by bisection of the offsets (validated: non-decreasing, from 0 to edges).
static __global__ void PairWeightKernel(const int *d_row_offsets, const int *d_cols, const int *d_weights, int nodes, long long edges,
                                        const int *d_ro, const int *d_ci, const int *d_eid, int *d_pw)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        int lo = 0, hi = nodes;  // first index in [0, nodes] whose offset exceeds e
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (d_row_offsets[mid] > e) hi = mid; else lo = mid + 1;
        }
        const int u = lo - 1, w = d_cols[e];
        if (u == w) continue;
        atomicMax(d_pw + d_eid[RowFind(d_ro, d_ci, u, w)], d_weights[e]);
    }
}

static __global__ void EntryWeightKernel(const int *d_eid, const int *d_pw, long long entries, int *d_ew)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < entries; i += stride) d_ew[i] = d_pw[d_eid[i]];
}

// ---------------- the contraction ----------------

// keep[v] = v represents its cluster: it is unmatched or the smaller end of its pair
static __global__ void RepFlagKernel(const int *d_mate, long long nodes, unsigned *d_keep)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int m = d_mate[v];
        d_keep[v] = (m < 0 || v < m) ? 1u : 0u;
    }
}

// map[v] = the rank of its representative; the representative adds up the cluster's vertex weights (NULL: 1 each) in 64 bits
static __global__ void MapKernel(const int *d_mate, const int *d_rank, const int *d_vw, long long nodes, int *d_map, int *d_vweight, unsigned *d_flag)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int m = d_mate[v];
        const bool rep = m < 0 || v < m;
        const int c = d_rank[rep ? v : m];
        d_map[v] = c;
        if (!rep) continue;
        long long sum = d_vw ? d_vw[v] : 1;
        if (m >= 0) sum += d_vw ? d_vw[m] : 1;
        if (sum < INT_MIN || sum > INT_MAX) {
            *d_flag = 1u;
            sum = 0;
        }
        d_vweight[c] = static_cast<int>(sum);
    }
}

// the coarse pair of a fine pair: (min << col_bits) | max of the two images, or the sentinel when they are one cluster
__device__ __forceinline__ unsigned long long CoarseKey(const int *d_map, int a, int b, int col_bits, unsigned long long sentinel)
{
    const unsigned x = static_cast<unsigned>(d_map[a]), y = static_cast<unsigned>(d_map[b]);
    if (x == y) return sentinel;
    return (static_cast<unsigned long long>(x < y ? x : y) << col_bits) | (x < y ? y : x);
}

static __global__ void CoarseKeysKernel(const int *d_src, const int *d_dst, const int *d_map, long long pairs, int col_bits,
                                        unsigned long long sentinel, unsigned long long *d_keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < pairs; e += stride)
        d_keys[e] = CoarseKey(d_map, d_src[e], d_dst[e], col_bits, sentinel);
}

// every fine pair adds its weight to its coarse pair, found by bisection of the sorted coarse keys, in 64 bits
static __global__ void CoarseWeightKernel(const int *d_src, const int *d_dst, const int *d_pw, const int *d_map, long long pairs, int col_bits,
                                          unsigned long long sentinel, const unsigned long long *d_ckeys, long long coarse_pairs,
                                          unsigned long long *d_sum)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < pairs; e += stride) {
        const unsigned long long key = CoarseKey(d_map, d_src[e], d_dst[e], col_bits, sentinel);
        if (key == sentinel) continue;
        long long lo = 0, hi = coarse_pairs;
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (d_ckeys[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < coarse_pairs) atomicAdd(d_sum + lo, static_cast<unsigned long long>(static_cast<long long>(d_pw[e])));  // (two's complement)
    }
}

// the sums must be int32: both copies of a coarse pair carry its weight
static __global__ void CoarseEntriesKernel(const int *d_eid, const unsigned long long *d_sum, long long entries, int *d_weights, unsigned *d_flag)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < entries; i += stride) {
        long long sum = static_cast<long long>(d_sum[d_eid[i]]);
        if (sum < INT_MIN || sum > INT_MAX) {
            *d_flag = 1u;
            sum = 0;
        }
        d_weights[i] = static_cast<int>(sum);
    }
}

}  // namespace matching
}  // namespace app
}  // namespace gunrock
