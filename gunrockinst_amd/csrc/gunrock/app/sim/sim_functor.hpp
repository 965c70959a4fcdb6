// app/sim/sim_functor.hpp -- device kernels of vertex similarity: pair scores and the k most similar vertices of a source.
//
// The reference snapshot has no similarity; the shape follows this tree's primitives: the neighbour CSR of graphio::PairGraph (rows
// ascending, no self-loops, no duplicates), truss's lanes-bisect-the-longer-row intersection, c4's lane / wave / workgroup / global
// balance and its open-addressed end -> count table.
//
// c(u, v) = |N(u) ^ N(v)| and the degrees are all a metric needs: every score is the fraction num / den of Fraction() below, two
// int32 (2M <= INT_MAX bounds every degree sum), widened to int64 on the way out.  Nothing here is floating point.
//
// Pair mode (PairKernel): lane l of a wave takes pair 64 g + l.  By d(u) + d(v) (PairRegime()):
//   LANE   <= lane_max: the lane merges the two sorted rows with two pointers
//   WAVE   the rest: one pair at a time by the whole wave, the lanes over the shorter row bisecting the longer, a wave sum of the hits
// u == v needs no case of its own: a row met with itself gives d(u).
//
// Top-k mode: the ends w != u of the wedges u - v - w of a source u are counted, c(u, w) each; Wd(u) = sum over v in N(u) of d(v) is the
// number of wedges (u itself among the ends) and bounds the distinct ends.  By Wd (TopkRegime()):
//   WAVE    Wd <= table_slots / 2: one source per wave, an open-addressed end -> count table in the wave's part of LDS
//   BLOCK   Wd <= block_slots / 2: one workgroup per source, the workgroup's LDS as one table
//   GLOBAL  the rest: one workgroup per source and a dense int32[n] counter row per workgroup slot in global scratch, which the walk
//           that collects the candidates clears again (its exchange hands an end to whoever clears it first)
// A table has at least 2 Wd slots, so it never fills.  With skip_neighbors the ends in row u are struck out (count 0) by a walk of that
// row.  What is left are the candidates.  Selection: a wave keeps a best list, one Entry per lane, lane i the i-th best by Better()
// (score by 64-bit cross products, then the smaller id).  Offer() merges 64 more entries into it: a bitonic sort of the 64 by shuffles,
// then the better of list[i] and new[63 - i] per lane -- the 64 best of the 128, a bitonic sequence -- and a bitonic merge.  The list
// after any sequence of offers is the set of the best of everything offered, in order: a function of the set, not of who inserted or
// claimed what first.  The waves of a workgroup merge their lists the same way through LDS (Combine()).
//
// Nothing in a launch reads what the same launch writes, apart from atomics.  No kernel waits on another workgroup and every loop bound
// is a kernel argument, a constant or a value of the build's arrays.  Every loop that holds a wave operation is wave-uniform.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/table_ladder.hpp>
#include <gunrock/oprtr/lds_table.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace sim {

enum { SIM_AUTO = 0, SIM_LANE = 1, SIM_WAVE = 2, SIM_BLOCK = 3, SIM_GLOBAL = 4 };  // "strategy"; 1 .. 4 are the regimes
static_assert(SIM_WAVE == ladder::WAVE && SIM_BLOCK == ladder::BLOCK && SIM_GLOBAL == ladder::GLOBAL, "the ladder's rungs");
enum { SIM_COMMON = 0, SIM_JACCARD = 1, SIM_OVERLAP = 2, SIM_SORENSEN = 3 };       // "metric"

constexpr int kSimThreads = 256;
constexpr int kSimWaves = kSimThreads / util::kWaveSize;
constexpr int kMaxK = 64;             // one entry of the best list per lane
constexpr int kLaneMax = 64;          // default "lane_max"  (by reasoning)
constexpr int kMaxLaneMax = 1 << 20;
constexpr int kExchangeInts = 3 * kSimThreads + kSimWaves;  // Combine()'s LDS: an Entry per thread, a candidate count per wave

// the table's options, their defaults and ranges, are the ladder's (app/table_ladder.hpp)
using ladder::kTableSlots;
using ladder::kMinTableSlots;
using ladder::kBlockSlots;
using ladder::kMinBlockSlots;
using ladder::kScratchMib;
using ladder::kMaxScratchMib;
using ladder::TableSize;

namespace lds = oprtr::lds;
using util::Fmix32;

// the 64-bit words the kernels and the host share
enum {
    W_PROBES = 0,     // table probes of the WAVE and BLOCK regimes
    W_CANDIDATES,     // candidates of all sources
    W_WALKED,         // wedges of all sources
    W_BLOCK_LIST,     // sources handed to BlockKernel
    W_GLOBAL_LIST,    // ... to GlobalKernel
    W_BAD,            // an id outside [0, nodes)
    W_PAIRS,          // two words: the pairs of the regimes LANE, WAVE
    W_SOURCES = W_PAIRS + 2,   // three words: the sources of the regimes WAVE, BLOCK, GLOBAL
    W_WEDGES = W_SOURCES + 3,  // three words: their wedges
    W_COUNT = 16
};

struct Ctx {
    const int *ro, *ci;  // the neighbour CSR of G, rows ascending
    const int *wd;       // Wd per vertex
    unsigned long long *words;
    int nodes;
    int metric, strategy, skip_neighbors, lane_max, table_slots, block_slots;
};

// what top-k mode writes: S x k each, then one per source
struct TopkOut {
    int *ids, *common;
    long long *num, *den;
    int *count, *candidates;
};

// The fraction of a metric from c = c(u, v) and the two degrees.  An isolated endpoint can make den 0: then 0 / 0.
__host__ __device__ __forceinline__ void Fraction(int metric, int c, int du, int dv, int &num, int &den)
{
    num = c;
    if (metric == SIM_COMMON) den = 1;
    else if (metric == SIM_JACCARD) den = du + dv - c;
    else if (metric == SIM_OVERLAP) den = du < dv ? du : dv;
    else {
        num = 2 * c;
        den = du + dv;
    }
    if (den == 0) num = 0;
}

// The regime of a pair: LANE while the two rows together are short and nothing larger is forced.
__host__ __device__ __forceinline__ int PairRegime(long long rows, int strategy, int lane_max)
{
    return strategy <= SIM_LANE && rows <= lane_max ? SIM_LANE : SIM_WAVE;
}

// The regime of a source with wd wedges: the smallest that holds it, not below a forced one.
__host__ __device__ __forceinline__ int TopkRegime(long long wd, int strategy, int table_slots, int block_slots)
{
    return ladder::Widen(strategy < SIM_WAVE ? SIM_WAVE : strategy, wd, table_slots, block_slots);
}

struct Tally {
    unsigned long long probes = 0, candidates = 0, walked = 0;
    unsigned pairs[2] = {0, 0}, sources[3] = {0, 0, 0};
    unsigned long long wedges[3] = {0, 0, 0};
};

// (all lanes of the wave call)
__device__ __forceinline__ void Flush(Tally &t, const Ctx &c)
{
    const unsigned long long probes = util::WaveSum(t.probes), candidates = util::WaveSum(t.candidates), walked = util::WaveSum(t.walked);
    const bool first = util::LaneId() == 0;
    if (first) {
        if (probes) atomicAdd(c.words + W_PROBES, probes);
        if (candidates) atomicAdd(c.words + W_CANDIDATES, candidates);
        if (walked) atomicAdd(c.words + W_WALKED, walked);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned pairs = util::WaveSum(t.pairs[r]);
        if (first && pairs) atomicAdd(c.words + W_PAIRS + r, static_cast<unsigned long long>(pairs));
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const unsigned sources = util::WaveSum(t.sources[r]);
        const unsigned long long wedges = util::WaveSum(t.wedges[r]);
        if (first && sources) {
            atomicAdd(c.words + W_SOURCES + r, static_cast<unsigned long long>(sources));
            atomicAdd(c.words + W_WEDGES + r, wedges);
        }
    }
    t = Tally();
}

// words[W_BAD] = 1 when a[] or b[] (b may be NULL) holds an id outside [0, nodes)
static __global__ void ValidateIdsKernel(const int *a, const int *b, long long count, int nodes, unsigned long long *words)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    bool bad = false;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        const int x = a[i], y = b ? b[i] : 0;
        bad |= x < 0 || x >= nodes || y < 0 || y >= nodes;
    }
    if (__ballot(bad) && util::LaneId() == 0) words[W_BAD] = 1ull;
}

// ---------------- pair mode ----------------

// (validated ids)
static __global__ __launch_bounds__(kSimThreads) void PairKernel(Ctx c, const int *qu, const int *qv, long long pairs, int *common, long long *num,
                                                                 long long *den)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    const long long groups = (pairs + util::kWaveSize - 1) / util::kWaveSize;
    Tally t;
    for (long long g = wave0; g < groups; g += nwaves) {  // (wave-uniform)
        const long long at = g * util::kWaveSize + lane;
        const bool live = at < pairs;
        int bu = 0, du = 0, bv = 0, dv = 0, regime = 0, hits = 0;
        if (live) {
            const int u = qu[at], v = qv[at];
            bu = c.ro[u];
            du = c.ro[u + 1] - bu;
            bv = c.ro[v];
            dv = c.ro[v + 1] - bv;
            regime = PairRegime(static_cast<long long>(du) + dv, c.strategy, c.lane_max);
            ++t.pairs[regime - 1];
        }
        if (regime == SIM_LANE) {
            int i = bu, j = bv;
            const int eu = bu + du, ev = bv + dv;
            while (i < eu && j < ev) {
                const int a = c.ci[i], b = c.ci[j];
                hits += a == b;
                i += a <= b;
                j += b <= a;
            }
        }
        unsigned long long todo = __ballot(regime == SIM_WAVE);
        while (todo) {  // (wave-uniform)
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lbu = __shfl(bu, leader, util::kWaveSize), ldu = __shfl(du, leader, util::kWaveSize);
            const int lbv = __shfl(bv, leader, util::kWaveSize), ldv = __shfl(dv, leader, util::kWaveSize);
            const bool u_short = ldu <= ldv;
            const int bs = u_short ? lbu : lbv, ds = u_short ? ldu : ldv, bl = u_short ? lbv : lbu, dl = u_short ? ldv : ldu;
            int found = 0;
            for (int i = lane; i < ds; i += util::kWaveSize) {
                const int x = c.ci[bs + i];
                int lo = 0, hi = dl;  // first entry of the longer row that is >= x
                while (lo < hi) {
                    const int mid = lo + (hi - lo) / 2;
                    if (c.ci[bl + mid] < x) lo = mid + 1; else hi = mid;
                }
                found += lo < dl && c.ci[bl + lo] == x;
            }
            found = util::WaveSum(found);
            if (lane == leader) hits = found;
            todo &= todo - 1;
        }
        if (live) {
            int n = 0, d = 0;
            Fraction(c.metric, hits, du, dv, n, d);
            common[at] = hits;
            num[at] = n;
            den[at] = d;
        }
    }
    Flush(t, c);
}

// ---------------- the best list ----------------

struct Entry {
    int num, den, id;
};

// below every candidate (a candidate has num >= 1 and den >= 1)
__device__ __forceinline__ Entry Empty() { return Entry{-1, 1, 0x7FFFFFFF}; }

// a ranks before b: the larger fraction by cross products (each below 2^62), then the smaller id.  Strict: two equal entries are two
// Empty() ones.
__device__ __forceinline__ bool Better(const Entry &a, const Entry &b)
{
    const long long l = static_cast<long long>(a.num) * b.den, r = static_cast<long long>(b.num) * a.den;
    return l > r || (l == r && a.id < b.id);
}

__device__ __forceinline__ Entry ShflEntry(const Entry &e, int from)
{
    return Entry{__shfl(e.num, from, util::kWaveSize), __shfl(e.den, from, util::kWaveSize), __shfl(e.id, from, util::kWaveSize)};
}

// the wave's 64 entries in order, lane 0 the best: a bitonic sort
__device__ __forceinline__ void SortBest(Entry &e, int lane)
{
#pragma unroll
    for (int k = 2; k <= util::kWaveSize; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const Entry o = ShflEntry(e, lane ^ j);
            const bool keep_better = ((lane & k) == 0) == ((lane & j) == 0);  // the lower lane of a best-first run, the upper of a worst-first
            if (keep_better ? Better(o, e) : Better(e, o)) e = o;
        }
    }
}

// a bitonic sequence over the lanes into order, lane 0 the best
__device__ __forceinline__ void MergeBest(Entry &e, int lane)
{
#pragma unroll
    for (int j = util::kWaveSize / 2; j > 0; j >>= 1) {
        const Entry o = ShflEntry(e, lane ^ j);
        if ((lane & j) == 0 ? Better(o, e) : Better(e, o)) e = o;
    }
}

// `sorted` (lane 0 the best) into the list: afterwards the list holds the 64 best of both, in order
__device__ __forceinline__ void MergeLists(Entry &best, const Entry &reversed, int lane)
{
    if (Better(reversed, best)) best = reversed;
    MergeBest(best, lane);
}

// All lanes of the wave call.  The entries with `valid` join the list; one that does not beat the k-th of the list cannot be among
// the k best and is dropped first (the list behind its k-th place is not used).
__device__ __forceinline__ void Offer(Entry &best, Entry cand, bool valid, int k, int lane)
{
    const Entry kth = ShflEntry(best, k - 1);
    valid = valid && Better(cand, kth);
    if (!__ballot(valid)) return;
    if (!valid) cand = Empty();
    SortBest(cand, lane);
    MergeLists(best, ShflEntry(cand, util::kWaveSize - 1 - lane), lane);
}

__device__ __forceinline__ Entry MakeEntry(const Ctx &c, int du, int w, int count)
{
    Entry e;
    e.id = w;
    Fraction(c.metric, count, du, c.ro[w + 1] - c.ro[w], e.num, e.den);
    return e;
}

// The lists and candidate counts of the workgroup's waves into wave 0's (all threads call; xch: kExchangeInts of LDS nobody else
// uses between the barriers here).
__device__ __forceinline__ void Combine(Entry &best, int &candidates, int *xch)
{
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    __syncthreads();
    int *mine = xch + 3 * static_cast<int>(threadIdx.x);
    mine[0] = best.num;
    mine[1] = best.den;
    mine[2] = best.id;
    if (lane == 0) xch[3 * kSimThreads + wave] = candidates;
    __syncthreads();
    if (wave == 0) {
        candidates = 0;
#pragma unroll
        for (int w = 0; w < kSimWaves; ++w) candidates += xch[3 * kSimThreads + w];
#pragma unroll
        for (int w = 1; w < kSimWaves; ++w) {  // (uniform over the wave)
            const int *theirs = xch + 3 * (w * util::kWaveSize + util::kWaveSize - 1 - lane);
            MergeLists(best, Entry{theirs[0], theirs[1], theirs[2]}, lane);
        }
    }
    __syncthreads();
}

// row s of the result from the wave's list (all lanes of the wave call)
__device__ __forceinline__ void WriteRow(const Ctx &c, const TopkOut &o, int s, int k, const Entry &best, int candidates)
{
    const int lane = static_cast<int>(util::LaneId());
    if (lane < k) {
        const size_t at = static_cast<size_t>(s) * static_cast<size_t>(k) + static_cast<size_t>(lane);
        const bool there = best.num > 0;
        o.ids[at] = there ? best.id : -1;
        o.common[at] = there ? (c.metric == SIM_SORENSEN ? best.num / 2 : best.num) : 0;
        o.num[at] = there ? best.num : 0;
        o.den[at] = there ? best.den : 0;
    }
    if (lane == 0) {
        o.count[s] = candidates < k ? candidates : k;
        o.candidates[s] = candidates;
    }
}

// ---------------- top-k mode: WAVE and BLOCK ----------------

// The best of source u, by a wave (BLOCK = false) or by the workgroup (BLOCK = true; then each wave has the best of its part of the
// table and its number of candidates: Combine() follows).  key[] / count[] are the group's table of `slots` slots.
template <bool BLOCK>
__device__ __forceinline__ void TableBest(const Ctx &c, int u, int k, int *key, int *count, int slots, Tally &t, Entry &best, int &candidates)
{
    constexpr int G = BLOCK ? kSimThreads : util::kWaveSize;
    constexpr int WAVES = BLOCK ? kSimWaves : 1;
    const int tid = BLOCK ? static_cast<int>(threadIdx.x) : static_cast<int>(util::LaneId());
    const int lane = static_cast<int>(util::LaneId());
    const int wave = BLOCK ? static_cast<int>(threadIdx.x) / util::kWaveSize : 0;
    const int size = TableSize(c.wd[u], slots);  // (a multiple of 64)
    const int b = c.ro[u], d = c.ro[u + 1] - b;
    lds::Clear<G>(key, size, tid, [&](int s) { count[s] = 0; });
    lds::GroupSync<BLOCK>();
    for (int i = b + wave; i < b + d; i += WAVES) {  // the count: a wave takes one v at a time and its lanes the w of that v
        const int v = c.ci[i], rv = c.ro[v], dv = c.ro[v + 1] - rv;
        for (int j = lane; j < dv; j += util::kWaveSize) {
            const int w = c.ci[rv + j];
            if (w == u) continue;
            const int at = lds::Claim(key, size, Fmix32(static_cast<unsigned>(w)), w, t.probes);
            if (at >= 0) atomicAdd(count + at, 1);  // (always: the table never fills)
        }
    }
    lds::GroupSync<BLOCK>();
    if (c.skip_neighbors) {  // (uniform) the ends in row u are no candidates
        for (int i = tid; i < d; i += G) {
            const int v = c.ci[b + i];
            const int at = lds::Find(key, size, Fmix32(static_cast<unsigned>(v)), v, t.probes);
            if (at >= 0) count[at] = 0;
        }
        lds::GroupSync<BLOCK>();
    }
    best = Empty();
    candidates = 0;
    for (int base = wave * util::kWaveSize; base < size; base += WAVES * util::kWaveSize) {  // (wave-uniform) every end once
        const int w = key[base + lane], same = count[base + lane];
        const bool valid = w >= 0 && same > 0;
        candidates += valid;
        Offer(best, valid ? MakeEntry(c, d, w, same) : Empty(), valid, k, lane);
    }
    candidates = util::WaveSum(candidates);
    if (!BLOCK) lds::WaveLdsSync();  // (the next source clears what this one still reads; a workgroup's Combine() has the barrier)
}

// the source of row s enters a regime's tallies, by one thread
__device__ __forceinline__ void Count(Tally &t, int regime, int wd)
{
    ++t.sources[regime - SIM_WAVE];
    t.wedges[regime - SIM_WAVE] += static_cast<unsigned long long>(wd);
    t.walked += static_cast<unsigned long long>(wd);
}

// One wave per source row: WAVE sources by the wave, the others into the lists of the kernels below.
static __global__ __launch_bounds__(kSimThreads) void SmallKernel(Ctx c, TopkOut o, const int *sources, int rows, int k, int *block_list,
                                                                  int *global_list)
{
    extern __shared__ int s_table[];  // kSimWaves * table_slots keys, then as many counts
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    int *key = s_table + static_cast<size_t>(wave) * c.table_slots;
    int *count = s_table + static_cast<size_t>(kSimWaves + wave) * c.table_slots;
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    for (long long s = wave0; s < rows; s += nwaves) {  // (wave-uniform)
        const int u = sources[s], wd = c.wd[u];
        const int regime = TopkRegime(wd, c.strategy, c.table_slots, c.block_slots);
        if (lane == 0) Count(t, regime, wd);
        if (regime == SIM_WAVE) {
            Entry best;
            int candidates;
            TableBest<false>(c, u, k, key, count, c.table_slots, t, best, candidates);
            if (lane == 0) t.candidates += static_cast<unsigned long long>(candidates);
            WriteRow(c, o, static_cast<int>(s), k, best, candidates);
        } else if (lane == 0) {  // (a row enters a list once, so a position stays under `rows`; the test keeps a mistake inside the array)
            const unsigned long long pos = atomicAdd(c.words + (regime == SIM_BLOCK ? W_BLOCK_LIST : W_GLOBAL_LIST), 1ull);
            if (pos < static_cast<unsigned long long>(rows)) (regime == SIM_BLOCK ? block_list : global_list)[pos] = static_cast<int>(s);
        }
    }
    Flush(t, c);
}

// One workgroup per row of block_list[]; W_BLOCK_LIST is what SmallKernel left (a kernel boundary lies between).
static __global__ __launch_bounds__(kSimThreads) void BlockKernel(Ctx c, TopkOut o, const int *sources, int rows, int k, const int *block_list)
{
    extern __shared__ int s_table[];  // block_slots keys, then as many counts; at least kExchangeInts
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    long long listed = static_cast<long long>(c.words[W_BLOCK_LIST]);
    if (listed > rows) listed = rows;
    Tally t;
    for (long long i = blockIdx.x; i < listed; i += gridDim.x) {  // (uniform over the workgroup)
        const int s = block_list[i];
        Entry best;
        int candidates;
        TableBest<true>(c, sources[s], k, s_table, s_table + c.block_slots, c.block_slots, t, best, candidates);
        Combine(best, candidates, s_table);  // (the table is read no more)
        if (wave == 0) {
            if (threadIdx.x == 0) t.candidates += static_cast<unsigned long long>(candidates);
            WriteRow(c, o, s, k, best, candidates);
        }
    }
    Flush(t, c);
}

// ---------------- top-k mode: GLOBAL ----------------

// One workgroup per row of global_list[], workgroup slot blockIdx.x with its counter row rows_[blockIdx.x * nodes ..), all 0 between two
// sources.  The host launches no more workgroups than there are counter rows.
static __global__ __launch_bounds__(kSimThreads) void GlobalKernel(Ctx c, TopkOut o, const int *sources, int rows, int k, const int *global_list,
                                                                   int *counters)
{
    __shared__ int s_xch[kExchangeInts];
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    int *row = counters + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(c.nodes);
    long long listed = static_cast<long long>(c.words[W_GLOBAL_LIST]);
    if (listed > rows) listed = rows;
    Tally t;
    for (long long at = blockIdx.x; at < listed; at += gridDim.x) {  // (uniform over the workgroup)
        const int s = global_list[at], u = sources[s];
        const int b = c.ro[u], d = c.ro[u + 1] - b;
        for (int i = b + wave; i < b + d; i += kSimWaves) {  // the count
            const int v = c.ci[i], rv = c.ro[v], dv = c.ro[v + 1] - rv;
            for (int j = lane; j < dv; j += util::kWaveSize) {
                const int w = c.ci[rv + j];
                if (w != u) atomicAdd(row + w, 1);
            }
        }
        lds::GlobalSync();
        if (c.skip_neighbors) {  // (uniform)
            for (int i = static_cast<int>(threadIdx.x); i < d; i += kSimThreads) atomicExch(row + c.ci[b + i], 0);
            lds::GlobalSync();
        }
        Entry best = Empty();
        int candidates = 0;
        for (int i = b + wave; i < b + d; i += kSimWaves) {  // the row back to 0; who clears an end offers it
            const int v = c.ci[i], rv = c.ro[v], dv = c.ro[v + 1] - rv;
            for (int j0 = 0; j0 < dv; j0 += util::kWaveSize) {  // (wave-uniform)
                const int j = j0 + lane;
                const int w = j < dv ? c.ci[rv + j] : u;
                const int same = w != u ? atomicExch(row + w, 0) : 0;
                const bool valid = same > 0;
                candidates += valid;
                Offer(best, valid ? MakeEntry(c, d, w, same) : Empty(), valid, k, lane);
            }
        }
        candidates = util::WaveSum(candidates);
        Combine(best, candidates, s_xch);
        if (wave == 0) {
            if (threadIdx.x == 0) t.candidates += static_cast<unsigned long long>(candidates);
            WriteRow(c, o, s, k, best, candidates);
        }
        lds::GlobalSync();  // (the next source counts in the row this one cleared)
    }
    Flush(t, c);
}

// ---------------- the build ----------------

// wd[u] = the sum of d(v) over row u, one wave per vertex at a time; summary[0] = the sum of wd, summary[1] = the largest
static __global__ __launch_bounds__(kSimThreads) void WedgeKernel(const int *ro, const int *ci, int nodes, int *wd, unsigned long long *summary)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    unsigned long long sum = 0, longest = 0;
    for (long long u = wave0; u < nodes; u += nwaves) {  // (wave-uniform)
        const int b = ro[u], e = ro[u + 1];
        int w = 0;
        for (int i = b + lane; i < e; i += util::kWaveSize) {
            const int v = ci[i];
            w += ro[v + 1] - ro[v];
        }
        w = util::WaveSum(w);
        if (lane == 0) wd[u] = w;
        sum += static_cast<unsigned long long>(w);
        longest = static_cast<unsigned long long>(w) > longest ? static_cast<unsigned long long>(w) : longest;
    }
    if (lane == 0 && sum) {  // (sum and longest are uniform over the wave)
        atomicAdd(summary, sum);
        atomicMax(summary + 1, longest);
    }
}

}  // namespace sim
}  // namespace app
}  // namespace gunrock
