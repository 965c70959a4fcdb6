// app/lp/lp_functor.hpp -- device kernels of label propagation: the weighted vote of a vertex over its neighbours' labels.
//
// The reference snapshot has no label propagation; the shape follows this tree's primitives: matching's neighbour CSR over the
// canonical pairs, its lane / wave row balance and its next list with one ticket per wave (mis_functor.hpp is included for the hash).
//
// Row v of the neighbour CSR holds the distinct neighbours of v ascending and ew[i] the weight of entry i (NULL: 1 each, every weight
// is at least 1).  The vote of v:  score(l) = sum of ew[i] over the entries with L[ci[i]] == l, as a 64-bit sum;  best = max score;
// the new label is L[v] when score(L[v]) == best, else the smallest l with score(l) == best.  That is the maximum of the candidates
// (score, label) under the total order (score desc, label == L[v] first, label asc), so partial maxima can be merged in any order.
//
// A row is voted in one of three regimes, chosen by its length d (Regime()):
//   LANE   d <= lane_max_row: one row per lane, a compare loop over the row in registers, no table
//   WAVE   d <= wave_max_row: one row per wave, an open-addressed label -> score table in the wave's part of LDS; the lanes add
//          their entries' weights with LDS atomics (64-bit integer sums: the order does not matter), then every lane scans its share
//          of the slots and a wave reduction picks the maximum
//   BLOCK  longer rows: one workgroup per row, the whole workgroup's LDS as one table, the same steps with workgroup barriers
// A table takes min(its slots, 2 d rounded up to a power of two) slots, at least 64.  A row with more distinct labels than the table
// holds is still exact and needs no global scratch: the row is passed over once per slice of the hash space, a pass counts only the
// labels whose hash falls into its slice, and the running maximum is carried over the passes.  A pass that fills its table sets a
// flag, and the row starts again with twice as many slices; Fmix32 is a bijection, so 2^26 slices hold at most 64 labels each and
// the doubling ends there at the latest (kMaxLogSlices).
//
// Nothing in a launch reads what the same launch writes.  SYNC: VoteKernel reads L[] and writes fresh[] of its own vertex,
// ApplyKernel moves fresh[] into L[] and lists the neighbours of what changed.  CLASSES: a launch holds one class, an independent set,
// so the L[] of a neighbour is never written by the launch that reads it; the kernel boundary publishes a sub-step.  No kernel waits
// on another workgroup and every loop bound is a kernel argument or a constant.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include <gunrock/oprtr/lds_table.hpp>
#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace lp {

enum { LP_SYNC = 0, LP_CLASSES = 1 };                                // "mode"
enum { LP_AUTO = 0, LP_LANE = 1, LP_WAVE = 2, LP_BLOCK = 3 };        // "strategy"
enum { LP_CONVERGED = 0, LP_PERIOD2 = 1, LP_CAPPED = 2 };            // how an Enact ended

constexpr int kLpThreads = 256;
constexpr int kLpWaves = kLpThreads / util::kWaveSize;
constexpr int kLaneMaxRow = 16;     // default "lane_max_row"  (by reasoning)
constexpr int kWaveMaxRow = 512;    // default "wave_max_row"
constexpr int kTableSlots = 1024;   // default and largest "table_slots": 12 KiB per wave, 48 KiB per workgroup
using oprtr::lds::kMinTableSlots;
constexpr int kMaxLogSlices = 26;   // 2^26 slices of the 32-bit hash space hold 64 labels each

namespace lds = oprtr::lds;
using util::Fmix32;

// the 64-bit words the kernels and the host share; the first kRoundWords are cleared in front of every round
enum {
    W_NEXT = 0,   // vertices in the next list (SYNC)
    W_HUBS,       // rows handed to HubKernel by the last VoteKernel
    W_CHANGED,    // labels changed in this round
    W_RETURNED,   // ... of them back at their value of two rounds ago (SYNC)
    kRoundWords,
    W_VISITS = kRoundWords,  // since Reset
    W_ENTRIES,
    W_REGIME,  // three words
    W_FALLBACK = W_REGIME + 3,
    W_FLAG,    // validation: a weight below 1, a pair inside a class
    W_COMMUNITIES,
    W_COUNT = 16
};

struct Ctx {
    const int *ro, *ci, *ew;  // the neighbour CSR and the weight of every entry (or NULL)
    int *labels, *fresh;      // L[]; SYNC: the vote's result until ApplyKernel takes it
    int *prev, *chround;      // SYNC: the label before the last change and the round of that change
    int *dirty;               // a neighbour changed since the last visit (or no visit yet)
    int *hubs;                // the rows VoteKernel leaves to HubKernel
    unsigned long long *words;
    int nodes;
    int strategy, lane_max_row, wave_max_row;
    int table_slots;          // per wave; a workgroup's table has kLpWaves times as many
};

struct Cand {
    unsigned long long score = 0;  // (every real candidate has a score of at least 1)
    int label = INT_MAX;
};

// a before b in (score desc, is-current, label asc)
__device__ __forceinline__ bool Better(const Cand &a, const Cand &b, int cur)
{
    if (a.score != b.score) return a.score > b.score;
    const bool ac = a.label == cur, bc = b.label == cur;
    if (ac != bc) return ac;
    return a.label < b.label;
}

__device__ __forceinline__ Cand WaveBest(Cand c, int cur)
{
#pragma unroll
    for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) {
        Cand o;
        o.score = __shfl_xor(c.score, d, util::kWaveSize);
        o.label = __shfl_xor(c.label, d, util::kWaveSize);
        if (Better(o, c, cur)) c = o;
    }
    return c;
}

__host__ __device__ __forceinline__ int Regime(int d, int strategy, int lane_max_row, int wave_max_row)
{
    if (strategy != LP_AUTO) return strategy;
    return d <= lane_max_row ? LP_LANE : (d <= wave_max_row ? LP_WAVE : LP_BLOCK);
}

struct Tally {
    unsigned visits = 0, changed = 0, returned = 0, fallback = 0;
    unsigned lane_rows = 0, wave_rows = 0, block_rows = 0;
    unsigned long long entries = 0;
};

__device__ __forceinline__ void Flush(Tally &t, const Ctx &c)
{
    const unsigned visits = util::WaveSum(t.visits), changed = util::WaveSum(t.changed), returned = util::WaveSum(t.returned);
    const unsigned fallback = util::WaveSum(t.fallback);
    const unsigned r0 = util::WaveSum(t.lane_rows), r1 = util::WaveSum(t.wave_rows), r2 = util::WaveSum(t.block_rows);
    const unsigned long long entries = util::WaveSum(t.entries);
    if (util::LaneId() == 0) {
        if (visits) atomicAdd(c.words + W_VISITS, static_cast<unsigned long long>(visits));
        if (entries) atomicAdd(c.words + W_ENTRIES, entries);
        if (changed) atomicAdd(c.words + W_CHANGED, static_cast<unsigned long long>(changed));
        if (returned) atomicAdd(c.words + W_RETURNED, static_cast<unsigned long long>(returned));
        if (fallback) atomicAdd(c.words + W_FALLBACK, static_cast<unsigned long long>(fallback));
        if (r0) atomicAdd(c.words + W_REGIME + 0, static_cast<unsigned long long>(r0));
        if (r1) atomicAdd(c.words + W_REGIME + 1, static_cast<unsigned long long>(r1));
        if (r2) atomicAdd(c.words + W_REGIME + 2, static_cast<unsigned long long>(r2));
    }
    t = Tally();
}

// All lanes of the wave call; the lanes with `hit` append v to list[] through words[word]: one atomic per wave.  A vertex enters a
// list once, so a position stays under `nodes`; the test keeps a mistake elsewhere from turning into a store outside the array.
__device__ __forceinline__ void Append(const Ctx &c, int word, int *list, bool hit, int v)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned long long pos = oprtr::WaveTicket(c.words + word, mask);
    if (hit) {
        if (pos < static_cast<unsigned long long>(c.nodes)) list[pos] = v;
    }
}

// ---------------- the vote ----------------

// LANE: every label of the row at its first entry, its score summed over the rest of the row
__device__ __forceinline__ int LaneVote(const Ctx &c, int b, int e, int cur)
{
    Cand best;
    for (int i = b; i < e; ++i) {
        const int l = c.labels[c.ci[i]];
        bool seen = false;
        for (int j = b; j < i && !seen; ++j) seen = c.labels[c.ci[j]] == l;
        if (seen) continue;
        Cand x;
        x.label = l;
        for (int j = i; j < e; ++j)
            if (c.labels[c.ci[j]] == l) x.score += static_cast<unsigned long long>(c.ew ? c.ew[j] : 1);
        if (Better(x, best, cur)) best = x;
    }
    return best.label;
}

// what a workgroup shares next to its table (HubKernel)
struct BlockShared {
    unsigned long long score[kLpWaves];
    int label[kLpWaves];
    int full;
};

// The vote of row [b, e) by a wave (tid = the lane) or by the workgroup (tid = threadIdx.x), uniform over the group: the new label.
// key[] / score[] are the group's table of `slots` slots (a power of two).  *fell: the row needed more than one slice.
template <bool BLOCK>
__device__ __forceinline__ int RowVote(const Ctx &c, int b, int e, int cur, int *key, unsigned long long *score, int slots, BlockShared *sh,
                                       bool *fell)
{
    constexpr int G = BLOCK ? kLpThreads : util::kWaveSize;
    const int tid = BLOCK ? static_cast<int>(threadIdx.x) : static_cast<int>(util::LaneId());
    const int size = lds::TableSize(e - b, slots);
    Cand best;
    int log_slices = 0;
    for (;;) {  // (at most kMaxLogSlices + 1 times)
        best = Cand();
        bool full = false;
        const unsigned slices = 1u << log_slices;
        for (unsigned s = 0; s < slices; ++s) {
            lds::Clear<G>(key, size, tid, [&](int k) { score[k] = 0; });
            lds::GroupSync<BLOCK>();
            for (int i = b + tid; i < e; i += G) {
                const int l = c.labels[c.ci[i]];
                const unsigned h = Fmix32(static_cast<unsigned>(l));
                if (log_slices && (h >> (32 - log_slices)) != s) continue;
                unsigned long long probes = 0;  // (not counted here)
                const int at = lds::Claim(key, size, h, l, probes);
                if (at >= 0) atomicAdd(score + at, static_cast<unsigned long long>(c.ew ? c.ew[i] : 1));
                full |= at < 0;
            }
            lds::GroupSync<BLOCK>();
            for (int k = tid; k < size; k += G) {
                Cand x;
                x.label = key[k];
                x.score = score[k];
                if (x.label >= 0 && Better(x, best, cur)) best = x;
            }
            lds::GroupSync<BLOCK>();  // (the next pass clears what this one still reads)
        }
        // did any pass fill its table?
        bool any;
        if (BLOCK) {
            if (tid == 0) sh->full = 0;
            __syncthreads();
            if (full) sh->full = 1;
            __syncthreads();
            any = sh->full != 0;
            __syncthreads();
        } else {
            any = __ballot(full) != 0;
        }
        if (!any || log_slices >= kMaxLogSlices) break;
        ++log_slices;
    }
    *fell = log_slices > 0;
    best = WaveBest(best, cur);
    if (BLOCK) {
        const int wave = tid / util::kWaveSize;
        if (util::LaneId() == 0) {
            sh->score[wave] = best.score;
            sh->label[wave] = best.label;
        }
        __syncthreads();
        best = Cand();
#pragma unroll
        for (int w = 0; w < kLpWaves; ++w) {
            Cand x;
            x.score = sh->score[w];
            x.label = sh->label[w];
            if (Better(x, best, cur)) best = x;
        }
        __syncthreads();
    }
    return best.label;
}

// One wave per 64 list entries.  SYNC: the list is the round's active list.  CLASSES: the list is a class and a vertex takes its turn
// when it is dirty.  LANE rows by their lane, WAVE rows one after the other by the whole wave, BLOCK rows into hubs[] for HubKernel.
// Every loop that holds a wave operation is wave-uniform.
template <bool SYNC>
static __global__ __launch_bounds__(kLpThreads) void VoteKernel(Ctx c, const int *list, long long count)
{
    extern __shared__ unsigned long long s_table[];  // kLpWaves * table_slots scores, then as many keys
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    unsigned long long *score = s_table + static_cast<size_t>(wave) * c.table_slots;
    int *key = reinterpret_cast<int *>(s_table + static_cast<size_t>(kLpWaves) * c.table_slots) + static_cast<size_t>(wave) * c.table_slots;
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    if (count > c.nodes) count = c.nodes;
    Tally t;
    for (long long from = wave0 * util::kWaveSize; from < count; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = from + lane;
        int v = i < count ? list[i] : -1;
        if (!SYNC && v >= 0 && !c.dirty[v]) v = -1;
        int b = 0, e = 0, cur = 0, regime = 0;
        if (v >= 0) {
            c.dirty[v] = 0;
            b = c.ro[v];
            e = c.ro[v + 1];
            cur = c.labels[v];
            ++t.visits;
            t.entries += static_cast<unsigned long long>(e - b);
            if (e > b) {
                regime = Regime(e - b, c.strategy, c.lane_max_row, c.wave_max_row);
                t.lane_rows += regime == LP_LANE;
                t.wave_rows += regime == LP_WAVE;
                t.block_rows += regime == LP_BLOCK;
            }
        }
        int nl = cur;
        if (regime == LP_LANE) nl = LaneVote(c, b, e, cur);
        unsigned long long todo = __ballot(regime == LP_WAVE);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
            const int lcur = __shfl(cur, leader, util::kWaveSize);
            bool fell = false;
            const int got = RowVote<false>(c, lb, le, lcur, key, score, c.table_slots, nullptr, &fell);
            if (lane == leader) {
                nl = got;
                if (fell) ++t.fallback;
            }
            if (!SYNC && got != lcur)  // the whole wave tells the row's neighbours
                for (int k = lb + lane; k < le; k += util::kWaveSize) c.dirty[c.ci[k]] = 1;
            todo &= todo - 1;
        }
        Append(c, W_HUBS, c.hubs, regime == LP_BLOCK, v);
        if (v < 0 || regime == LP_BLOCK) continue;
        if (SYNC) {
            c.fresh[v] = nl;
        } else if (nl != cur) {
            c.labels[v] = nl;
            ++t.changed;
            if (regime == LP_LANE)
                for (int k = b; k < e; ++k) c.dirty[c.ci[k]] = 1;
        }
    }
    Flush(t, c);
}

// One workgroup per row of hubs[]; W_HUBS is what the VoteKernel in front left (a kernel boundary lies between), `bound` its upper
// bound from the host: the length of that kernel's list.
template <bool SYNC>
static __global__ __launch_bounds__(kLpThreads) void HubKernel(Ctx c, long long bound)
{
    extern __shared__ unsigned long long s_table[];
    __shared__ BlockShared sh;
    const int slots = kLpWaves * c.table_slots;
    unsigned long long *score = s_table;
    int *key = reinterpret_cast<int *>(s_table + slots);
    long long hubs = static_cast<long long>(c.words[W_HUBS]);
    if (hubs > bound) hubs = bound;
    if (hubs > c.nodes) hubs = c.nodes;
    Tally t;
    for (long long i = blockIdx.x; i < hubs; i += gridDim.x) {  // (uniform over the workgroup)
        const int v = c.hubs[i];
        const int b = c.ro[v], e = c.ro[v + 1], cur = c.labels[v];
        bool fell = false;
        const int nl = RowVote<true>(c, b, e, cur, key, score, slots, &sh, &fell);
        if (threadIdx.x == 0 && fell) ++t.fallback;
        if (SYNC) {
            if (threadIdx.x == 0) c.fresh[v] = nl;
        } else if (nl != cur) {
            if (threadIdx.x == 0) {
                c.labels[v] = nl;
                ++t.changed;
            }
            for (int k = b + static_cast<int>(threadIdx.x); k < e; k += kLpThreads) c.dirty[c.ci[k]] = 1;
        }
    }
    Flush(t, c);
}

// the first to make u dirty lists it
__device__ __forceinline__ bool Claim(const Ctx &c, int u) { return atomicExch(c.dirty + u, 1) == 0; }

// SYNC, behind the votes of round `round`: L[v] = fresh[v] for the round's list; a vertex that changed notes where it came from and
// lists every neighbour that is not listed yet (dirty[] is the claim).  Rows up to lane_max_row by their lane, in a loop as long as
// the wave's longest; the others by the whole wave.
static __global__ __launch_bounds__(kLpThreads) void ApplyKernel(Ctx c, const int *list, long long count, int *next, int round)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    if (count > c.nodes) count = c.nodes;
    Tally t;
    for (long long from = wave0 * util::kWaveSize; from < count; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = from + lane;
        const int v = i < count ? list[i] : -1;
        int b = 0, e = 0;
        if (v >= 0) {
            const int nl = c.fresh[v], cur = c.labels[v];
            if (nl != cur) {
                if (c.chround[v] == round - 1 && c.prev[v] == nl) ++t.returned;
                c.prev[v] = cur;
                c.chround[v] = round;
                c.labels[v] = nl;
                ++t.changed;
                b = c.ro[v];
                e = c.ro[v + 1];
            }
        }
        const bool wide = e - b > c.lane_max_row;
        int longest = wide ? 0 : e - b;
#pragma unroll
        for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) {
            const int o = __shfl_xor(longest, d, util::kWaveSize);
            longest = o > longest ? o : longest;
        }
        for (int k = 0; k < longest; ++k) {
            int u = -1;
            if (!wide && b + k < e) u = c.ci[b + k];
            Append(c, W_NEXT, next, u >= 0 && Claim(c, u), u);
        }
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
            for (int base = lb; base < le; base += util::kWaveSize) {
                const int k = base + lane;
                const int u = k < le ? c.ci[k] : -1;
                Append(c, W_NEXT, next, u >= 0 && Claim(c, u), u);
            }
            todo &= todo - 1;
        }
    }
    Flush(t, c);
}

// ---------------- reset, classes, results ----------------

// every vertex at its start label (NULL: its id), dirty, never changed, and in the first list
static __global__ void ResetKernel(Ctx c, const int *start, int *list)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < c.nodes; v += stride) {
        c.labels[v] = start ? start[v] : static_cast<int>(v);
        c.dirty[v] = 1;
        c.prev[v] = c.chround[v] = -1;
        list[v] = static_cast<int>(v);
    }
}

// a pair weight below 1 is refused
static __global__ void MinWeightKernel(const int *d_pw, long long pairs, unsigned long long *d_flag)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    bool bad = false;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < pairs; e += stride) bad |= d_pw[e] < 1;
    if (__ballot(bad) && util::LaneId() == 0) *d_flag = 1ull;
}

// the longest row: whether any row can reach the BLOCK regime
static __global__ void LongestRowKernel(const int *d_ro, long long nodes, unsigned long long *d_longest)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    int longest = 0;
    for (long long r = 0; r < rounds; ++r, v += stride)  // (wave-uniform)
        if (v < nodes && d_ro[v + 1] - d_ro[v] > longest) longest = d_ro[v + 1] - d_ro[v];
#pragma unroll
    for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) {
        const int o = __shfl_xor(longest, d, util::kWaveSize);
        longest = o > longest ? o : longest;
    }
    if (util::LaneId() == 0 && longest) atomicMax(d_longest, static_cast<unsigned long long>(longest));
}

// a pair inside one class is refused
static __global__ void ClassCheckKernel(const int *d_src, const int *d_dst, const int *d_class, long long pairs, unsigned long long *d_flag)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    bool bad = false;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < pairs; e += stride)
        bad |= d_class[d_src[e]] == d_class[d_dst[e]];
    if (__ballot(bad) && util::LaneId() == 0) *d_flag = 1ull;
}

// (class << col_bits) | v: sorted, the vertices grouped by class, ascending inside one; the longest row of every class on the way
static __global__ void ClassKeysKernel(const int *d_class, const int *d_ro, long long nodes, int col_bits, unsigned long long *d_keys, int *d_longest)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        d_keys[v] = (static_cast<unsigned long long>(d_class[v]) << col_bits) | static_cast<unsigned long long>(v);
        atomicMax(d_longest + d_class[v], d_ro[v + 1] - d_ro[v]);
    }
}

// list[i] = the vertex of sorted key i; off[k] = the first key of class k, for k = 0 .. classes
static __global__ void ClassListKernel(const unsigned long long *d_keys, long long nodes, int classes, int col_bits, int *d_list, int *d_off)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    const long long count = nodes > classes + 1 ? nodes : classes + 1;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (i < nodes) d_list[i] = static_cast<int>(d_keys[i] & mask);
        if (i <= classes) {
            const unsigned long long x = static_cast<unsigned long long>(i) << col_bits;
            long long lo = 0, hi = nodes;
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (d_keys[mid] < x) lo = mid + 1; else hi = mid;
            }
            d_off[i] = static_cast<int>(lo);
        }
    }
}

static __global__ void UsedKernel(const int *d_labels, long long nodes, unsigned *d_used)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) d_used[d_labels[v]] = 1u;
}

// community[v] = the rank of L[v] among the labels in use
static __global__ void CommunityKernel(const int *d_labels, const int *d_rank, long long nodes, int *d_community)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) d_community[v] = d_rank[d_labels[v]];
}

// size[] and volume[] (the weighted degrees) per community
static __global__ void SizeVolumeKernel(const int *d_community, const int *d_ro, const int *d_ew, long long nodes, unsigned long long *d_size,
                                        unsigned long long *d_volume)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        unsigned long long sum = 0;
        if (d_ew)
            for (int i = d_ro[v]; i < d_ro[v + 1]; ++i) sum += static_cast<unsigned long long>(d_ew[i]);
        else
            sum = static_cast<unsigned long long>(d_ro[v + 1] - d_ro[v]);
        atomicAdd(d_size + d_community[v], 1ull);
        if (sum) atomicAdd(d_volume + d_community[v], sum);
    }
}

// internal[] per community and W, the sum of all pair weights
static __global__ void InternalKernel(const int *d_src, const int *d_dst, const int *d_pw, const int *d_community, long long pairs,
                                      unsigned long long *d_internal, unsigned long long *d_total)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (pairs + stride - 1) / stride;
    long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned long long sum = 0;
    for (long long r = 0; r < rounds; ++r, e += stride) {  // (wave-uniform)
        if (e >= pairs) continue;
        const unsigned long long w = static_cast<unsigned long long>(d_pw[e]);
        sum += w;
        const int a = d_community[d_src[e]];
        if (a == d_community[d_dst[e]]) atomicAdd(d_internal + a, w);
    }
    sum = util::WaveSum(sum);
    if (util::LaneId() == 0 && sum) atomicAdd(d_total, sum);
}

}  // namespace lp
}  // namespace app
}  // namespace gunrock
