// app/c4/c4_functor.hpp -- device kernels of 4-cycle (butterfly) counting: per vertex, per edge, total.
//
// The reference snapshot has no 4-cycle counting; the shape follows this tree's primitives: the canonical pairs of
// graphio::PairGraph, label propagation's lane / wave / workgroup balance and its open-addressed LDS table, the clique primitive's
// refusal to overflow.
//
// The kernels work on a copy of the neighbour CSR in which the vertices are renumbered by their rank in (degree, id) order
// (c4_problem.hpp): row u ascending by rank, eid[] the canonical pair of every entry, dlow[u] the length of the prefix of row u that
// ranks below u, pre[i] for an entry i = (u, v) of that prefix the length of the prefix of row v that ranks below u.  A wedge of u is
// u - v - w with v and w below u; W[u] is their number, c(u, w) the number of them that end in w.  Every 4-cycle is counted once, at
// its highest-ranked vertex u, as a pair of wedges of u with the same end:
//   cycles[u] += C(c, 2), cycles[w] += C(c, 2), total += C(c, 2)   per end w
//   cycles[v] += c - 1, edge[uv] += c - 1, edge[vw] += c - 1        per wedge (u, v, w)
// Pass 1 of a start vertex counts the ends, pass 2 walks the same wedges again, looks c up and credits; the credits of one (u, v)
// are summed over its w in registers and reduced before the one atomic for cycles[v] and the one for edge[uv]; a credit of 0 is not
// sent.  All sums are integers: every regime gives identical arrays.  By W (Regime()):
//   LANE    W <= lane_max_wedges: one start vertex per lane, the ends in a private array, a compare loop finds every c
//   WAVE    W <= table_slots / 2: one start vertex per wave, an open-addressed end -> count table in the wave's part of LDS
//   BLOCK   W <= block_slots / 2: one workgroup per start vertex, the workgroup's LDS as one table, workgroup barriers
//   GLOBAL  the rest: one workgroup per start vertex and a dense int32[n] counter row per workgroup slot in global scratch, which a
//           third walk of the same wedges clears again (its exchange hands C(c, 2) to whoever clears an end first)
// W[u] bounds the distinct ends of u and a table has at least 2 W slots, so a table never fills: no overflow flag and no retry.
//
// Nothing in a launch reads what the same launch writes, apart from atomics (the counter rows are read by atomic loads).  No kernel
// waits on another workgroup and every loop bound is a kernel argument, a constant or a value of the build's arrays.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/table_ladder.hpp>
#include <gunrock/graphio/pair_graph.hpp>
#include <gunrock/oprtr/lds_table.hpp>
#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace c4 {

typedef unsigned long long Count;  // the bits of an int64 count (never beyond 2^62: the enactor refuses first)

enum { C4_AUTO = 0, C4_LANE = 1, C4_WAVE = 2, C4_BLOCK = 3, C4_GLOBAL = 4 };  // "strategy"; 1 .. 4 are the regimes
static_assert(C4_WAVE == ladder::WAVE && C4_BLOCK == ladder::BLOCK && C4_GLOBAL == ladder::GLOBAL, "the ladder's rungs");

constexpr int kC4Threads = 256;
constexpr int kC4Waves = kC4Threads / util::kWaveSize;
constexpr int kLaneArray = 32;        // the private array of the LANE regime: the largest "lane_max_wedges"
constexpr int kLaneMaxWedges = 16;    // default "lane_max_wedges"  (by reasoning)
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
    W_TOTAL = 0,     // 4-cycles
    W_PROBES,        // table probes of passes 1 and 2
    W_BLOCK_LIST,    // start vertices handed to BlockKernel
    W_GLOBAL_LIST,   // ... to GlobalKernel
    W_VERTICES,      // four words: the start vertices of the regimes LANE .. GLOBAL
    W_WEDGES = W_VERTICES + 4,  // four words: their wedges
    W_COUNT = 16
};

struct Ctx {
    const int *ro, *ci, *eid;  // the renumbered neighbour CSR and the canonical pair of every entry
    const int *pre;            // per entry (u, v) of the lower prefix of row u: the entries of row v below u
    const int *dlow, *wedges;  // per start vertex: the lower prefix of its row, W
    const int *inv;            // rank -> vertex id
    Count *cycles;             // by vertex id
    Count *edge_cycles;        // by canonical pair, or NULL ("edges" = 0)
    unsigned long long *words;
    int *block_list, *global_list;
    int nodes;
    int strategy, lane_max_wedges, table_slots, block_slots;
};

// The regime of a start vertex with w >= 2 wedges: the smallest that holds it, not below a forced one.
__host__ __device__ __forceinline__ int Regime(long long w, int strategy, int lane_max_wedges, int table_slots, int block_slots)
{
    int r = strategy == C4_AUTO ? C4_LANE : strategy;
    if (r == C4_LANE && w > lane_max_wedges) r = C4_WAVE;
    return ladder::Widen(r, w, table_slots, block_slots);
}

__device__ __forceinline__ Count Pairs(int c) { return static_cast<Count>(c) * static_cast<Count>(c - 1) / 2; }

struct Tally {
    Count total = 0, probes = 0;
    unsigned vertices[4] = {0, 0, 0, 0};
    Count wedges[4] = {0, 0, 0, 0};
};

// (all lanes of the wave call)
__device__ __forceinline__ void Flush(Tally &t, const Ctx &c)
{
    const Count total = util::WaveSum(t.total), probes = util::WaveSum(t.probes);
    if (util::LaneId() == 0) {
        if (total) atomicAdd(c.words + W_TOTAL, total);
        if (probes) atomicAdd(c.words + W_PROBES, probes);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned vertices = util::WaveSum(t.vertices[r]);
        const Count wedges = util::WaveSum(t.wedges[r]);
        if (util::LaneId() == 0 && vertices) {
            atomicAdd(c.words + W_VERTICES + r, static_cast<Count>(vertices));
            atomicAdd(c.words + W_WEDGES + r, wedges);
        }
    }
    t = Tally();
}

__device__ __forceinline__ void Credit(Count *array, int at, Count value)
{
    if (value) atomicAdd(array + at, value);
}

// All lanes of the wave call; the lanes with `hit` append u to list[] through words[word]: one atomic per wave.  A start vertex enters
// a list once, so a position stays under `nodes`; the test keeps a mistake elsewhere from turning into a store outside the array.
__device__ __forceinline__ void Append(const Ctx &c, int word, int *list, bool hit, int u)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned long long pos = oprtr::WaveTicket(c.words + word, mask);
    if (hit) {
        if (pos < static_cast<unsigned long long>(c.nodes)) list[pos] = u;
    }
}

// ---------------- LANE ----------------

// the ends of u in a private array, in the order of the walk; c of wedge k is the number of equal ends, and the first wedge of an end
// credits its C(c, 2)
__device__ __forceinline__ void LaneCount(const Ctx &c, int u, Tally &t)
{
    int ends[kLaneArray];
    const int b = c.ro[u], d = c.dlow[u];
    int count = 0;
    for (int i = b; i < b + d; ++i) {
        const int rv = c.ro[c.ci[i]], p = c.pre[i];
        for (int j = 0; j < p; ++j)
            if (count < kLaneArray) ends[count++] = c.ci[rv + j];
    }
    Count own = 0;
    int k = 0;
    for (int i = b; i < b + d; ++i) {
        const int v = c.ci[i], rv = c.ro[v], p = c.pre[i];
        Count through = 0;
        for (int j = 0; j < p && k < count; ++j, ++k) {
            const int w = ends[k];
            int same = 0;
            bool first = true;
            for (int q = 0; q < count; ++q) {
                const bool equal = ends[q] == w;
                same += equal;
                first &= !(equal && q < k);
            }
            if (same < 2) continue;
            through += static_cast<Count>(same - 1);
            if (c.edge_cycles) Credit(c.edge_cycles, c.eid[rv + j], static_cast<Count>(same - 1));
            if (first) {
                Credit(c.cycles, c.inv[w], Pairs(same));
                own += Pairs(same);
            }
        }
        Credit(c.cycles, c.inv[v], through);
        if (c.edge_cycles) Credit(c.edge_cycles, c.eid[i], through);
    }
    Credit(c.cycles, c.inv[u], own);
    t.total += own;
}

// ---------------- WAVE and BLOCK ----------------

// The 4-cycles owned by u, by a wave (BLOCK = false) or by the workgroup (BLOCK = true), uniform over the group.  key[] / count[] are
// the group's table of `slots` slots.  A wave takes one v at a time and its lanes the w of that v.
template <bool BLOCK>
__device__ __forceinline__ void TableCount(const Ctx &c, int u, int *key, int *count, int slots, Tally &t)
{
    constexpr int G = BLOCK ? kC4Threads : util::kWaveSize;
    constexpr int WAVES = BLOCK ? kC4Waves : 1;
    const int tid = BLOCK ? static_cast<int>(threadIdx.x) : static_cast<int>(util::LaneId());
    const int lane = static_cast<int>(util::LaneId());
    const int wave = BLOCK ? static_cast<int>(threadIdx.x) / util::kWaveSize : 0;
    const int size = TableSize(c.wedges[u], slots);
    const int b = c.ro[u], d = c.dlow[u];
    lds::Clear<G>(key, size, tid, [&](int k) { count[k] = 0; });
    lds::GroupSync<BLOCK>();
    for (int i = b + wave; i < b + d; i += WAVES) {  // pass 1
        const int rv = c.ro[c.ci[i]], p = c.pre[i];
        for (int j = lane; j < p; j += util::kWaveSize) {
            const int w = c.ci[rv + j];
            const int at = lds::Claim(key, size, Fmix32(static_cast<unsigned>(w)), w, t.probes);
            if (at >= 0) atomicAdd(count + at, 1);  // (always: the table never fills)
        }
    }
    lds::GroupSync<BLOCK>();
    for (int i = b + wave; i < b + d; i += WAVES) {  // pass 2 (wave-uniform)
        const int v = c.ci[i], rv = c.ro[v], p = c.pre[i];
        Count through = 0;
        for (int j = lane; j < p; j += util::kWaveSize) {
            const int w = c.ci[rv + j];
            const int at = lds::Find(key, size, Fmix32(static_cast<unsigned>(w)), w, t.probes);  // (there: pass 1 claimed it)
            const int same = at >= 0 ? count[at] : 0;
            if (same < 2) continue;
            through += static_cast<Count>(same - 1);
            if (c.edge_cycles) Credit(c.edge_cycles, c.eid[rv + j], static_cast<Count>(same - 1));
        }
        through = util::WaveSum(through);
        if (lane == 0) {
            Credit(c.cycles, c.inv[v], through);
            if (c.edge_cycles) Credit(c.edge_cycles, c.eid[i], through);
        }
    }
    Count own = 0;
    for (int k = tid; k < size; k += G) {  // every end once
        const int w = key[k], same = count[k];
        if (w < 0 || same < 2) continue;
        Credit(c.cycles, c.inv[w], Pairs(same));
        own += Pairs(same);
    }
    t.total += own;
    own = util::WaveSum(own);
    if (lane == 0) Credit(c.cycles, c.inv[u], own);
    lds::GroupSync<BLOCK>();  // (the next start vertex clears what this one still reads)
}

// One wave per 64 start vertices, lane l of wave group g takes the rank l * groups + g: every wave meets the whole range of degrees.
// LANE vertices by their lane, WAVE vertices one after the other by the whole wave, the others into the lists of the kernels below.
// Every loop that holds a wave operation is wave-uniform.
static __global__ __launch_bounds__(kC4Threads) void SmallKernel(Ctx c)
{
    extern __shared__ int s_table[];  // kC4Waves * table_slots keys, then as many counts
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    int *key = s_table + static_cast<size_t>(wave) * c.table_slots;
    int *count = s_table + static_cast<size_t>(kC4Waves + wave) * c.table_slots;
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    const long long groups = (static_cast<long long>(c.nodes) + util::kWaveSize - 1) / util::kWaveSize;
    Tally t;
    for (long long g = wave0; g < groups; g += nwaves) {  // (wave-uniform)
        const long long at = lane * groups + g;
        const int u = at < c.nodes ? static_cast<int>(at) : -1;
        int regime = 0;
        if (u >= 0) {
            const int w = c.wedges[u];
            if (w >= 2) {
                regime = Regime(w, c.strategy, c.lane_max_wedges, c.table_slots, c.block_slots);
                ++t.vertices[regime - 1];
                t.wedges[regime - 1] += static_cast<Count>(w);
            }
        }
        if (regime == C4_LANE) LaneCount(c, u, t);
        unsigned long long todo = __ballot(regime == C4_WAVE);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            TableCount<false>(c, __shfl(u, leader, util::kWaveSize), key, count, c.table_slots, t);
            todo &= todo - 1;
        }
        Append(c, W_BLOCK_LIST, c.block_list, regime == C4_BLOCK, u);
        Append(c, W_GLOBAL_LIST, c.global_list, regime == C4_GLOBAL, u);
    }
    Flush(t, c);
}

// One workgroup per start vertex of block_list[]; W_BLOCK_LIST is what SmallKernel left (a kernel boundary lies between).
static __global__ __launch_bounds__(kC4Threads) void BlockKernel(Ctx c)
{
    extern __shared__ int s_table[];  // block_slots keys, then as many counts
    long long listed = static_cast<long long>(c.words[W_BLOCK_LIST]);
    if (listed > c.nodes) listed = c.nodes;
    Tally t;
    for (long long i = blockIdx.x; i < listed; i += gridDim.x)  // (uniform over the workgroup)
        TableCount<true>(c, c.block_list[i], s_table, s_table + c.block_slots, c.block_slots, t);
    Flush(t, c);
}

// ---------------- GLOBAL ----------------

// One workgroup per start vertex of global_list[], workgroup slot blockIdx.x with its counter row rows[blockIdx.x * nodes ..), all 0
// between two start vertices.  The host launches no more workgroups than there are rows.
static __global__ __launch_bounds__(kC4Threads) void GlobalKernel(Ctx c, int *rows)
{
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    int *row = rows + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(c.nodes);
    long long listed = static_cast<long long>(c.words[W_GLOBAL_LIST]);
    if (listed > c.nodes) listed = c.nodes;
    Tally t;
    for (long long at = blockIdx.x; at < listed; at += gridDim.x) {  // (uniform over the workgroup)
        const int u = c.global_list[at];
        const int b = c.ro[u], d = c.dlow[u];
        for (int i = b + wave; i < b + d; i += kC4Waves) {  // pass 1
            const int rv = c.ro[c.ci[i]], p = c.pre[i];
            for (int j = lane; j < p; j += util::kWaveSize) atomicAdd(row + c.ci[rv + j], 1);
        }
        lds::GlobalSync();
        for (int i = b + wave; i < b + d; i += kC4Waves) {  // pass 2 (wave-uniform)
            const int v = c.ci[i], rv = c.ro[v], p = c.pre[i];
            Count through = 0;
            for (int j = lane; j < p; j += util::kWaveSize) {
                const int same = util::LoadAgent(row + c.ci[rv + j]);
                if (same < 2) continue;
                through += static_cast<Count>(same - 1);
                if (c.edge_cycles) Credit(c.edge_cycles, c.eid[rv + j], static_cast<Count>(same - 1));
            }
            through = util::WaveSum(through);
            if (lane == 0) {
                Credit(c.cycles, c.inv[v], through);
                if (c.edge_cycles) Credit(c.edge_cycles, c.eid[i], through);
            }
        }
        lds::GlobalSync();
        Count own = 0;
        for (int i = b + wave; i < b + d; i += kC4Waves) {  // pass 3: the row back to 0; who clears an end credits it
            const int rv = c.ro[c.ci[i]], p = c.pre[i];
            for (int j = lane; j < p; j += util::kWaveSize) {
                const int w = c.ci[rv + j];
                const int same = atomicExch(row + w, 0);
                if (same < 2) continue;
                Credit(c.cycles, c.inv[w], Pairs(same));
                own += Pairs(same);
            }
        }
        t.total += own;
        own = util::WaveSum(own);
        if (lane == 0) Credit(c.cycles, c.inv[u], own);
        lds::GlobalSync();
    }
    Flush(t, c);
}

// ---------------- the build ----------------

static __global__ void PairDegreeKernel(const int *d_src, const int *d_dst, long long pairs, unsigned *d_deg)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < pairs; e += stride) {
        atomicAdd(d_deg + d_src[e], 1u);
        atomicAdd(d_deg + d_dst[e], 1u);
    }
}

// (d(v) << col_bits) | v: sorted, the vertices by (degree, id)
static __global__ void RankKeysKernel(const unsigned *d_deg, long long nodes, int col_bits, unsigned long long *d_keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride)
        d_keys[v] = (static_cast<unsigned long long>(d_deg[v]) << col_bits) | static_cast<unsigned long long>(v);
}

static __global__ void RankKernel(const unsigned long long *d_keys, long long nodes, int col_bits, int *d_rank, int *d_inv)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long r = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; r < nodes; r += stride) {
        const int v = static_cast<int>(d_keys[r] & mask);
        d_inv[r] = v;
        d_rank[v] = static_cast<int>(r);
    }
}

// both directions of every pair in ranks: (rank(a) << cb) | rank(b) at e, the reverse at pairs + e
static __global__ void RowKeysKernel(const int *d_src, const int *d_dst, const int *d_rank, long long pairs, int col_bits, unsigned long long *d_keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < pairs; e += stride) {
        const unsigned long long a = static_cast<unsigned long long>(d_rank[d_src[e]]), b = static_cast<unsigned long long>(d_rank[d_dst[e]]);
        d_keys[e] = (a << col_bits) | b;
        d_keys[pairs + e] = (b << col_bits) | a;
    }
}

// for u = 0 .. nodes: ro[u] = the keys below (u, 0); for u < nodes: dlow[u] = those of row u below (u, u)
static __global__ void OffsetsKernel(const unsigned long long *d_keys, long long entries, long long nodes, int col_bits, int *d_ro, int *d_dlow)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long u = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; u <= nodes; u += stride) {
        const unsigned long long x = static_cast<unsigned long long>(u) << col_bits;
        const long long start = graphio::KeyLowerBound(d_keys, entries, x);
        d_ro[u] = static_cast<int>(start);
        if (u < nodes) d_dlow[u] = static_cast<int>(graphio::KeyLowerBound(d_keys, entries, x | static_cast<unsigned long long>(u)) - start);
    }
}

// entry i = (u, v) of the sorted keys: its column, its canonical pair (bisected in the pairs' keys) and, for v below u, the entries
// of row v below u, added to W[u]
static __global__ void EntriesKernel(const unsigned long long *d_keys, long long entries, int col_bits, const int *d_ro, const int *d_inv,
                                     const unsigned long long *d_ckeys, long long pairs, int *d_ci, int *d_eid, int *d_pre, int *d_wedges)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < entries; i += stride) {
        const unsigned long long key = d_keys[i];
        const unsigned long long u = key >> col_bits, v = key & mask;
        const unsigned a = static_cast<unsigned>(d_inv[u]), b = static_cast<unsigned>(d_inv[v]);
        const unsigned long long pair = a < b ? ((static_cast<unsigned long long>(a) << col_bits) | b) : ((static_cast<unsigned long long>(b) << col_bits) | a);
        d_ci[i] = static_cast<int>(v);
        d_eid[i] = static_cast<int>(graphio::KeyLowerBound(d_ckeys, pairs, pair));
        int below = 0;
        if (v < u) {
            below = static_cast<int>(graphio::KeyLowerBound(d_keys, entries, (v << col_bits) | u) - d_ro[v]);
            if (below) atomicAdd(d_wedges + u, below);
        }
        d_pre[i] = below;
    }
}

// summary[0] = the wedges, summary[1] = the largest W; *d_bound += W (dlow - 1) / 2 over the start vertices, in float64
static __global__ void SummaryKernel(const int *d_wedges, const int *d_dlow, long long nodes, unsigned long long *d_summary, double *d_bound)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (nodes + stride - 1) / stride;
    long long u = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned long long sum = 0, longest = 0;
    double bound = 0;
    for (long long r = 0; r < rounds; ++r, u += stride) {  // (wave-uniform)
        if (u >= nodes) continue;
        const unsigned long long w = static_cast<unsigned long long>(d_wedges[u]);
        sum += w;
        longest = w > longest ? w : longest;
        if (w) bound += static_cast<double>(w) * static_cast<double>(d_dlow[u] - 1) / 2.0;
    }
    sum = util::WaveSum(sum);
    bound = util::WaveSum(bound);
#pragma unroll
    for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(longest, d, util::kWaveSize);
        longest = o > longest ? o : longest;
    }
    if (util::LaneId() == 0 && sum) {
        atomicAdd(d_summary, sum);
        atomicMax(d_summary + 1, longest);
        if (bound > 0) atomicAdd(d_bound, bound);
    }
}

}  // namespace c4
}  // namespace app
}  // namespace gunrock
