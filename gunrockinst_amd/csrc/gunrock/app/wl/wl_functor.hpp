// app/wl/wl_functor.hpp -- colour refinement (1-WL): the definition (host and device) and the kernels of a round.
//
// The reference snapshot has no colour refinement.  The graph is the CSR as given: a row is the multiset of its entries, duplicates
// and self-loops count, one-way entries are one-way.  A round maps the colouring c to c' with c'(u) = c'(v) iff c(u) = c(v) and the
// multisets {c(w) : w in row(u)} and {c(w) : w in row(v)} are equal.
//
// Between the kernels a colour is the smallest member of its class, a vertex id; the dense ids 0 .. count - 1 by ascending smallest
// member are made once, on the way out (wl_problem.hpp Finish).  A round is
//   SigKernel     sig(v) = the wrapping 128-bit sum over row v of Mix(seed, attempt, c[col]), cut to its top sig_bits bits.  A sum commutes, so the
//                 value does not depend on who adds.  By the row's length (Regime(), lp's split and option names): LANE one row per
//                 lane; WAVE into waves[] for SigWaveKernel, one row per wave, the lanes over the entries (16-byte loads of the
//                 aligned body of the row) and a cross-lane add; BLOCK into hubs[] for SigHubKernel, a workgroup per row.  The
//                 gather c[col] is the cost.
//   GroupKernel   an open-addressed global table of at least 2 n slots groups the vertices by (c(v), sig(v)): a slot is claimed by CAS
//                 with a vertex id, equality is decided by comparing that owner's stored (c, sig) with one's own -- c exactly, so a
//                 round never merges two classes of the round before -- and smallest[slot] is kept by atomicMin.  The lanes of a wave
//                 that hold one key send one of them.  Who claimed a slot reaches no output: only smallest[] is read afterwards.
//                 When the certificate refused an attempt at this round, the next attempt groups by (that attempt's group, sig)
//                 in place of (c, sig): what one hash told apart stays apart, and the attempts of a round add up.
//   AssignKernel  fresh(v) = smallest[slot(v)]; a vertex with fresh(v) = v is the smallest of its group and counts one class.
//   CertKernel    the certificate.  A hash can merge what should be split and nothing else (equal multisets hash equal), so for
//                 every v with r = fresh(v) != v the multisets of c over row(v) and row(r) are compared exactly: unequal lengths fail
//                 at once; else a colour -> int table takes +1 per entry of row(r) and -1 per entry of row(v) and every slot must end
//                 at 0.  The table is the ladder's (app/table_ladder.hpp) over w = the entries of both rows: a wave's part of LDS,
//                 the workgroup's LDS (CertBlockKernel), or a dense int32[n] row in global scratch that the check itself puts back
//                 to 0 (CertGlobalKernel).  words[W_FAILS] counts the failing vertices.  With gate >= 0 the three kernels do nothing
//                 unless the round left `gate` classes: the host asks for the certificate of a round that split nothing without
//                 reading the count first.
//
// Nothing in a launch reads what the same launch writes, apart from atomics.  No kernel waits on another workgroup and every loop
// bound is a kernel argument, a constant or a value of the CSR.  Every loop that holds a wave operation is wave-uniform.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include <gunrock/app/table_ladder.hpp>
#include <gunrock/graphio/splitmix.hpp>
#include <gunrock/oprtr/lds_table.hpp>
#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace wl {

enum { WL_AUTO = 0, WL_LANE = 1, WL_WAVE = 2, WL_BLOCK = 3 };  // "strategy": the signature pass
enum { WL_STABLE = 0, WL_CAPPED = 1 };                         // how an Enact ended
enum { WL_RUNG_WAVE = 0, WL_RUNG_BLOCK = 1, WL_RUNG_GLOBAL = 2 };

constexpr int kWlThreads = 256;
constexpr int kWlWaves = kWlThreads / util::kWaveSize;
constexpr int kLaneMaxRow = 16;    // default "lane_max_row"  (lp's, by the same reasoning)
constexpr int kWaveMaxRow = 4096;  // default "wave_max_row"

namespace lds = oprtr::lds;
using util::Fmix32;

// ---------------- the definition ----------------

struct Sig {
    uint64_t lo, hi;
};

// the 128-bit mix of one entry: two splitmix64 streams over (attempt << 32 | colour); attempt < 2^32, colour in [0, 2^31)
GRX_HOST_DEVICE inline Sig Mix(uint64_t seed, uint64_t attempt, int colour)
{
    const uint64_t x = (attempt << 32) | static_cast<uint64_t>(static_cast<uint32_t>(colour));
    return Sig{graphio::Mix64(seed ^ graphio::Mix64(x)), graphio::Mix64(seed ^ graphio::Mix64(~x))};
}

// a += b as 128-bit numbers, wrapping
GRX_HOST_DEVICE inline void Add(Sig &a, const Sig &b)
{
    a.lo += b.lo;
    a.hi += b.hi + (a.lo < b.lo ? 1ull : 0ull);
}

// The top `bits` bits of the 128, bits in 1 .. 128.  The top, not the bottom: a row that holds one colour k times sums to k times
// its mix, and the low bits of such a product do not depend on the colour when k is even.
GRX_HOST_DEVICE inline Sig Truncate(Sig s, int bits)
{
    if (bits >= 128) return s;
    const int shift = 128 - bits;  // 1 .. 127
    if (shift >= 64) return Sig{s.hi >> (shift - 64), 0};
    return Sig{(s.lo >> shift) | (s.hi << (64 - shift)), s.hi >> shift};
}

GRX_HOST_DEVICE inline int Regime(int d, int strategy, int lane_max_row, int wave_max_row)
{
    if (strategy != WL_AUTO) return strategy;
    return d <= lane_max_row ? WL_LANE : (d <= wave_max_row ? WL_WAVE : WL_BLOCK);
}

// the rung of the certificate of a vertex with d entries: both rows together are what the table holds at the most
GRX_HOST_DEVICE inline int Rung(long long d, int table_slots, int block_slots)
{
    return ladder::Widen(ladder::WAVE, 2 * d, table_slots, block_slots) - ladder::WAVE;
}

// ---------------- the kernels ----------------

// the 64-bit words the kernels and the host share; the first kRoundWords are cleared in front of every round
enum {
    W_CLASSES = 0,  // groups of this round
    W_FAILS,        // vertices the certificate refused
    W_CERT,         // vertices the certificate compared
    W_WAVES,        // rows handed to SigWaveKernel
    W_HUBS,         // rows handed to SigHubKernel
    W_BLOCK_LIST,   // vertices handed to CertBlockKernel
    W_GLOBAL_LIST,  // ... to CertGlobalKernel
    kRoundWords,
    W_REGIME = kRoundWords,  // three words: rows of the signature passes since the Enact began, per regime
    W_RUNG = W_REGIME + 3,   // three words: vertices compared, per rung
    W_COUNT = 16
};

struct Ctx {
    const int *ro, *ci;
    const int *colour;  // c: the smallest member of the class
    const int *key;     // what a group must share exactly: c, or what a refused attempt at this round made of it (the start
                        // grouping: the labels, any int32, or NULL for one class)
    int *fresh;         // c' of this round
    Sig *sig;
    unsigned long long *slot;  // per vertex, its slot of the table
    int *owner;                // the table: the vertex that claimed the slot, -1 none
    unsigned *smallest;        // ... and the smallest vertex of the group, 0xFFFFFFFF none
    int *waves, *hubs, *block_list, *global_list;
    unsigned long long *words;
    unsigned long long table_mask;  // slots - 1
    uint64_t seed, attempt;
    int nodes;
    int strategy, lane_max_row, wave_max_row, sig_bits;
    int table_slots, block_slots;
    int vector_loads;  // ci is 16-byte aligned
};

__device__ __forceinline__ Sig WaveAdd(Sig s)
{
#pragma unroll
    for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) {
        Sig o;
        o.lo = __shfl_xor(static_cast<unsigned long long>(s.lo), d, util::kWaveSize);
        o.hi = __shfl_xor(static_cast<unsigned long long>(s.hi), d, util::kWaveSize);
        Add(s, o);
    }
    return s;
}

// This thread's share of the sum over row [b, e), thread tid of G: the entries in front of the first 16-byte boundary and behind the
// last one by one, the body four at a time.
template <int G>
__device__ __forceinline__ Sig RowShare(const Ctx &c, int b, int e, int tid)
{
    Sig s{0, 0};
    int head = b, tail = e;
    if (c.vector_loads && e - b >= 8) {
        head = (b + 3) & ~3;
        tail = e & ~3;
        for (int i = head + 4 * tid; i < tail; i += 4 * G) {
            const int4 q = *reinterpret_cast<const int4 *>(c.ci + i);
            Add(s, Mix(c.seed, c.attempt, c.colour[q.x]));
            Add(s, Mix(c.seed, c.attempt, c.colour[q.y]));
            Add(s, Mix(c.seed, c.attempt, c.colour[q.z]));
            Add(s, Mix(c.seed, c.attempt, c.colour[q.w]));
        }
        for (int i = b + tid; i < head; i += G) Add(s, Mix(c.seed, c.attempt, c.colour[c.ci[i]]));
        for (int i = tail + tid; i < e; i += G) Add(s, Mix(c.seed, c.attempt, c.colour[c.ci[i]]));
        return s;
    }
    for (int i = b + tid; i < e; i += G) Add(s, Mix(c.seed, c.attempt, c.colour[c.ci[i]]));
    return s;
}

// All lanes of the wave call; the lanes with `hit` append v to list[] through words[word]: one atomic per wave.  A vertex enters a
// list once, so a position stays under `nodes`; the test keeps a mistake elsewhere from turning into a store outside the array.
__device__ __forceinline__ void Append(const Ctx &c, int word, int *list, bool hit, int v)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned long long pos = oprtr::WaveTicket(c.words + word, mask);
    if (hit && pos < static_cast<unsigned long long>(c.nodes)) list[pos] = v;
}

// One lane per vertex: LANE rows by their lane, WAVE rows into waves[] and BLOCK rows into hubs[] for the two kernels below -- a
// wave that walked the long rows of its own 64 vertices one after the other would be the tail of the launch on a skewed graph,
// whose long rows sit next to each other.
static __global__ __launch_bounds__(kWlThreads) void SigKernel(Ctx c)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    unsigned rows[3] = {0, 0, 0};
    for (long long from = wave0 * util::kWaveSize; from < c.nodes; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long at = from + lane;
        const int v = at < c.nodes ? static_cast<int>(at) : -1;
        int b = 0, e = 0, regime = 0;
        if (v >= 0) {
            b = c.ro[v];
            e = c.ro[v + 1];
            if (e > b) {
                regime = Regime(e - b, c.strategy, c.lane_max_row, c.wave_max_row);
                rows[0] += regime == WL_LANE;
                rows[1] += regime == WL_WAVE;
                rows[2] += regime == WL_BLOCK;
            }
        }
        Append(c, W_WAVES, c.waves, regime == WL_WAVE, v);
        Append(c, W_HUBS, c.hubs, regime == WL_BLOCK, v);
        if (v < 0 || regime > WL_LANE) continue;
        Sig s{0, 0};
        for (int i = b; i < e; ++i) Add(s, Mix(c.seed, c.attempt, c.colour[c.ci[i]]));
        c.sig[v] = Truncate(s, c.sig_bits);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const unsigned sum = util::WaveSum(rows[r]);
        if (lane == 0 && sum) atomicAdd(c.words + W_REGIME + r, static_cast<unsigned long long>(sum));
    }
}

// One wave per row of waves[]; W_WAVES is what SigKernel left (a kernel boundary lies between).
static __global__ __launch_bounds__(kWlThreads) void SigWaveKernel(Ctx c)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    long long listed = static_cast<long long>(c.words[W_WAVES]);
    if (listed > c.nodes) listed = c.nodes;
    for (long long i = wave0; i < listed; i += nwaves) {  // (wave-uniform)
        const int v = c.waves[i];
        const Sig s = WaveAdd(RowShare<util::kWaveSize>(c, c.ro[v], c.ro[v + 1], lane));
        if (lane == 0) c.sig[v] = Truncate(s, c.sig_bits);
    }
}

// One workgroup per row of hubs[]; W_HUBS is what SigKernel left (a kernel boundary lies between).
static __global__ __launch_bounds__(kWlThreads) void SigHubKernel(Ctx c)
{
    __shared__ Sig s_part[kWlWaves];
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    long long hubs = static_cast<long long>(c.words[W_HUBS]);
    if (hubs > c.nodes) hubs = c.nodes;
    for (long long i = blockIdx.x; i < hubs; i += gridDim.x) {  // (uniform over the workgroup)
        const int v = c.hubs[i];
        const Sig part = WaveAdd(RowShare<kWlThreads>(c, c.ro[v], c.ro[v + 1], static_cast<int>(threadIdx.x)));
        if (lane == 0) s_part[wave] = part;
        __syncthreads();
        if (threadIdx.x == 0) {
            Sig s{0, 0};
#pragma unroll
            for (int w = 0; w < kWlWaves; ++w) Add(s, s_part[w]);
            c.sig[v] = Truncate(s, c.sig_bits);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int LoadRelaxed(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned LoadRelaxed(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The groups of (key[v], sig(v)) (key NULL: 0 for all); sig = 0 for all when START (the start grouping by labels).
// The lanes of a wave with one key are sent by the lowest of them, which is also their smallest vertex.
template <bool START>
static __global__ __launch_bounds__(kWlThreads) void GroupKernel(Ctx c)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    for (long long from = wave0 * util::kWaveSize; from < c.nodes; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long id = from + lane;
        const bool live = id < c.nodes;
        const int v = live ? static_cast<int>(id) : -1;
        const int key = live && c.key ? c.key[v] : 0;
        const Sig s = live && !START ? c.sig[v] : Sig{0, 0};
        // one sender per key of the wave
        int sender = lane;
        unsigned long long todo = __ballot(live);
        while (todo) {  // (wave-uniform; at most 64 times)
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lkey = __shfl(key, leader, util::kWaveSize);
            const unsigned long long llo = __shfl(static_cast<unsigned long long>(s.lo), leader, util::kWaveSize);
            const unsigned long long lhi = __shfl(static_cast<unsigned long long>(s.hi), leader, util::kWaveSize);
            const bool same = live && key == lkey && s.lo == llo && s.hi == lhi;
            if (same) sender = leader;
            todo &= ~__ballot(same);
        }
        unsigned long long at = 0;
        if (live && sender == lane) {
            at = graphio::Mix64(s.lo ^ graphio::Mix64(s.hi ^ static_cast<uint64_t>(static_cast<uint32_t>(key)))) & c.table_mask;
            for (unsigned long long probe = 0; probe <= c.table_mask; ++probe) {  // (the table has 2 n slots: an empty one is met)
                int was = LoadRelaxed(c.owner + at);
                if (was == -1) was = atomicCAS(c.owner + at, -1, v);
                if (was == -1 || was == v) break;
                if (was >= 0 && was < c.nodes) {
                    const int okey = c.key ? c.key[was] : 0;
                    const Sig os = START ? Sig{0, 0} : c.sig[was];
                    if (okey == key && os.lo == s.lo && os.hi == s.hi) break;
                }
                at = (at + 1) & c.table_mask;
            }
            if (LoadRelaxed(c.smallest + at) > static_cast<unsigned>(v)) atomicMin(c.smallest + at, static_cast<unsigned>(v));
        }
        at = __shfl(at, sender, util::kWaveSize);
        if (live) c.slot[v] = at;
    }
}

// fresh(v) = the smallest vertex of v's group; the groups are counted at their smallest vertices
static __global__ __launch_bounds__(kWlThreads) void AssignKernel(Ctx c)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long passes = (c.nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned count = 0;
    for (long long r = 0; r < passes; ++r, v += stride) {  // (wave-uniform)
        if (v >= c.nodes) continue;
        const unsigned long long at = c.slot[v] & c.table_mask;
        const unsigned f = c.smallest[at];
        c.fresh[v] = static_cast<int>(f <= static_cast<unsigned>(v) ? f : static_cast<unsigned>(v));  // (f <= v always: v itself took part in the min)
        count += f == static_cast<unsigned>(v);
    }
    count = util::WaveSum(count);
    if (util::LaneId() == 0 && count) atomicAdd(c.words + W_CLASSES, static_cast<unsigned long long>(count));
}

// ---------------- the certificate ----------------

__device__ __forceinline__ bool Gated(const Ctx &c, long long gate) { return gate >= 0 && c.words[W_CLASSES] != static_cast<unsigned long long>(gate); }

// Rows [rb, re) (the representative's) and [vb, ve) of equal length against each other in the group's table key[] / count[] of
// `slots` slots; uniform over the group: whether the multisets of colours differ.
template <bool BLOCK>
__device__ __forceinline__ bool TableDiffers(const Ctx &c, int rb, int re, int vb, int ve, int *key, int *count, int slots, int *s_flag)
{
    constexpr int G = BLOCK ? kWlThreads : util::kWaveSize;
    const int tid = BLOCK ? static_cast<int>(threadIdx.x) : static_cast<int>(util::LaneId());
    const int size = lds::TableSize(2ll * (re - rb), slots);
    unsigned long long probes = 0;  // (not counted)
    bool bad = false;
    lds::Clear<G>(key, size, tid, [&](int k) { count[k] = 0; });
    lds::GroupSync<BLOCK>();
    for (int i = rb + tid; i < re; i += G) {
        const int x = c.colour[c.ci[i]];
        const int at = lds::Claim(key, size, Fmix32(static_cast<unsigned>(x)), x, probes);
        if (at >= 0) atomicAdd(count + at, 1);
        bad |= at < 0;  // (never: the table holds both rows)
    }
    for (int i = vb + tid; i < ve; i += G) {
        const int x = c.colour[c.ci[i]];
        const int at = lds::Claim(key, size, Fmix32(static_cast<unsigned>(x)), x, probes);
        if (at >= 0) atomicAdd(count + at, -1);
        bad |= at < 0;
    }
    lds::GroupSync<BLOCK>();
    for (int k = tid; k < size; k += G) bad |= count[k] != 0;
    bool any;
    if (BLOCK) {
        if (tid == 0) *s_flag = 0;
        __syncthreads();
        if (bad) *s_flag = 1;
        __syncthreads();
        any = *s_flag != 0;
        __syncthreads();  // (the next vertex clears what this one still reads)
    } else {
        any = __ballot(bad) != 0;
        lds::WaveLdsSync();
    }
    return any;
}

// One wave per 64 vertices: a vertex that is its own representative passes, rows of unequal length fail, WAVE-rung vertices are
// compared one after the other by the whole wave, the others go into the lists of the kernels below.
static __global__ __launch_bounds__(kWlThreads) void CertKernel(Ctx c, long long gate)
{
    extern __shared__ int s_table[];  // kWlWaves * table_slots keys, then as many counts
    if (Gated(c, gate)) return;
    const int lane = static_cast<int>(util::LaneId());
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize;
    int *key = s_table + static_cast<size_t>(wave) * c.table_slots;
    int *count = s_table + static_cast<size_t>(kWlWaves + wave) * c.table_slots;
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    unsigned fails = 0, compared = 0, rung_rows[3] = {0, 0, 0};
    for (long long from = wave0 * util::kWaveSize; from < c.nodes; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long id = from + lane;
        const int v = id < c.nodes ? static_cast<int>(id) : -1;
        int rb = 0, re = 0, vb = 0, ve = 0, rung = -1;
        if (v >= 0) {
            const int r = c.fresh[v];
            if (r != v && r >= 0 && r < c.nodes) {
                ++compared;
                rb = c.ro[r];
                re = c.ro[r + 1];
                vb = c.ro[v];
                ve = c.ro[v + 1];
                if (re - rb != ve - vb) {
                    ++fails;
                } else if (ve > vb) {
                    rung = Rung(ve - vb, c.table_slots, c.block_slots);
                    rung_rows[0] += rung == WL_RUNG_WAVE;
                    rung_rows[1] += rung == WL_RUNG_BLOCK;
                    rung_rows[2] += rung == WL_RUNG_GLOBAL;
                }
            }
        }
        unsigned long long todo = __ballot(rung == WL_RUNG_WAVE);
        while (todo) {  // (wave-uniform)
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lrb = __shfl(rb, leader, util::kWaveSize), lre = __shfl(re, leader, util::kWaveSize);
            const int lvb = __shfl(vb, leader, util::kWaveSize), lve = __shfl(ve, leader, util::kWaveSize);
            const bool differs = TableDiffers<false>(c, lrb, lre, lvb, lve, key, count, c.table_slots, nullptr);
            if (lane == leader && differs) ++fails;
            todo &= todo - 1;
        }
        Append(c, W_BLOCK_LIST, c.block_list, rung == WL_RUNG_BLOCK, v);
        Append(c, W_GLOBAL_LIST, c.global_list, rung == WL_RUNG_GLOBAL, v);
    }
    fails = util::WaveSum(fails);
    compared = util::WaveSum(compared);
    if (lane == 0 && fails) atomicAdd(c.words + W_FAILS, static_cast<unsigned long long>(fails));
    if (lane == 0 && compared) atomicAdd(c.words + W_CERT, static_cast<unsigned long long>(compared));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const unsigned sum = util::WaveSum(rung_rows[r]);
        if (lane == 0 && sum) atomicAdd(c.words + W_RUNG + r, static_cast<unsigned long long>(sum));
    }
}

// One workgroup per vertex of block_list[]; W_BLOCK_LIST is what CertKernel left (a kernel boundary lies between).
static __global__ __launch_bounds__(kWlThreads) void CertBlockKernel(Ctx c, long long gate)
{
    extern __shared__ int s_table[];  // block_slots keys, then as many counts
    __shared__ int s_flag;
    if (Gated(c, gate)) return;
    long long listed = static_cast<long long>(c.words[W_BLOCK_LIST]);
    if (listed > c.nodes) listed = c.nodes;
    unsigned fails = 0;
    for (long long i = blockIdx.x; i < listed; i += gridDim.x) {  // (uniform over the workgroup)
        const int v = c.block_list[i], r = c.fresh[v];
        if (TableDiffers<true>(c, c.ro[r], c.ro[r + 1], c.ro[v], c.ro[v + 1], s_table, s_table + c.block_slots, c.block_slots, &s_flag)) ++fails;
    }
    if (threadIdx.x == 0 && fails) atomicAdd(c.words + W_FAILS, static_cast<unsigned long long>(fails));
}

// One workgroup per vertex of global_list[], workgroup slot blockIdx.x with its counter row counters[blockIdx.x * nodes ..), all 0
// between two vertices.  The host launches no more workgroups than there are counter rows.
static __global__ __launch_bounds__(kWlThreads) void CertGlobalKernel(Ctx c, long long gate, int *counters)
{
    __shared__ int s_flag;
    if (Gated(c, gate)) return;
    int *row = counters + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(c.nodes);
    long long listed = static_cast<long long>(c.words[W_GLOBAL_LIST]);
    if (listed > c.nodes) listed = c.nodes;
    const int tid = static_cast<int>(threadIdx.x);
    unsigned fails = 0;
    for (long long i = blockIdx.x; i < listed; i += gridDim.x) {  // (uniform over the workgroup)
        const int v = c.global_list[i], r = c.fresh[v];
        const int rb = c.ro[r], re = c.ro[r + 1], vb = c.ro[v], ve = c.ro[v + 1];
        for (int k = rb + tid; k < re; k += kWlThreads) atomicAdd(row + c.colour[c.ci[k]], 1);
        for (int k = vb + tid; k < ve; k += kWlThreads) atomicAdd(row + c.colour[c.ci[k]], -1);
        if (tid == 0) s_flag = 0;
        lds::GlobalSync();
        // the row back to 0 by walking the two rows again; whoever takes a counter that is not 0 has found a difference
        bool bad = false;
        for (int k = rb + tid; k < re; k += kWlThreads) bad |= atomicExch(row + c.colour[c.ci[k]], 0) != 0;
        for (int k = vb + tid; k < ve; k += kWlThreads) bad |= atomicExch(row + c.colour[c.ci[k]], 0) != 0;
        if (bad) s_flag = 1;
        lds::GlobalSync();  // (the next vertex counts in the row this one cleared)
        if (s_flag) ++fails;
        __syncthreads();
    }
    if (tid == 0 && fails) atomicAdd(c.words + W_FAILS, static_cast<unsigned long long>(fails));
}

// ---------------- the build, the way out ----------------

// the longest row: whether any row can reach SigHubKernel, CertBlockKernel or CertGlobalKernel
static __global__ void LongestKernel(const int *ro, long long nodes, unsigned long long *longest)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long passes = (nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    int most = 0;
    for (long long r = 0; r < passes; ++r, v += stride)  // (wave-uniform)
        if (v < nodes && ro[v + 1] - ro[v] > most) most = ro[v + 1] - ro[v];
#pragma unroll
    for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) {
        const int o = __shfl_xor(most, d, util::kWaveSize);
        most = o > most ? o : most;
    }
    if (util::LaneId() == 0 && most) atomicMax(longest, static_cast<unsigned long long>(most));
}

static __global__ void LeaderFlagKernel(const int *colour, long long nodes, unsigned *flag)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) flag[v] = colour[v] == v ? 1u : 0u;
}

// dense[v] = the rank of v's class by ascending smallest member; with size[] and representative[], those too (size[] all 0 before).
// The lanes of a wave that share a class add once: a class of half the graph would otherwise be half the graph's atomics on a word.
static __global__ void DenseKernel(const int *colour, const int *rank, long long nodes, int *dense, unsigned long long *size, int *representative)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long passes = (nodes + stride - 1) / stride;
    const int lane = static_cast<int>(util::LaneId());
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (long long p = 0; p < passes; ++p, v += stride) {  // (wave-uniform)
        const bool live = v < nodes;
        int r = -1, id = -1;
        if (live) {
            r = colour[v];
            id = rank[r];
            dense[v] = id;
            if (representative && r == v) representative[id] = static_cast<int>(v);
        }
        unsigned long long todo = size ? __ballot(live) : 0ull;
        while (todo) {  // (wave-uniform; at most 64 times)
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const unsigned long long same = __ballot(live && id == __shfl(id, leader, util::kWaveSize));
            if (lane == leader) atomicAdd(size + id, static_cast<unsigned long long>(__popcll(same)));
            todo &= ~same;
        }
    }
}

}  // namespace wl
}  // namespace app
}  // namespace gunrock
