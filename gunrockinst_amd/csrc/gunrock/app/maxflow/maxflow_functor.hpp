// app/maxflow/maxflow_functor.hpp -- device kernels of the maximum flow and the minimum cut (push-relabel on the residual graph).
//
// The reference snapshot has no app/mf (later Gunrock releases do); the shape follows this tree's primitives: BCC's one queue with
// the levels of a search as ranges of it, its lane / wave row balance and its one-workgroup device loop (scc_functor.hpp is
// included for the accessors and the tile rule, not changed).
//
// The residual graph is a symmetric CSR over the canonical pairs: row v holds the distinct neighbours of v ascending, entry i of
// row v is the arc v -> ci[i] with residual capacity res[i], and mate[i] is the entry of the reverse arc.  res[i] + res[mate[i]] is
// the pair's total capacity all the time, so one int holds each.
//
//   search     level-synchronous over residual arcs, forwards (res[i] > 0) or backwards (res[mate[i]] > 0), from one root; out[w]
//              is claimed by CAS from `unseen` to the level.  It is the global relabel (out = height), the return phase's relabel
//              and both sides of the cut.
//   discharge  one round over the list of active vertices.  A vertex finds its lowest residual neighbour (height, entry), pushes
//              to it when it is lower and relabels to lowest + 1 otherwise, up to discharge_steps times.  Only the owner lowers
//              res[] of its row and its own excess; everybody else only raises them, so a residual read by the owner is a lower
//              bound and nothing goes below 0.  Heights read from other vertices may be stale: that can cost rounds and can make
//              the labelling invalid, which is why the enactor certifies the result (no excess left, sink not reachable) before it
//              reports it.
//   the next list is appended to with one atomic per wave; mark[] (a round stamp, atomicMax) keeps a vertex from entering twice.
// A round and a search level are STEPs: a wide launch, or one of a stretch of steps inside a one-workgroup loop on the device, which
// puts a fence and a barrier between steps.  Everything one step leaves for the next -- and everything another wave may change
// within a step: res, height, excess -- is read with agent-scope loads (a CU's L1 is not refreshed by what lands in L2).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace maxflow {

enum { MAXFLOW_AUTO = 0, MAXFLOW_ROUNDS = 1, MAXFLOW_DEVICE_LOOP = 2 };
enum { PHASE_PREFLOW = 0, PHASE_RETURN, PHASE_CUT, PHASE_COUNT };

constexpr int kMaxflowThreads = 256;
constexpr int kDischargeSteps = 4;           // default "discharge_steps"
constexpr int kFar = INT_MAX;                // the cut's searches: not reached
constexpr unsigned kNever = 0xFFFFFFFFu;     // relabel limit: no global relabel on account of the count

using oprtr::kLoopMaxSteps;
using oprtr::kLoopThreads;
using oprtr::Ld;
using oprtr::Limits;
using oprtr::Narrow;
using oprtr::St;
using oprtr::TileFor;

// the words the kernels and the host share
enum {
    W_TAIL = 0,      // search: queue tickets handed out
    W_ENTRIES,       // search: row entries of the vertices queued so far, modulo 2^32
    W_NEXT,          // discharge: vertices in the next list
    W_NEXT_ENTRIES,  // discharge: their row entries (the word behind W_NEXT: the two are cleared together)
    W_RELABELS,      // relabels since the last global relabel
    W_FLAG,          // the certificate failed
    W_BAD,           // the build: a bad capacity
    W_COUNT = 8
};

// the 64-bit counters
enum { C_READS = 0, C_PUSHES, C_RELABELS, C_SIDE0, C_SIDE1, C_SIDE2, C_CUT0, C_CUT1, C_CAP0, C_CAP1, C_COUNT };

struct Ctx {
    const int *ro, *ci, *mate;  // the residual CSR, rows ascending, and the reverse entry of every entry
    int *res;                   // residual capacity per entry
    long long *excess;          // per vertex; src's is minus what left it
    int *height;
    int *queue;                 // a search's vertices, level by level
    int *mark;                  // the last round stamp under which a vertex entered a list
    unsigned *words;
    unsigned long long *counters;
    int nodes, src, sink;
    int wave_min_row, discharge_steps;
};

// one search: out[root] = base, out[w] = base + the residual distance; `skip` is never entered (-1: nobody)
struct Search {
    int *out;
    int unseen, skip, backward;
};

// a search's next level; the host and SearchLoopKernel carry the same
struct Front {
    int level;  // the value out[] holds for [head, tail)
    unsigned head, tail;
    unsigned entries_seen;  // W_ENTRIES when the level was complete
    unsigned step_entries;  // row entries of [head, tail)
};

// the discharge's next round; the host and DischargeLoopKernel carry the same
struct Active {
    unsigned count, entries;  // the current list and its row entries
    int cur;                  // which of the two lists it is
    int stamp;                // the round's stamp: vertices of the next list get stamp + 1
    unsigned relabels;        // W_RELABELS behind the last round
    int steps;                // rounds run by the loop launch
};

__device__ __forceinline__ long long LdExcess(const long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void AddExcess(long long *p, long long d)
{
    atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(d));  // (two's complement: d may be negative)
}

struct Tally {
    unsigned entries = 0;  // row entries of the vertices this lane queued or listed
    unsigned reads = 0;    // row entries this lane walked
    unsigned pushes = 0, relabels = 0;
};

// entries go to words[word]
__device__ __forceinline__ void Flush(Tally &t, const Ctx &c, int word)
{
    const unsigned entries = util::WaveSum(t.entries);
    const unsigned long long reads = util::WaveSum(static_cast<unsigned long long>(t.reads));
    const unsigned pushes = util::WaveSum(t.pushes), relabels = util::WaveSum(t.relabels);
    if (util::LaneId() == 0) {
        if (entries) atomicAdd(c.words + word, entries);
        if (reads) atomicAdd(c.counters + C_READS, reads);
        if (pushes) atomicAdd(c.counters + C_PUSHES, static_cast<unsigned long long>(pushes));
        if (relabels) {
            atomicAdd(c.counters + C_RELABELS, static_cast<unsigned long long>(relabels));
            atomicAdd(c.words + W_RELABELS, relabels);
        }
    }
    t = Tally();
}

// All lanes of the wave call; the lanes with `hit` append w to list[] through the ticket word `word`: one atomic per wave.  A vertex
// enters a queue or a list once, so a position stays under `nodes`; the test keeps a mistake elsewhere from turning into a store
// outside the array.
template <bool FRESH>
__device__ __forceinline__ void Append(const Ctx &c, int *list, int word, bool hit, int w, Tally &t)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned pos = oprtr::WaveTicket(c.words + word, mask);
    if (hit) {
        if (pos < static_cast<unsigned>(c.nodes)) St<FRESH>(list + pos, w);
        t.entries += static_cast<unsigned>(c.ro[w + 1] - c.ro[w]);
    }
}

// ---------------- the search ----------------

// entry i of row v, v at level L: claims w = ci[i] when the arc between them has residual capacity in the search's direction
template <bool FRESH>
__device__ __forceinline__ bool Claim(const Ctx &c, const Search &s, int i, int L, int &w)
{
    w = c.ci[i];
    if (w == s.skip) return false;
    const int r = Ld<FRESH>(c.res + (s.backward ? c.mate[i] : i));
    if (r <= 0) return false;
    if (Ld<FRESH>(s.out + w) != s.unseen) return false;
    return atomicCAS(s.out + w, s.unseen, L + 1) == s.unseen;  // (a stale plain read can only say "not reached")
}

// 64 queue entries by one wave: lane `lane` holds v (or -1) of level L.  Rows shorter than wave_min_row by their lane, the others by
// the whole wave, one after the other.  Every loop that holds a wave operation is wave-uniform.
template <bool FRESH>
__device__ __forceinline__ void SearchTile(const Ctx &c, const Search &s, int v, int L, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    int b = 0, e = 0;
    if (v >= 0) {
        b = c.ro[v];
        e = c.ro[v + 1];
    }
    const bool wide = e - b >= c.wave_min_row && e > b;
    unsigned long long todo = __ballot(wide);
    int longest = wide ? 0 : e - b;
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const int other = __shfl_xor(longest, o, util::kWaveSize);
        longest = other > longest ? other : longest;
    }
    for (int j = 0; j < longest; ++j) {  // (wave-uniform)
        int w = 0;
        bool hit = false;
        if (!wide && b + j < e) {
            ++t.reads;
            hit = Claim<FRESH>(c, s, b + j, L, w);
        }
        Append<FRESH>(c, c.queue, W_TAIL, hit, w, t);
    }
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
        for (int from = lb; from < le; from += util::kWaveSize) {  // (wave-uniform)
            const int i = from + lane;
            int w = 0;
            bool hit = false;
            if (i < le) {
                ++t.reads;
                hit = Claim<FRESH>(c, s, i, L, w);
            }
            Append<FRESH>(c, c.queue, W_TAIL, hit, w, t);
        }
        todo &= todo - 1;
    }
}

// level L = queue[head, tail), `tile` entries per wave at a time
template <bool FRESH>
__device__ __forceinline__ void SearchLevel(const Ctx &c, const Search &s, int L, long long head, long long tail, int tile, long long wave0,
                                            long long nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    if (tail > c.nodes) tail = c.nodes;
    for (long long from = head + wave0 * tile; from < tail; from += nwaves * tile) {  // (wave-uniform)
        const long long i = from + lane;
        int v = -1;
        if (lane < tile && i < tail) v = Ld<FRESH>(c.queue + i);
        SearchTile<FRESH>(c, s, v, L, t);
    }
}

// the root at level `base`, alone in the queue
static __global__ void SeedKernel(Ctx c, Search s, int root, int base)
{
    s.out[root] = base;
    c.queue[0] = root;
    c.words[W_TAIL] = 1u;
    c.words[W_ENTRIES] = static_cast<unsigned>(c.ro[root + 1] - c.ro[root]);
}

static __global__ __launch_bounds__(kMaxflowThreads) void SearchKernel(Ctx c, Search s, int L, unsigned head, unsigned tail, int tile)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    SearchLevel<false>(c, s, L, head, tail, tile, wave0, nwaves, t);
    Flush(t, c, W_ENTRIES);
}

// One workgroup searches level after level while each is narrow.  Every step ends in a barrier behind a fence, the two words are read
// with agent-scope loads by every thread, and a second barrier keeps the next step's atomics behind those reads.  Uniform control
// flow: every thread carries the same Front.  At most lim.max_steps levels per launch.
static __global__ __launch_bounds__(kLoopThreads) void SearchLoopKernel(Ctx c, Search s, Front f, Limits lim, Front *d_front)
{
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    Tally t;
    for (int step = 0; step < lim.max_steps && f.head < f.tail && Narrow(f.tail - f.head, f.step_entries, lim); ++step) {
        const int tile = TileFor(static_cast<long long>(f.tail - f.head), nwaves, f.step_entries);
        SearchLevel<true>(c, s, f.level, f.head, f.tail, tile, wave0, nwaves, t);
        Flush(t, c, W_ENTRIES);
        __threadfence();
        __syncthreads();
        const unsigned tail = static_cast<unsigned>(Ld<true>(reinterpret_cast<const int *>(c.words) + W_TAIL));
        const unsigned entries = static_cast<unsigned>(Ld<true>(reinterpret_cast<const int *>(c.words) + W_ENTRIES));
        ++f.level;
        f.head = f.tail;
        f.tail = tail;
        f.step_entries = entries - f.entries_seen;
        f.entries_seen = entries;
        __syncthreads();
    }
    if (threadIdx.x == 0) *d_front = f;
}

// ---------------- the discharge ----------------

__device__ __forceinline__ unsigned long long WaveMinKey(unsigned long long x)
{
#pragma unroll
    for (int d = util::kWaveSize / 2; d >= 1; d >>= 1) {
        const unsigned long long other = __shfl_xor(x, d, util::kWaveSize);
        x = other < x ? other : x;
    }
    return x;
}

// entry i as a candidate: (height of its end << 32 | i) when it has residual capacity, so that ties on height go to the smaller entry
__device__ __forceinline__ unsigned long long Candidate(const Ctx &c, int i, Tally &t)
{
    ++t.reads;
    if (Ld<true>(c.res + i) <= 0) return ~0ull;
    const unsigned hw = static_cast<unsigned>(Ld<true>(c.height + c.ci[i]));
    return (static_cast<unsigned long long>(hw) << 32) | static_cast<unsigned>(i);
}

// 64 list entries by one wave: lane `lane` holds v (or -1).  `bound` is the height from which a vertex is out of the phase (n in the
// preflow phase, 2n in the return phase).  Vertices that receive a push enter next[] under `stamp`, and so does v when it is still
// active behind its steps.
template <bool FRESH>
__device__ __forceinline__ void DischargeTile(const Ctx &c, int v, int bound, int stamp, int *next, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    int b = 0, e = 0, h = bound;
    if (v >= 0) {
        b = c.ro[v];
        e = c.ro[v + 1];
        h = Ld<true>(c.height + v);
    }
    const bool wide = e - b >= c.wave_min_row && e > b;
    for (int step = 0; step < c.discharge_steps; ++step) {  // (wave-uniform)
        const long long x = v >= 0 ? LdExcess(c.excess + v) : 0;
        const bool live = v >= 0 && x > 0 && h < bound;
        if (!__ballot(live)) break;
        unsigned long long best = ~0ull;
        if (live && !wide)
            for (int i = b; i < e; ++i) {
                const unsigned long long k = Candidate(c, i, t);
                best = k < best ? k : best;
            }
        unsigned long long todo = __ballot(live && wide);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
            unsigned long long part = ~0ull;
            for (int i = lb + lane; i < le; i += util::kWaveSize) {
                const unsigned long long k = Candidate(c, i, t);
                part = k < part ? k : part;
            }
            part = WaveMinKey(part);
            if (lane == leader) best = part;
            todo &= todo - 1;
        }
        int w = 0;
        bool pushed = false;
        if (live && best != ~0ull) {  // (no candidate: the arc its excess came over is not visible yet; the next step or round sees it)
            const int hw = static_cast<int>(best >> 32), i = static_cast<int>(best & 0xFFFFFFFFull);
            if (hw < h) {
                w = c.ci[i];
                const int r = Ld<true>(c.res + i);  // (>= what Candidate saw: only this lane lowers it)
                const int d = x < static_cast<long long>(r) ? static_cast<int>(x) : r;
                atomicSub(c.res + i, d);
                atomicAdd(c.res + c.mate[i], d);
                AddExcess(c.excess + v, -static_cast<long long>(d));
                AddExcess(c.excess + w, static_cast<long long>(d));
                ++t.pushes;
                pushed = w != c.src && w != c.sink;
            } else {
                h = hw + 1 < bound ? hw + 1 : bound;
                St<true>(c.height + v, h);
                ++t.relabels;
            }
        }
        const bool hit = pushed && atomicMax(c.mark + w, stamp) < stamp;
        Append<FRESH>(c, next, W_NEXT, hit, w, t);
    }
    bool again = false;
    if (v >= 0 && h < bound && LdExcess(c.excess + v) > 0) again = atomicMax(c.mark + v, stamp) < stamp;
    Append<FRESH>(c, next, W_NEXT, again, v, t);
}

template <bool FRESH>
__device__ __forceinline__ void DischargeList(const Ctx &c, const int *cur, int *next, long long count, int bound, int stamp, int tile,
                                              long long wave0, long long nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    if (count > c.nodes) count = c.nodes;
    for (long long from = wave0 * tile; from < count; from += nwaves * tile) {  // (wave-uniform)
        const long long i = from + lane;
        int v = -1;
        if (lane < tile && i < count) v = Ld<FRESH>(cur + i);
        DischargeTile<FRESH>(c, v, bound, stamp, next, t);
    }
}

static __global__ __launch_bounds__(kMaxflowThreads) void DischargeKernel(Ctx c, const int *cur, int *next, unsigned count, int bound, int stamp,
                                                                          int tile)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    DischargeList<false>(c, cur, next, count, bound, stamp, tile, wave0, nwaves, t);
    Flush(t, c, W_NEXT_ENTRIES);
}

// One workgroup runs round after round while the list is narrow, not empty, and the relabels stay under relabel_limit; at most
// lim.max_steps rounds per launch.  W_NEXT and W_NEXT_ENTRIES are 0 at entry and at exit.
static __global__ __launch_bounds__(kLoopThreads) void DischargeLoopKernel(Ctx c, int *list0, int *list1, Active a, Limits lim, int bound,
                                                                           unsigned relabel_limit, Active *d_active)
{
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    const int *words = reinterpret_cast<const int *>(c.words);
    Tally t;
    a.steps = 0;
    while (a.steps < lim.max_steps && a.count > 0 && Narrow(a.count, a.entries, lim) && (relabel_limit == kNever || a.relabels < relabel_limit)) {
        const int *cur = a.cur ? list1 : list0;
        int *next = a.cur ? list0 : list1;
        const int tile = TileFor(static_cast<long long>(a.count), nwaves, a.entries);
        DischargeList<true>(c, cur, next, a.count, bound, a.stamp + 1, tile, wave0, nwaves, t);
        Flush(t, c, W_NEXT_ENTRIES);
        __threadfence();
        __syncthreads();
        const unsigned count = static_cast<unsigned>(Ld<true>(words + W_NEXT));
        a.entries = static_cast<unsigned>(Ld<true>(words + W_NEXT_ENTRIES));
        a.relabels = static_cast<unsigned>(Ld<true>(words + W_RELABELS));
        a.count = count < static_cast<unsigned>(c.nodes) ? count : static_cast<unsigned>(c.nodes);
        a.cur ^= 1;
        ++a.stamp;
        ++a.steps;
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

// every arc out of src is saturated (one workgroup)
static __global__ void SaturateKernel(Ctx c)
{
    const int b = c.ro[c.src], e = c.ro[c.src + 1];
    long long out = 0;
    for (int i = b + static_cast<int>(threadIdx.x); i < e; i += static_cast<int>(blockDim.x)) {
        const int r = c.res[i];
        if (r <= 0) continue;
        c.res[i] = 0;
        atomicAdd(c.res + c.mate[i], r);
        AddExcess(c.excess + c.ci[i], r);
        out += r;
    }
    if (out) AddExcess(c.excess + c.src, -out);
}

// the active vertices of a phase, from scratch: excess > 0, height < bound, neither src nor sink
static __global__ void BuildActiveKernel(Ctx c, int *list, int bound)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (c.nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    Tally t;
    for (long long r = 0; r < rounds; ++r, v += stride) {  // (wave-uniform)
        const bool hit = v < c.nodes && v != c.src && v != c.sink && c.excess[v] > 0 && c.height[v] < bound;
        Append<false>(c, list, W_NEXT, hit, static_cast<int>(v), t);
    }
    Flush(t, c, W_NEXT_ENTRIES);
}

// ---------------- the cut ----------------

// side[] from the two searches, the sizes of the sides, and the certificate: excess outside src and sink, or sink reached from src
static __global__ void SidesKernel(Ctx c, const int *d_fwd, const int *d_bwd, unsigned char *d_side)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (c.nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned n0 = 0, n1 = 0, n2 = 0;
    bool bad = false;
    for (long long r = 0; r < rounds; ++r, v += stride) {
        if (v >= c.nodes) continue;
        const bool f = d_fwd[v] != kFar, g = d_bwd[v] != kFar;
        const int s = f ? 0 : (g ? 2 : 1);
        d_side[v] = static_cast<unsigned char>(s);
        n0 += s == 0;
        n1 += s == 1;
        n2 += s == 2;
        if (v == c.sink) bad |= f;
        else if (v != c.src) bad |= c.excess[v] != 0;
    }
    n0 = util::WaveSum(n0);
    n1 = util::WaveSum(n1);
    n2 = util::WaveSum(n2);
    const bool any_bad = __ballot(bad) != 0;
    if (util::LaneId() == 0) {
        if (n0) atomicAdd(c.counters + C_SIDE0, static_cast<unsigned long long>(n0));
        if (n1) atomicAdd(c.counters + C_SIDE1, static_cast<unsigned long long>(n1));
        if (n2) atomicAdd(c.counters + C_SIDE2, static_cast<unsigned long long>(n2));
        if (any_bad) c.words[W_FLAG] = 1u;
    }
}

// per pair: the net flow, the two cut bits, their counts and the capacity under each
static __global__ void PairsKernel(Ctx c, const int *d_a, const int *d_b, const int *d_pent, const int *d_cap, const unsigned char *d_side,
                                   long long pairs, int *d_flow, unsigned char *d_cut)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (pairs + stride - 1) / stride;
    long long p = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned k0 = 0, k1 = 0;
    unsigned long long s0 = 0, s1 = 0;
    for (long long r = 0; r < rounds; ++r, p += stride) {
        if (p >= pairs) continue;
        const int i = d_pent[p], j = c.mate[i];
        const int cab = d_cap[i], cba = d_cap[j];
        d_flow[p] = cab - c.res[i];
        const int sa = d_side[d_a[p]], sb = d_side[d_b[p]];
        unsigned long long c0 = 0, c1 = 0;
        if (sa == 0 && sb != 0) c0 = static_cast<unsigned long long>(cab);
        if (sb == 0 && sa != 0) c0 = static_cast<unsigned long long>(cba);
        if (sa != 2 && sb == 2) c1 = static_cast<unsigned long long>(cab);
        if (sb != 2 && sa == 2) c1 = static_cast<unsigned long long>(cba);
        d_cut[p] = static_cast<unsigned char>((c0 > 0 ? 1 : 0) | (c1 > 0 ? 2 : 0));
        k0 += c0 > 0;
        k1 += c1 > 0;
        s0 += c0;
        s1 += c1;
    }
    k0 = util::WaveSum(k0);
    k1 = util::WaveSum(k1);
    s0 = util::WaveSum(s0);
    s1 = util::WaveSum(s1);
    if (util::LaneId() == 0) {
        if (k0) atomicAdd(c.counters + C_CUT0, static_cast<unsigned long long>(k0));
        if (k1) atomicAdd(c.counters + C_CUT1, static_cast<unsigned long long>(k1));
        if (s0) atomicAdd(c.counters + C_CAP0, s0);
        if (s1) atomicAdd(c.counters + C_CAP1, s1);
    }
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

// every arc of the input adds its capacity (NULL: 1) to its entry of the residual CSR, in 64 bits; a negative one is bad.  The row
// of input entry e is found by bisection of the offsets (validated: non-decreasing, from 0 to edges).
static __global__ void AccumulateKernel(const int *d_row_offsets, const int *d_cols, const int *d_caps, int nodes, long long edges, const int *d_ro,
                                        const int *d_ci, unsigned long long *d_cap64, unsigned *d_bad)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        int lo = 0, hi = nodes;  // first index in [0, nodes] whose offset exceeds e
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (d_row_offsets[mid] > e) hi = mid; else lo = mid + 1;
        }
        const int u = lo - 1, w = d_cols[e];
        const int cap = d_caps ? d_caps[e] : 1;
        if (cap < 0) {
            *d_bad = 1u;
            continue;
        }
        if (u == w) continue;
        atomicAdd(d_cap64 + RowFind(d_ro, d_ci, u, w), static_cast<unsigned long long>(cap));
    }
}

// per pair (a, b): its two entries are each other's mates, and its two capacities must fit one int together
static __global__ void PairEntriesKernel(const int *d_a, const int *d_b, long long pairs, const int *d_ro, const int *d_ci,
                                         const unsigned long long *d_cap64, int *d_pent, int *d_mate, int *d_cap, int *d_cap_ab, int *d_cap_ba,
                                         unsigned *d_bad)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long p = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; p < pairs; p += stride) {
        const int a = d_a[p], b = d_b[p];
        const int i = RowFind(d_ro, d_ci, a, b), j = RowFind(d_ro, d_ci, b, a);
        d_pent[p] = i;
        d_mate[i] = j;
        d_mate[j] = i;
        const unsigned long long cab = d_cap64[i], cba = d_cap64[j];
        if (cab + cba > 0x7FFFFFFFull) {
            *d_bad = 1u;
            d_cap[i] = d_cap[j] = d_cap_ab[p] = d_cap_ba[p] = 0;
            continue;
        }
        d_cap[i] = d_cap_ab[p] = static_cast<int>(cab);
        d_cap[j] = d_cap_ba[p] = static_cast<int>(cba);
    }
}

// per input entry e = (u -> w): the pair's net flow in that direction goes to the direction's entries in CSR order, each filled to
// its capacity before the next; what the entries of row u before e with the same end hold comes off first
static __global__ void ArcFlowKernel(const int *d_row_offsets, const int *d_cols, const int *d_caps, int nodes, long long edges, const int *d_ro,
                                     const int *d_ci, const int *d_cap, const int *d_res, int *d_arc_flow)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        int lo = 0, hi = nodes;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (d_row_offsets[mid] > e) hi = mid; else lo = mid + 1;
        }
        const int u = lo - 1, w = d_cols[e];
        if (u == w) {
            d_arc_flow[e] = 0;
            continue;
        }
        const int i = RowFind(d_ro, d_ci, u, w);
        long long left = static_cast<long long>(d_cap[i]) - d_res[i];  // the net flow u -> w when positive
        for (long long k = d_row_offsets[u]; k < e && left > 0; ++k)
            if (d_cols[k] == w) left -= d_caps ? d_caps[k] : 1;
        const long long cap = d_caps ? d_caps[e] : 1;
        d_arc_flow[e] = static_cast<int>(left <= 0 ? 0 : (left < cap ? left : cap));
    }
}

}  // namespace maxflow
}  // namespace app
}  // namespace gunrock
