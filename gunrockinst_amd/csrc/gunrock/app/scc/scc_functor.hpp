// app/scc/scc_functor.hpp -- device kernels of the strongly connected components (trim, one pivot phase, colouring rounds).
//
// The reference snapshot has no app/scc (later Gunrock releases do); the shape follows this tree's primitives, k-core's most of
// all (app/kcore/kcore_functor.hpp: the queue-and-tail peel, the row walk, the one-workgroup device loop).  The CSR is read as a
// directed multigraph; Init (scc_problem.hpp) adds its transpose.
//
// Per vertex: region[] (>= 0: live, and every traversal stays among the vertices that hold the walker's value; the sign bit set:
// finished, a value no live vertex has), outdeg[] / indeg[] (live, same-region, non-loop entries of the two rows), colour[],
// mark[] (search bits, and the queued-once flag of a propagation sweep) and comp[] (the representative of a finished vertex: the
// vertex itself when trimmed, the pivot, or a colour root; the canonical pass turns it into the smallest id).
//
// The run is a sequence of STEPS, each a pass over the live list or over a range [head, tail) of a queue:
//   K_COUNT   the two counters of every live vertex of the list
//   K_SCAN    live vertices with a counter at 0 are claimed (the sign bit of region[]) and queued; the rest go to the other list
//   K_TRIM    a sub-round of the peel: a queued vertex takes one off the in-counter of every live successor and off the
//             out-counter of every live predecessor with a returning atomicSub; the lane that sees 1 claims and queues
//   K_PAIR    when the peel has run dry: v whose one live in-edge comes from u, whose one live in-edge comes from v (or the same
//             with out-edges), is a component of two; both are claimed and queued, and the peel goes on from them.  (Without it
//             a chain of two-cycles costs a colouring round per pair, each as many sweeps as the chain is long.)
//   K_PICK    the live vertex with the largest indeg * outdeg: per-wave maximum, one 64-bit atomicMax
//   K_FWD / K_BWD   a level of the search from the pivot on G / on the transpose: bit 1 / bit 2 of mark[]
//   K_SPLIT   mark 3: finished, comp = pivot; mark 1 and mark 2: regions 1 and 2; mark 0 stays in region 0
//   K_INIT    colour[v] = v, every live vertex queued
//   K_SWEEP   a queued vertex clears its flag, reads its colour and raises the smaller colours of its live successors by atomicMax
//             (behind a plain read that can only be stale low); the lane that raised one and flips its flag queues it
//   K_ROOTS   the live vertices with colour[v] == v are marked and queued
//   K_BACK    a level of the search from all roots on the transpose, among live vertices of the walker's colour
//   K_FINISH  marked: finished, comp = colour; the others: region = colour
// Which step follows is Advance(), a pure function of the state and of the shared words, run by the host after a read-back (the
// wide form: StepKernel, one launch per step) or by every thread of LoopKernel after a barrier (one workgroup looping on the
// device, agent-scope accesses on everything a step hands to the next: its CU's L1 is not refreshed by atomics that land in L2).
// No word is ever reset during a run: tails and counters only grow, and a step's positions are differences to the value its
// state recorded when its queue or list was opened.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace scc {

using oprtr::kLoopThreads;
using oprtr::Ld;
using oprtr::Limits;
using oprtr::St;
using oprtr::TileFor;

enum { SCC_AUTO = 0, SCC_ROUNDS = 1, SCC_DEVICE_LOOP = 2 };
enum { PHASE_TRIM = 0, PHASE_PIVOT = 1, PHASE_COLOUR = 2 };

constexpr int kSccThreads = 256;
constexpr int kWaveUnroll = 4;             // chunks of 64 row entries a wave keeps in flight per step of a long row
constexpr int kDone = static_cast<int>(0x80000000u);  // region[]: finished
constexpr unsigned kTraceRows = 1u << 16;  // phases recorded (a run has at most 2 * nodes + 3)

// the words the kernels and the host share: none is reset during a run
enum {
    W_TAIL = 0,      // queue tickets handed out
    W_LIST,          // list tickets handed out
    W_ENTRIES,       // row entries (both rows) of the vertices queued so far, modulo 2^32
    W_LIST_ENTRIES,  // the same for the vertices listed
    W_FINISHED,      // vertices finished
    W_SPARE,
    W_PIVOT,         // 64-bit: ((indeg * outdeg, clipped) + 1) << 32 | vertex
    W_PIVOT_HI,
    W_COUNT = 8
};

enum { K_COUNT = 0, K_SCAN, K_TRIM, K_PICK, K_FWD, K_BWD, K_SPLIT, K_INIT, K_SWEEP, K_ROOTS, K_BACK, K_FINISH, K_PAIR, K_DONE, K_STUCK };
// (K_STUCK: a colouring round that finished nothing, or more sweeps than vertices: a defect, reported and not looped on)

struct Ctx {
    const int *ro, *ci;      // G
    const int *iro, *ici;    // its transpose
    int *region, *outdeg, *indeg, *colour, *mark, *comp;
    int *list[2];            // the live list, rebuilt from one into the other
    int *queue[2];
    unsigned *words;
    unsigned long long *reads;  // row entries walked
    int *trace_kind;            // one row per phase: its kind,
    unsigned *trace_finished;   // the vertices finished when it began,
    unsigned long long *trace_clock;  // the constant-rate counter then
    int nodes;
    int wave_min_row;
};

// what the next step is and where its input lies; the host and LoopKernel carry the same
struct State {
    int kind;
    int list_buf;            // -1: every vertex
    unsigned list_len, list_entries;
    unsigned list_base, lentries_base;  // W_LIST / W_LIST_ENTRIES when K_SCAN's output list was opened
    int q_buf;               // the queue that holds [head, tail); K_SWEEP appends to the other one, the rest to the same
    unsigned head, tail;
    unsigned q_base;         // W_TAIL when the queue being appended to was opened
    unsigned entries_seen;   // W_ENTRIES when the last step ended
    unsigned step_entries;   // row entries of [head, tail)
    int seed;                // >= 0: the search starts here and the queue is empty
    int pivot;
    int pivot_pending;       // the pivot phase is still to come
    int trim;
    int pairs;               // K_PAIR runs when the peel is dry (needs trim: the counters are the peel's)
    int stamp;               // this step opens a phase of this kind + 1 (0: it does not)
    unsigned trace_at;
    unsigned finished;       // W_FINISHED when the last step ended
    unsigned phase_finished; // ... when the phase began
    unsigned round_sweeps;   // sweeps of this colouring round
    unsigned trimmed, trim_rounds, pivot_component, colour_rounds, sweeps, bfs_levels;
};

struct Tally {
    unsigned entries = 0;   // row entries of the vertices this lane queued
    unsigned lentries = 0;  // ... listed
    unsigned reads = 0;     // row entries this lane walked
    unsigned finished = 0;  // vertices this lane finished outside Append
};

__device__ __forceinline__ void Flush(Tally &t, const Ctx &c)
{
    const unsigned entries = util::WaveSum(t.entries), lentries = util::WaveSum(t.lentries), finished = util::WaveSum(t.finished);
    const unsigned long long reads = util::WaveSum(static_cast<unsigned long long>(t.reads));
    if (util::LaneId() == 0) {
        if (entries) atomicAdd(c.words + W_ENTRIES, entries);
        if (lentries) atomicAdd(c.words + W_LIST_ENTRIES, lentries);
        if (finished) atomicAdd(c.words + W_FINISHED, finished);
        if (reads) atomicAdd(c.reads, reads);
    }
    t = Tally();
}

__device__ __forceinline__ unsigned RowEntries(const Ctx &c, int u) { return static_cast<unsigned>(c.ro[u + 1] - c.ro[u] + c.iro[u + 1] - c.iro[u]); }

// All lanes of the wave call; the lanes with `hit` append u: one atomic on the ticket word per wave.  A vertex is appended at most
// once between two openings of a queue or a list, so a position stays under `nodes`, the length of both; the test is there so
// that a mistake elsewhere cannot turn into a store outside the buffer.
template <bool FRESH, bool FINISHES, bool LIST>
__device__ __forceinline__ void Append(const Ctx &c, bool hit, int u, int *d_out, unsigned base, Tally &t)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned pos = oprtr::WaveTicket(c.words + (LIST ? W_LIST : W_TAIL), mask, FINISHES ? c.words + W_FINISHED : nullptr) - base;
    if (hit) {
        if (pos < static_cast<unsigned>(c.nodes)) St<FRESH>(d_out + pos, u);
        if (LIST) t.lentries += RowEntries(c, u);
        else t.entries += RowEntries(c, u);
    }
}

// ---------------- what a walker does with one row entry: (v, key, val) describe the row's vertex ----------------

// one off the counter of a live vertex of v's region; the lane that empties it claims the vertex
template <bool FRESH>
struct TrimOp {
    int *counter;
    __device__ __forceinline__ bool operator()(const Ctx &c, int v, int key, int /*val*/, int u) const
    {
        if (u == v || Ld<FRESH>(c.region + u) != key) return false;  // (a stale read is only ever live: the atomics below sort it out)
        if (atomicSub(counter + u, 1) != 1) return false;
        if (atomicOr(c.region + u, kDone) < 0) return false;         // the other counter emptied first
        St<FRESH>(c.comp + u, u);
        return true;
    }
};

// the search bit of a live vertex that holds the walker's key (its region, or its colour)
template <bool FRESH, bool BY_COLOUR>
struct SearchOp {
    int bit;
    __device__ __forceinline__ bool operator()(const Ctx &c, int /*v*/, int key, int /*val*/, int u) const
    {
        const int r = Ld<FRESH>(c.region + u);
        if (r < 0) return false;
        if ((BY_COLOUR ? Ld<FRESH>(c.colour + u) : r) != key) return false;
        if (Ld<FRESH>(c.mark + u) & bit) return false;
        return !(atomicOr(c.mark + u, bit) & bit);
    }
};

// val = the walker's colour; a successor it raises is queued once per sweep
template <bool FRESH>
struct RaiseOp {
    __device__ __forceinline__ bool operator()(const Ctx &c, int v, int key, int val, int u) const
    {
        if (u == v || Ld<FRESH>(c.region + u) != key) return false;
        if (Ld<FRESH>(c.colour + u) >= val) return false;  // colours only rise: a stale read is low and the atomic decides
        if (atomicMax(c.colour + u, val) >= val) return false;
        return atomicExch(c.mark + u, 1) == 0;
    }
};

// 64 vertices by one wave: lane `lane` holds v (or -1) with its key and value.  Rows shorter than wave_min_row by their lane, the
// others by the wave, kWaveUnroll chunks of 64 entries at a time; both loops are wave-uniform, so a step's appends are one
// ballot and one atomic per wave.
template <bool FRESH, bool FINISHES, typename Op>
__device__ __forceinline__ void WalkTile(const Ctx &c, const int *ro, const int *ci, int v, int key, int val, const Op &op, int *d_out,
                                         unsigned base, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    int b = 0, e = 0;
    if (v >= 0) {
        b = ro[v];
        e = ro[v + 1];
    }
    const bool wide = e - b >= c.wave_min_row && e > b;
    int longest = wide ? 0 : e - b;
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const int other = __shfl_xor(longest, o, util::kWaveSize);
        longest = other > longest ? other : longest;
    }
    for (int j = 0; j < longest; ++j) {  // (wave-uniform)
        int u = 0;
        bool hit = false;
        if (!wide && b + j < e) {
            u = ci[b + j];
            ++t.reads;
            hit = op(c, v, key, val, u);
        }
        Append<FRESH, FINISHES, false>(c, hit, u, d_out, base, t);
    }
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
        const int lv = __shfl(v, leader, util::kWaveSize), lkey = __shfl(key, leader, util::kWaveSize), lval = __shfl(val, leader, util::kWaveSize);
        for (int from = lb; from < le; from += util::kWaveSize * kWaveUnroll) {  // (wave-uniform)
            int us[kWaveUnroll];
            bool hits[kWaveUnroll];
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) {
                const int i = from + j * util::kWaveSize + lane;
                us[j] = i < le ? ci[i] : -1;
            }
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) {
                hits[j] = false;
                if (us[j] >= 0) {
                    ++t.reads;
                    hits[j] = op(c, lv, lkey, lval, us[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < kWaveUnroll; ++j) Append<FRESH, FINISHES, false>(c, hits[j], us[j], d_out, base, t);
        }
        todo &= todo - 1;
    }
}

// the live, same-region, non-loop entries of v's row; lane `lane` gets its own vertex's count
template <bool FRESH>
__device__ __forceinline__ int CountTile(const Ctx &c, const int *ro, const int *ci, int v, int key, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    int b = 0, e = 0, count = 0;
    if (v >= 0) {
        b = ro[v];
        e = ro[v + 1];
    }
    const bool wide = e - b >= c.wave_min_row && e > b;
    if (!wide)
        for (int i = b; i < e; ++i) {
            const int u = ci[i];
            ++t.reads;
            if (u != v && Ld<FRESH>(c.region + u) == key) ++count;
        }
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize);
        const int lv = __shfl(v, leader, util::kWaveSize), lkey = __shfl(key, leader, util::kWaveSize);
        int part = 0;
        for (int i = lb + lane; i < le; i += util::kWaveSize) {
            const int u = ci[i];
            ++t.reads;
            if (u != lv && Ld<FRESH>(c.region + u) == lkey) ++part;
        }
        part = util::WaveSum(part);
        if (lane == leader) count = part;
        todo &= todo - 1;
    }
    return count;
}

// the one live, same-region, non-loop entry of v's row (the caller has seen its counter at 1); -1 when a claim of this step took it
template <bool FRESH>
__device__ __forceinline__ int OnlyLive(const Ctx &c, const int *ro, const int *ci, int v, int key, Tally &t)
{
    for (int i = ro[v], e = ro[v + 1]; i < e; ++i) {
        const int u = ci[i];
        ++t.reads;
        if (u != v && Ld<FRESH>(c.region + u) == key) return u;
    }
    return -1;
}

// v's partner in a component of two by the rule above on one pair of arrays (the in-rows and in-counters, or the out ones)
template <bool FRESH>
__device__ __forceinline__ int MateOf(const Ctx &c, const int *ro, const int *ci, const int *counter, int v, int key, Tally &t)
{
    if (Ld<FRESH>(counter + v) != 1) return -1;
    const int u = OnlyLive<FRESH>(c, ro, ci, v, key, t);
    if (u < 0 || Ld<FRESH>(counter + u) != 1) return -1;
    return OnlyLive<FRESH>(c, ro, ci, u, key, t) == v ? u : -1;
}

// ---------------- one step ----------------

// the steps that pass over the live list; the others take a range of a queue
__host__ __device__ __forceinline__ bool ByList(int kind)
{
    return kind == K_COUNT || kind == K_SCAN || kind == K_PICK || kind == K_SPLIT || kind == K_INIT || kind == K_ROOTS || kind == K_FINISH || kind == K_PAIR;
}

template <bool FRESH>
__device__ __forceinline__ void RunStep(const Ctx &c, const State &s, int kind, int tile, long long wave0, long long nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    if (s.stamp && wave0 == 0 && lane == 0 && s.trace_at < kTraceRows) {
        c.trace_kind[s.trace_at] = s.stamp - 1;
        c.trace_finished[s.trace_at] = s.finished;
        c.trace_clock[s.trace_at] = wall_clock64();
    }
    if (ByList(kind)) {
        const int *list = s.list_buf < 0 ? nullptr : c.list[s.list_buf];
        int *list_out = c.list[s.list_buf == 0 ? 1 : 0];
        unsigned long long best = 0;
        for (long long from = wave0 * util::kWaveSize; from < s.list_len; from += nwaves * util::kWaveSize) {  // (wave-uniform)
            const long long i = from + lane;
            int v = -1, r = kDone;
            if (i < s.list_len) {
                v = list ? Ld<FRESH>(list + i) : static_cast<int>(i);
                r = Ld<FRESH>(c.region + v);
            }
            const bool live = r >= 0;
            if (kind == K_COUNT) {
                const int out = CountTile<FRESH>(c, c.ro, c.ci, live ? v : -1, r, t);
                const int in = CountTile<FRESH>(c, c.iro, c.ici, live ? v : -1, r, t);
                if (live) {
                    St<FRESH>(c.outdeg + v, out);
                    St<FRESH>(c.indeg + v, in);
                }
            } else if (kind == K_SCAN) {
                bool hit = false;
                if (live && s.trim && (Ld<FRESH>(c.outdeg + v) == 0 || Ld<FRESH>(c.indeg + v) == 0)) {
                    St<FRESH>(c.region + v, r | kDone);  // (nobody else claims during this step)
                    St<FRESH>(c.comp + v, v);
                    hit = true;
                }
                Append<FRESH, true, false>(c, hit, v, c.queue[s.q_buf], s.q_base, t);
                Append<FRESH, false, true>(c, live && !hit, v, list_out, s.list_base, t);
            } else if (kind == K_PAIR) {
                // the counters are the peel's and do not move in this step; regions only lose vertices, so a pair seen here is
                // one.  A vertex has at most one partner (its one in-edge, or its one out-edge, is the partner's), and the
                // smaller of the two acts for both.
                int mate = -1;
                if (live) {
                    mate = MateOf<FRESH>(c, c.iro, c.ici, c.indeg, v, r, t);
                    if (mate < 0) mate = MateOf<FRESH>(c, c.ro, c.ci, c.outdeg, v, r, t);
                }
                const bool hit = mate >= 0 && v < mate;
                if (hit) {
                    St<FRESH>(c.region + v, r | kDone);
                    St<FRESH>(c.region + mate, r | kDone);
                    St<FRESH>(c.comp + v, v);
                    St<FRESH>(c.comp + mate, v);
                }
                Append<FRESH, true, false>(c, hit, v, c.queue[s.q_buf], s.q_base, t);
                Append<FRESH, true, false>(c, hit, mate, c.queue[s.q_buf], s.q_base, t);
            } else if (kind == K_PICK) {
                if (live) {
                    unsigned long long weight = static_cast<unsigned long long>(Ld<FRESH>(c.outdeg + v)) * static_cast<unsigned long long>(Ld<FRESH>(c.indeg + v));
                    if (weight > 0xFFFFFFFEull) weight = 0xFFFFFFFEull;
                    const unsigned long long key = ((weight + 1ull) << 32) | static_cast<unsigned>(v);
                    best = key > best ? key : best;
                }
            } else if (kind == K_SPLIT) {
                const int m = live ? Ld<FRESH>(c.mark + v) : 0;
                if (m) {
                    St<FRESH>(c.mark + v, 0);
                    if (m == 3) {
                        St<FRESH>(c.comp + v, s.pivot);
                        St<FRESH>(c.region + v, r | kDone);
                        ++t.finished;
                    } else {
                        St<FRESH>(c.region + v, m);
                    }
                }
            } else if (kind == K_INIT) {
                if (live) {
                    St<FRESH>(c.colour + v, v);
                    St<FRESH>(c.mark + v, 1);
                }
                Append<FRESH, false, false>(c, live, v, c.queue[s.q_buf], s.q_base, t);
            } else if (kind == K_ROOTS) {
                const bool root = live && Ld<FRESH>(c.colour + v) == v;
                if (root) St<FRESH>(c.mark + v, 1);
                Append<FRESH, false, false>(c, root, v, c.queue[s.q_buf], s.q_base, t);
            } else {  // K_FINISH
                if (live) {
                    const int colour = Ld<FRESH>(c.colour + v);
                    if (Ld<FRESH>(c.mark + v)) {
                        St<FRESH>(c.mark + v, 0);
                        St<FRESH>(c.comp + v, colour);
                        St<FRESH>(c.region + v, r | kDone);
                        ++t.finished;
                    } else {
                        St<FRESH>(c.region + v, colour);
                    }
                }
            }
        }
        if (kind == K_PICK) {
            for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(best, o, util::kWaveSize);
                best = other > best ? other : best;
            }
            if (lane == 0 && best) atomicMax(reinterpret_cast<unsigned long long *>(c.words + W_PIVOT), best);
        }
        return;
    }

    // a range of a queue, `tile` entries per wave at a time (or the seed of a search, alone)
    const int *in = c.queue[s.q_buf];
    int *out = c.queue[kind == K_SWEEP ? (s.q_buf ^ 1) : s.q_buf];
    const bool seeded = (kind == K_FWD || kind == K_BWD) && s.seed >= 0;
    const long long head = seeded ? 0 : s.head, tail = seeded ? 1 : (s.tail < static_cast<unsigned>(c.nodes) ? s.tail : c.nodes);
    for (long long from = head + wave0 * tile; from < tail; from += nwaves * tile) {  // (wave-uniform)
        const long long i = from + lane;
        int v = -1;
        if (lane < tile && i < tail) v = seeded ? s.seed : Ld<FRESH>(in + i);
        if (kind == K_TRIM) {
            const int key = v >= 0 ? (Ld<FRESH>(c.region + v) & ~kDone) : 0;
            WalkTile<FRESH, true>(c, c.ro, c.ci, v, key, 0, TrimOp<FRESH>{c.indeg}, out, s.q_base, t);
            WalkTile<FRESH, true>(c, c.iro, c.ici, v, key, 0, TrimOp<FRESH>{c.outdeg}, out, s.q_base, t);
        } else if (kind == K_FWD || kind == K_BWD) {
            const int bit = kind == K_FWD ? 1 : 2;
            if (seeded && v >= 0) atomicOr(c.mark + v, bit);
            const int key = v >= 0 ? Ld<FRESH>(c.region + v) : 0;
            if (kind == K_FWD) WalkTile<FRESH, false>(c, c.ro, c.ci, v, key, 0, SearchOp<FRESH, false>{bit}, out, s.q_base, t);
            else WalkTile<FRESH, false>(c, c.iro, c.ici, v, key, 0, SearchOp<FRESH, false>{bit}, out, s.q_base, t);
        } else if (kind == K_SWEEP) {
            int key = 0, val = 0;
            if (v >= 0) {
                // the flag goes down before the colour is read: whoever raises the colour after this read finds the flag down
                // and queues v again (the exchange is an acquire, so the read cannot pass it); the read is an agent-scope one in
                // the wide form too, where another CU may have raised the colour during this launch
                __hip_atomic_exchange(c.mark + v, 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                val = Ld<true>(c.colour + v);
                key = Ld<FRESH>(c.region + v);
            }
            WalkTile<FRESH, false>(c, c.ro, c.ci, v, key, val, RaiseOp<FRESH>{}, out, s.q_base, t);
        } else {  // K_BACK
            const int key = v >= 0 ? Ld<FRESH>(c.colour + v) : 0;
            WalkTile<FRESH, false>(c, c.iro, c.ici, v, key, 0, SearchOp<FRESH, true>{1}, out, s.q_base, t);
        }
    }
}

// ---------------- which step follows ----------------

__host__ __device__ __forceinline__ void OpenQueue(State &s, const unsigned *w)
{
    s.q_buf = 0;
    s.q_base = w[W_TAIL];
    s.head = s.tail = 0;
}

__host__ __device__ __forceinline__ void OpenPhase(State &s, int phase)
{
    s.stamp = phase + 1;
    s.phase_finished = s.finished;
}

// the trim phase: the counters when something reads them, then the scan (which also rebuilds the live list)
__host__ __device__ __forceinline__ void EnterTrim(State &s, const unsigned *w)
{
    if (s.trim) OpenPhase(s, PHASE_TRIM);
    s.kind = s.trim || s.pivot_pending ? K_COUNT : K_SCAN;
    s.list_base = w[W_LIST];
    s.lentries_base = w[W_LIST_ENTRIES];
    OpenQueue(s, w);
}

__host__ __device__ __forceinline__ void LeaveTrim(State &s, const unsigned *w, unsigned nodes)
{
    if (s.trim) s.trimmed += s.finished - s.phase_finished;
    if (s.finished >= nodes) {
        s.kind = K_DONE;
    } else if (s.pivot_pending) {
        OpenPhase(s, PHASE_PIVOT);
        s.kind = K_PICK;
    } else {
        OpenPhase(s, PHASE_COLOUR);
        s.round_sweeps = 0;
        s.kind = K_INIT;
        OpenQueue(s, w);
    }
}

// [head, tail) becomes what the step appended; false when that is nothing
__host__ __device__ __forceinline__ bool NextRange(State &s, const unsigned *w)
{
    s.head = s.seed >= 0 ? 0 : s.tail;
    s.seed = -1;
    s.tail = w[W_TAIL] - s.q_base;
    return s.head < s.tail;
}

__host__ __device__ __forceinline__ State StartState(unsigned nodes, unsigned long long entries, bool trim, bool pairs, bool pivot_phase, const unsigned *w)
{
    State s = {};
    s.list_buf = -1;
    s.list_len = nodes;
    s.list_entries = entries > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<unsigned>(entries);
    s.seed = -1;
    s.pivot = -1;
    s.trim = trim ? 1 : 0;
    s.pairs = pairs ? 1 : 0;
    s.pivot_pending = pivot_phase ? 1 : 0;
    s.entries_seen = w[W_ENTRIES];
    s.finished = w[W_FINISHED];
    EnterTrim(s, w);
    return s;
}

// the step s.kind has run and w holds the words after it
__host__ __device__ __forceinline__ void Advance(State &s, const unsigned *w, unsigned nodes)
{
    if (s.stamp) ++s.trace_at;
    s.stamp = 0;
    s.finished = w[W_FINISHED];
    s.step_entries = w[W_ENTRIES] - s.entries_seen;
    s.entries_seen = w[W_ENTRIES];
    switch (s.kind) {
        case K_COUNT:
            s.kind = K_SCAN;
            break;
        case K_SCAN:
            s.list_buf = s.list_buf == 0 ? 1 : 0;
            s.list_len = w[W_LIST] - s.list_base;
            s.list_entries = w[W_LIST_ENTRIES] - s.lentries_base;
            if (NextRange(s, w)) s.kind = K_TRIM;
            else if (s.trim && s.pairs && s.finished < nodes) s.kind = K_PAIR;
            else LeaveTrim(s, w, nodes);
            break;
        case K_TRIM:
            ++s.trim_rounds;
            if (!NextRange(s, w)) {
                if (s.pairs && s.finished < nodes) s.kind = K_PAIR;
                else LeaveTrim(s, w, nodes);
            }
            break;
        case K_PAIR:
            if (NextRange(s, w)) s.kind = K_TRIM;
            else LeaveTrim(s, w, nodes);
            break;
        case K_PICK:
            s.pivot = static_cast<int>(w[W_PIVOT]);
            s.seed = s.pivot;
            s.kind = K_FWD;
            OpenQueue(s, w);
            break;
        case K_FWD:
            ++s.bfs_levels;
            if (!NextRange(s, w)) {
                s.seed = s.pivot;
                s.kind = K_BWD;
                OpenQueue(s, w);
            }
            break;
        case K_BWD:
            ++s.bfs_levels;
            if (!NextRange(s, w)) s.kind = K_SPLIT;
            break;
        case K_SPLIT:
            s.pivot_component = s.finished - s.phase_finished;
            s.pivot_pending = 0;
            if (s.finished >= nodes) s.kind = K_DONE;
            else EnterTrim(s, w);
            break;
        case K_INIT:
            if (NextRange(s, w)) {
                s.kind = K_SWEEP;
                s.q_base = w[W_TAIL];  // (of the other queue)
            } else {
                s.kind = K_DONE;  // (nothing is live: LeaveTrim has seen that)
            }
            break;
        case K_SWEEP:
            ++s.sweeps;
            if (++s.round_sweeps > nodes) {  // (a colour travels along a simple path: at most nodes - 1 sweeps raise anything)
                s.kind = K_STUCK;
                break;
            }
            s.q_buf ^= 1;
            s.head = 0;
            s.tail = w[W_TAIL] - s.q_base;
            s.q_base = w[W_TAIL];
            if (s.tail == 0) {
                s.kind = K_ROOTS;
                OpenQueue(s, w);
            }
            break;
        case K_ROOTS:
            s.kind = NextRange(s, w) ? K_BACK : K_FINISH;
            break;
        case K_BACK:
            ++s.bfs_levels;
            if (!NextRange(s, w)) s.kind = K_FINISH;
            break;
        case K_FINISH:
            ++s.colour_rounds;
            if (s.finished == s.phase_finished) s.kind = K_STUCK;  // (the largest live id is a root: a round finishes its component)
            else if (s.finished >= nodes) s.kind = K_DONE;
            else EnterTrim(s, w);
            break;
        default:
            break;
    }
}

// a step one workgroup takes: a list up to max_list (the counting step walks its rows, so those count too), a range up to max_list
// whose rows hold up to max_entries
__host__ __device__ __forceinline__ bool Narrow(const State &s, const Limits &lim)
{
    if (ByList(s.kind)) return s.list_len <= lim.max_list && (s.kind != K_COUNT || s.list_entries <= lim.max_entries);
    if (s.seed >= 0) return true;
    return oprtr::Narrow(static_cast<long long>(s.tail - s.head), s.step_entries, lim);
}

// ---------------- the wide form and the device loop ----------------

template <int KIND>
static __global__ __launch_bounds__(kSccThreads) void StepKernel(Ctx c, State s, int tile)
{
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    RunStep<false>(c, s, KIND, tile, wave0, nwaves, t);
    Flush(t, c);
}

// One workgroup.  Every step ends in a barrier behind a fence, the words are read with agent-scope loads by every thread, and a
// second barrier keeps the next step's atomics behind those reads.  Uniform control flow: Advance() and Narrow() see the same
// values in every thread.
static __global__ __launch_bounds__(kLoopThreads) void LoopKernel(Ctx c, State s, Limits lim, State *d_state)
{
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    Tally t;
    for (int step = 0; step < lim.max_steps && s.kind < K_DONE && Narrow(s, lim); ++step) {
        const int tile = ByList(s.kind) ? util::kWaveSize : TileFor(static_cast<long long>(s.tail - s.head), nwaves, s.step_entries);
        switch (s.kind) {  // (a constant kind per call: each step is compiled on its own)
            case K_COUNT: RunStep<true>(c, s, K_COUNT, tile, wave0, nwaves, t); break;
            case K_SCAN: RunStep<true>(c, s, K_SCAN, tile, wave0, nwaves, t); break;
            case K_TRIM: RunStep<true>(c, s, K_TRIM, tile, wave0, nwaves, t); break;
            case K_PICK: RunStep<true>(c, s, K_PICK, tile, wave0, nwaves, t); break;
            case K_FWD: RunStep<true>(c, s, K_FWD, tile, wave0, nwaves, t); break;
            case K_BWD: RunStep<true>(c, s, K_BWD, tile, wave0, nwaves, t); break;
            case K_SPLIT: RunStep<true>(c, s, K_SPLIT, tile, wave0, nwaves, t); break;
            case K_INIT: RunStep<true>(c, s, K_INIT, tile, wave0, nwaves, t); break;
            case K_SWEEP: RunStep<true>(c, s, K_SWEEP, tile, wave0, nwaves, t); break;
            case K_ROOTS: RunStep<true>(c, s, K_ROOTS, tile, wave0, nwaves, t); break;
            case K_BACK: RunStep<true>(c, s, K_BACK, tile, wave0, nwaves, t); break;
            case K_PAIR: RunStep<true>(c, s, K_PAIR, tile, wave0, nwaves, t); break;
            default: RunStep<true>(c, s, K_FINISH, tile, wave0, nwaves, t); break;
        }
        Flush(t, c);
        __threadfence();
        __syncthreads();
        unsigned w[W_COUNT];
#pragma unroll
        for (int i = 0; i < W_COUNT; ++i) w[i] = static_cast<unsigned>(Ld<true>(reinterpret_cast<const int *>(c.words) + i));
        Advance(s, w, static_cast<unsigned>(c.nodes));
        __syncthreads();
    }
    if (threadIdx.x == 0) *d_state = s;
}

// ---------------- after the run ----------------

static __global__ void IotaKernel(int *d_out, long long nodes)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) d_out[v] = static_cast<int>(v);
}

// ADD: d_of[d_rep[v]] += 1, else d_of[d_rep[v]] = min(.., v): the lanes of a wave that hold the same representative send one
// atomic (the giant component of an R-MAT graph is one word)
template <bool ADD>
static __global__ void MergeKernel(const int *d_rep, long long nodes, int *d_of)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long rounds = (nodes + stride - 1) / stride;
    long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (long long r = 0; r < rounds; ++r, v += stride) {  // (wave-uniform)
        const int rep = v < nodes ? d_rep[v] : -1;
        unsigned long long todo = __ballot(rep >= 0);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int value = __shfl(rep, leader, util::kWaveSize);
            const unsigned long long same = __ballot(rep == value);
            if (static_cast<int>(util::LaneId()) == leader) {
                if (ADD) atomicAdd(d_of + value, __popcll(same));
                else atomicMin(d_of + value, static_cast<int>(v));  // (the leader is the lowest lane: the smallest v of the group)
            }
            todo &= ~same;
        }
    }
}

// d_out[v] = d_of[d_rep[v]] (d_out may be d_rep)
static __global__ void GatherKernel(const int *d_rep, long long nodes, const int *d_of, int *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int rep = d_rep[v];
        d_out[v] = rep >= 0 ? d_of[rep] : -1;  // (every vertex has a representative after a run)
    }
}

// d_out[0] += the components (comp[v] == v), d_out[1] += those of one vertex, d_out[2] = max of size << 32 | ~root
static __global__ void SummaryKernel(const int *d_comp, const int *d_size, long long nodes, unsigned long long *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned long long components = 0, trivial = 0, best = 0;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        if (d_comp[v] != v) continue;
        ++components;
        const unsigned size = static_cast<unsigned>(d_size[v]);
        if (size == 1) ++trivial;
        const unsigned long long key = (static_cast<unsigned long long>(size) << 32) | (0xFFFFFFFFu - static_cast<unsigned>(v));
        best = key > best ? key : best;
    }
    components = util::WaveSum(components);
    trivial = util::WaveSum(trivial);
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, util::kWaveSize);
        best = other > best ? other : best;
    }
    if (util::LaneId() == 0) {
        if (components) atomicAdd(d_out, components);
        if (trivial) atomicAdd(d_out + 1, trivial);
        if (best) atomicMax(d_out + 2, best);
    }
}

// one key per CSR entry u -> v: comp[u] << col_bits | comp[v], or the sentinel inside a component.  The row of entry e is found by
// bisection of the offsets (validated: non-decreasing, from 0 to edges).
static __global__ void CondensationKeysKernel(const int *d_ro, const int *d_ci, const int *d_comp, int nodes, long long edges, int col_bits,
                                              unsigned long long sentinel, unsigned long long *d_keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        int lo = 0, hi = nodes;  // the last row with ro[row] <= e
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (d_ro[mid] <= e) lo = mid;
            else hi = mid;
        }
        const unsigned a = static_cast<unsigned>(d_comp[lo]), b = static_cast<unsigned>(d_comp[d_ci[e]]);
        d_keys[e] = a == b ? sentinel : (static_cast<unsigned long long>(a) << col_bits) | b;
    }
}

static __global__ void CondensationEmitKernel(const unsigned long long *d_keys, const unsigned *d_keep, const unsigned long long *d_pos, long long count,
                                              int col_bits, long long max_edges, int *d_from, int *d_to)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (!d_keep[i]) continue;
        const long long pos = static_cast<long long>(d_pos[i]);
        if (pos >= max_edges) continue;
        d_from[pos] = static_cast<int>(d_keys[i] >> col_bits);
        d_to[pos] = static_cast<int>(d_keys[i] & mask);
    }
}

}  // namespace scc
}  // namespace app
}  // namespace gunrock
