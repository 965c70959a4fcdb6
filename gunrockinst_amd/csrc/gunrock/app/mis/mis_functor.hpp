// app/mis/mis_functor.hpp -- device kernels of the maximal independent set / greedy colourings.
//
// Stands for the reference's MIS functor (gunrock/app/mis/mis_functor.cuh:33-120): a MAX-reducing advance gives every
// uncoloured vertex the largest label among its uncoloured neighbours, and CondFilter (:84-89) colours the vertex with
// `iteration + 1` when its own label is at least that.  Here the three results are defined by equations over the strict key
// order key(v) = (prio(v), v) and H(v) = the neighbours of v with a larger key:
//   SET              ids[v] = 1 iff no u in H(v) has ids[u] = 1                  (the lexicographically first maximal independent set)
//   COLOR_ROUNDS     ids[v] = 1 + max(ids[u], u in H(v)), 1 when H(v) is empty   (the reference's schedule run to the end)
//   COLOR_FIRST_FIT  ids[v] = the smallest positive integer not among ids[u], u in H(v)   (Jones-Plassmann)
// Departures from the reference: ties cannot occur (its `>=` lets two adjacent vertices with equal labels take one colour);
// there is no iteration cap and no -1 remains; the label order is a seeded hash or the caller's, not std::random_shuffle.
//
// A value, once written, is final, and a vertex only needs its larger-keyed neighbours.  So a sweep reads the state table
// while other lanes, waves and workgroups write it, fresh or stale, and the result does not change: no double buffer, no
// snapshot per round.  One sweep over the worklist of undecided vertices (SweepKernel):
//   * a lane per vertex; rows with at most kLaneRow entries left are walked by their lane, longer ones by the whole wave, four
//     chunks of 64 entries in flight per step (R-MAT hubs sit at the low ids: DESIGN.md 3.8);
//   * the hashed key of a neighbour is computed in registers, the caller's priority is gathered;
//   * the state table is a byte per vertex for the set (0 undecided, 1 in, 2 out) and the int32 result for the colourings
//     (0 undecided);
//   * the colourings stop at the first undecided member of H(v) and keep a cursor (its position in the row, plus the running
//     maximum / the colours seen in a 64-wide window), so a vertex blocked for hundreds of rounds reads every row entry once.
//     The set walks on past undecided entries, because one member of H(v) in the set decides v whatever the others do (5-6
//     rounds instead of the chain depth); its cursor skips the prefix that is already out;
//   * first-fit keeps the exact forbidden set of the colours [base, base + 64) as one 64-bit word; when the window is full at
//     the end of the row (all of H(v) is decided by then) it moves up by 64 and the row is scanned again;
//   * survivors are appended to the next worklist, one atomic per wave.
// TailKernel is the same walk inside a bounded device loop for the long thin tail: a window of the worklist (sorted by
// descending key), one vertex per thread kept in registers, state read and written with agent-scope accesses (another CU's
// L1 and another XCD's L2 are not coherent with plain ones), nobody waits for anybody: a wave leaves when its vertices are
// decided or after max_sweeps, and the host launches again while something is left.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace mis {

enum Mode { MIS_SET = 0, MIS_COLOR_ROUNDS = 1, MIS_COLOR_FIRST_FIT = 2 };

constexpr int kLaneRow = 32;      // rows with more entries left than this are walked by the whole wave
constexpr int kSweepThreads = 256;
constexpr int kWaveUnroll = 4;    // chunks of 64 row entries a wave keeps in flight per step of a long row

using util::Fmix32;

struct Graph {
    const int *d_row_offsets;
    const int *d_cols;
    const int *d_inv_row_offsets;  // in-neighbour CSR of an asymmetric input, else NULL: the row is its own mirror
    const int *d_inv_cols;
};

struct Keys {
    const int *d_prio;   // caller priorities (signed), or NULL: hashed
    unsigned seed_mul;   // seed * 0x9E3779B9
};

struct State {
    unsigned char *d_state;       // SET: 0 undecided, 1 in, 2 out
    int *d_ids;                   // the result; the colourings' state table (0 undecided)
    int *d_pos;                   // cursor: position in the (out-row, in-row) sequence of the entry that blocked
    int *d_acc;                   // COLOR_ROUNDS: running maximum; COLOR_FIRST_FIT: base of the colour window
    unsigned long long *d_mask;   // COLOR_FIRST_FIT: colours seen in [base, base + 64)
};

// (prio, v) as one unsigned 64-bit key
template <bool HASHED>
__device__ __forceinline__ unsigned long long MisKey(const Keys &k, int v)
{
    const unsigned p = HASHED ? Fmix32(static_cast<unsigned>(v) + k.seed_mul) : (static_cast<unsigned>(k.d_prio[v]) ^ 0x80000000u);
    return (static_cast<unsigned long long>(p) << 32) | static_cast<unsigned>(v);
}

// state of u: 0 undecided; SET 1 in / 2 out; colourings: the colour
template <int MODE, bool FRESH>
__device__ __forceinline__ int Probe(const State &st, int u)
{
    if (MODE == MIS_SET) return FRESH ? __hip_atomic_load(st.d_state + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : st.d_state[u];
    return FRESH ? __hip_atomic_load(st.d_ids + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : st.d_ids[u];
}

template <int MODE, bool FRESH>
__device__ __forceinline__ void Decide(const State &st, int v, int value)
{
    if (MODE == MIS_SET) {
        if (value == 1) st.d_ids[v] = 1;
        if (FRESH) __hip_atomic_store(st.d_state + v, static_cast<unsigned char>(value), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else st.d_state[v] = static_cast<unsigned char>(value);
    } else {
        if (FRESH) __hip_atomic_store(st.d_ids + v, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else st.d_ids[v] = value;
    }
}

// what a lane knows about its vertex while a tile is processed
struct Walk {
    int v;
    int out_begin, out_len;  // row v
    int in_begin;            // row v of the in-neighbour CSR
    int len;                 // out_len + in-degree (in-degree 0 on a symmetric input)
    int pos, acc;
    unsigned long long mask;
    unsigned long long key;
};

__device__ __forceinline__ int Entry(const Graph &g, int out_begin, int out_len, int in_begin, int p)
{
    return p < out_len ? g.d_cols[out_begin + p] : g.d_inv_cols[in_begin + (p - out_len)];
}

enum Status { kIdle = 0, kTodo = 1, kBlocked = 2, kDone = 3 };

// One pass of a lane over what is left of its row.  Returns kDone (value = what to write), kBlocked, or kTodo (first-fit: the
// window was full and has moved up, the row is to be scanned again).
template <int MODE, bool HASHED, bool FRESH>
__device__ __forceinline__ int LaneWalk(const Graph &g, const Keys &k, const State &st, Walk &w, int &value, unsigned &reads)
{
    int first_blocked = -1;
    for (int p = w.pos; p < w.len; ++p) {
        const int u = Entry(g, w.out_begin, w.out_len, w.in_begin, p);
        ++reads;
        if (u == w.v || MisKey<HASHED>(k, u) < w.key) continue;
        const int s = Probe<MODE, FRESH>(st, u);
        if (MODE == MIS_SET) {
            if (s == 1) { value = 2; return kDone; }
            if (s == 0 && first_blocked < 0) first_blocked = p;
        } else {
            if (s == 0) { w.pos = p; return kBlocked; }
            if (MODE == MIS_COLOR_ROUNDS) {
                w.acc = s > w.acc ? s : w.acc;
            } else {
                const unsigned d = static_cast<unsigned>(s - w.acc);  // (colours below the window wrap to a huge value)
                if (d < 64u) w.mask |= 1ull << d;
            }
        }
    }
    if (MODE == MIS_SET) {
        if (first_blocked < 0) { value = 1; return kDone; }
        w.pos = first_blocked;
        return kBlocked;
    }
    if (MODE == MIS_COLOR_ROUNDS) { value = w.acc + 1; return kDone; }
    if (~w.mask) { value = w.acc + __ffsll(static_cast<long long>(~w.mask)) - 1; return kDone; }
    w.acc += 64;
    w.mask = 0;
    w.pos = 0;
    return kTodo;
}

// The same pass by the whole wave over the row of lane `leader`, kWaveUnroll chunks of 64 entries per step.  Every value that leaves is
// wave-uniform; the leader takes it into its own Walk.
template <int MODE, bool HASHED, bool FRESH>
__device__ __forceinline__ int WaveWalk(const Graph &g, const Keys &k, const State &st, Walk &w, int leader, int &value, unsigned &reads)
{
    const int lane = static_cast<int>(util::LaneId());
    const int v = __shfl(w.v, leader, util::kWaveSize);
    const int out_begin = __shfl(w.out_begin, leader, util::kWaveSize), out_len = __shfl(w.out_len, leader, util::kWaveSize);
    const int in_begin = __shfl(w.in_begin, leader, util::kWaveSize), len = __shfl(w.len, leader, util::kWaveSize);
    int pos = __shfl(w.pos, leader, util::kWaveSize);
    int acc = __shfl(w.acc, leader, util::kWaveSize);
    unsigned long long mask = __shfl(w.mask, leader, util::kWaveSize);
    const unsigned long long key = __shfl(w.key, leader, util::kWaveSize);
    int status = kDone, out = 0, first_blocked = -1;
    bool stop = false;
    for (int base = pos; base < len && !stop; base += util::kWaveSize * kWaveUnroll) {  // (wave-uniform)
        // kWaveUnroll chunks of 64 entries with their loads in flight together: a hub's row is walked at memory latency per
        // step, and that walk lies on the dependency chain of the tail
        int us[kWaveUnroll], ss[kWaveUnroll];
#pragma unroll
        for (int j = 0; j < kWaveUnroll; ++j) {
            const int p = base + j * util::kWaveSize + lane;
            us[j] = p < len ? Entry(g, out_begin, out_len, in_begin, p) : -1;
        }
#pragma unroll
        for (int j = 0; j < kWaveUnroll; ++j) {
            ss[j] = -1;  // not a member of H(v)
            if (us[j] >= 0) {
                ++reads;
                if (us[j] != v && MisKey<HASHED>(k, us[j]) > key) ss[j] = Probe<MODE, FRESH>(st, us[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < kWaveUnroll; ++j) {
            if (stop) continue;
            const int s = ss[j];
            const int chunk = base + j * util::kWaveSize;
            const unsigned long long blocked = __ballot(s == 0);
            if (MODE == MIS_SET) {
                if (__ballot(s == 1)) { out = 2; stop = true; continue; }
                if (blocked && first_blocked < 0) first_blocked = chunk + __ffsll(static_cast<long long>(blocked)) - 1;
                continue;
            }
            const int limit = blocked ? __ffsll(static_cast<long long>(blocked)) - 1 : util::kWaveSize;
            const bool counts = lane < limit && s > 0;
            if (MODE == MIS_COLOR_ROUNDS) {
                int m = counts ? s : 0;
                for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
                    const int other = __shfl_xor(m, o, util::kWaveSize);
                    m = other > m ? other : m;
                }
                acc = m > acc ? m : acc;
            } else {
                const unsigned d = static_cast<unsigned>(s - acc);
                unsigned long long bits = counts && d < 64u ? 1ull << d : 0ull;
                for (int o = util::kWaveSize / 2; o > 0; o >>= 1) bits |= __shfl_xor(bits, o, util::kWaveSize);
                mask |= bits;
            }
            if (blocked) { pos = chunk + limit; status = kBlocked; stop = true; }
        }
    }
    if (MODE == MIS_SET) {
        if (out == 0) {
            if (first_blocked < 0) out = 1;
            else { pos = first_blocked; status = kBlocked; }
        }
    } else if (status == kDone) {
        if (MODE == MIS_COLOR_ROUNDS) out = acc + 1;
        else if (~mask) out = acc + __ffsll(static_cast<long long>(~mask)) - 1;
        else { acc += 64; mask = 0; pos = 0; status = kTodo; }
    }
    if (lane == leader) { w.pos = pos; w.acc = acc; w.mask = mask; value = out; }
    return status;
}

// All lanes of a wave together: status is kTodo for the lanes that hold an undecided vertex, kIdle for the others; on return
// it is kDone (decided and written), kBlocked (cursor in w) or kIdle.
template <int MODE, bool HASHED, bool FRESH>
__device__ __forceinline__ void ProcessTile(const Graph &g, const Keys &k, const State &st, Walk &w, int &status, unsigned &reads)
{
    const int lane = static_cast<int>(util::LaneId());
    while (__ballot(status == kTodo)) {  // (more than one turn only when a first-fit window moved up)
        int value = 0;
        const bool wide = status == kTodo && w.len - w.pos > kLaneRow;
        if (status == kTodo && !wide) status = LaneWalk<MODE, HASHED, FRESH>(g, k, st, w, value, reads);
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int s = WaveWalk<MODE, HASHED, FRESH>(g, k, st, w, leader, value, reads);
            if (lane == leader) status = s;
            todo &= todo - 1;
        }
        if (status == kDone && value) {
            Decide<MODE, FRESH>(st, w.v, value);
            value = 0;
        }
    }
}

__device__ __forceinline__ void LoadRow(const Graph &g, Walk &w)
{
    w.out_begin = g.d_row_offsets[w.v];
    w.out_len = g.d_row_offsets[w.v + 1] - w.out_begin;
    w.in_begin = 0;
    w.len = w.out_len;
    if (g.d_inv_row_offsets) {
        w.in_begin = g.d_inv_row_offsets[w.v];
        w.len += g.d_inv_row_offsets[w.v + 1] - w.in_begin;
    }
}

template <int MODE>
__device__ __forceinline__ void LoadCursor(const State &st, Walk &w, bool first)
{
    w.pos = 0;
    w.acc = MODE == MIS_COLOR_FIRST_FIT ? 1 : 0;
    w.mask = 0;
    if (first) return;
    w.pos = st.d_pos[w.v];
    if (MODE != MIS_SET) w.acc = st.d_acc[w.v];
    if (MODE == MIS_COLOR_FIRST_FIT) w.mask = st.d_mask[w.v];
}

template <int MODE>
__device__ __forceinline__ void StoreCursor(const State &st, const Walk &w)
{
    st.d_pos[w.v] = w.pos;
    if (MODE != MIS_SET) st.d_acc[w.v] = w.acc;
    if (MODE == MIS_COLOR_FIRST_FIT) st.d_mask[w.v] = w.mask;
}

// A colouring's vertex that comes back with a cursor first asks its blocking entry alone (a member of H(v): it blocked): while
// that neighbour is undecided nothing else about v can change, and the poll costs one entry instead of a walk.
template <int MODE, bool HASHED, bool FRESH>
__device__ __forceinline__ bool StillBlocked(const Graph &g, const State &st, const Walk &w, unsigned &polls)
{
    if (MODE == MIS_SET) return false;  // (the set may be decided by any later member of H(v): it walks on)
    ++polls;
    return Probe<MODE, FRESH>(st, Entry(g, w.out_begin, w.out_len, w.in_begin, w.pos)) == 0;
}

// d_reads[0] += row entries walked, d_reads[3] += polls of a blocking entry
__device__ __forceinline__ void AddReads(unsigned reads, unsigned polls, unsigned long long *d_reads)
{
    unsigned long long r = reads, q = polls;
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        r += __shfl_xor(r, o, util::kWaveSize);
        q += __shfl_xor(q, o, util::kWaveSize);
    }
    if (util::LaneId() == 0 && r) atomicAdd(d_reads, r);
    if (util::LaneId() == 0 && q) atomicAdd(d_reads + 3, q);
}

// One sweep over the worklist (d_list == NULL: every vertex, the first sweep, cursors not yet written); the vertices that are
// still undecided go to d_out_list, *d_out_count of them.
template <int MODE, bool HASHED>
static __global__ __launch_bounds__(kSweepThreads) void SweepKernel(Graph g, Keys k, State st, const int *d_list, long long count, int *d_out_list,
                                                                     int *d_out_count, unsigned long long *d_reads)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    unsigned reads = 0, polls = 0;
    for (long long base = wave0 * util::kWaveSize; base < count; base += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = base + lane;
        Walk w = {};
        int status = kIdle;
        bool moved = true;  // the cursor in w is not the stored one
        if (i < count) {
            w.v = d_list ? d_list[i] : static_cast<int>(i);
            LoadRow(g, w);
            LoadCursor<MODE>(st, w, d_list == nullptr);
            w.key = MisKey<HASHED>(k, w.v);
            status = kTodo;
            if (d_list && StillBlocked<MODE, HASHED, false>(g, st, w, polls)) { status = kBlocked; moved = false; }
        }
        ProcessTile<MODE, HASHED, false>(g, k, st, w, status, reads);
        const bool left = status == kBlocked;
        if (left && moved) StoreCursor<MODE>(st, w);
        const unsigned long long keep = __ballot(left);
        if (keep) {
            int at = 0;
            if (lane == 0) at = atomicAdd(d_out_count, __popcll(keep));
            at = __shfl(at, 0, util::kWaveSize);
            if (left) d_out_list[at + __popcll(keep & ((1ull << lane) - 1))] = w.v;
        }
    }
    AddReads(reads, polls, d_reads);
}

// The tail: one window of the worklist, at most one vertex per thread (count <= gridDim.x * blockDim.x), swept up to max_sweeps
// times in one launch with everything about the vertex in registers: a blocked vertex polls the state of its one blocking
// neighbour (the set too: here it walks again only when its first undecided member of H(v) is decided, so a vertex stuck behind
// a long chain does not re-read its row every sweep).  State is read and written with agent-scope accesses.
// Nobody waits for anybody: a wave leaves when its vertices are decided or after max_sweeps.  The host lists the vertices in
// descending key order, so all of H(v) lies in this window or in an earlier one; when an earlier window of the same pass
// left something undecided (*d_left != 0 on entry), this one only counts its own undecided vertices.
// d_window[0] += the vertices still undecided, d_window[1] = the largest number of sweeps a wave made, *d_left += d_window[0].
template <int MODE, bool HASHED>
static __global__ __launch_bounds__(kSweepThreads) void TailKernel(Graph g, Keys k, State st, const int *d_list, int count, int max_sweeps,
                                                                    int *d_left, int *d_window, unsigned long long *d_reads)
{
    const int lane = static_cast<int>(util::LaneId());
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool skip = __hip_atomic_load(d_left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    unsigned reads = 0, polls = 0;
    Walk w = {};
    int status = kIdle, blocker = 0, sweeps = 0;
    bool moved = false;  // the cursor in w is not the stored one
    if (i < count) {
        w.v = d_list[i];
        if (Probe<MODE, true>(st, w.v) == 0) status = kBlocked;
    }
    if (status == kBlocked && !skip) {
        LoadRow(g, w);
        LoadCursor<MODE>(st, w, false);
        w.key = MisKey<HASHED>(k, w.v);
        blocker = Entry(g, w.out_begin, w.out_len, w.in_begin, w.pos);
    }
    while (!skip && sweeps < max_sweeps && __ballot(status == kBlocked)) {  // (wave-uniform)
        ++sweeps;
        if (status == kBlocked) {
            ++polls;
            if (Probe<MODE, true>(st, blocker) != 0) status = kTodo;
        }
        if (__ballot(status == kTodo)) {
            const bool walked = status == kTodo;
            ProcessTile<MODE, HASHED, true>(g, k, st, w, status, reads);
            if (walked && status == kBlocked) {
                moved = true;
                blocker = Entry(g, w.out_begin, w.out_len, w.in_begin, w.pos);
            }
        } else {
            __builtin_amdgcn_s_sleep(1);
        }
    }
    const bool left = status == kBlocked;
    if (left && moved) StoreCursor<MODE>(st, w);
    const int n_left = __popcll(__ballot(left));
    if (lane == 0) {
        if (n_left) {
            atomicAdd(d_window, n_left);
            atomicAdd(d_left, n_left);
        }
        if (sweeps) atomicMax(d_window + 1, sweeps);
    }
    AddReads(reads, polls, d_reads);
}

// the worklist in descending key order: keys = ~key(v) for an ascending sort, then the vertex back out of the low half
template <bool HASHED>
static __global__ void OrderKeysKernel(Keys k, const int *d_list, long long count, unsigned long long *d_keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) d_keys[i] = ~MisKey<HASHED>(k, d_list[i]);
}
static __global__ void OrderedListKernel(const unsigned long long *d_sorted, long long count, int *d_list)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
        d_list[i] = static_cast<int>(static_cast<unsigned>(~d_sorted[i]));
}

// d_summary[0] = sum of ids (the size of the set), d_summary[1] = max of ids (the number of colours)
static __global__ void SummaryKernel(const int *d_ids, long long nodes, unsigned long long *d_summary)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned long long sum = 0;
    int most = 0;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int c = d_ids[v];
        sum += static_cast<unsigned long long>(c);
        most = c > most ? c : most;
    }
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, util::kWaveSize);
        const int other = __shfl_xor(most, o, util::kWaveSize);
        most = other > most ? other : most;
    }
    if (util::LaneId() == 0) {
        atomicAdd(d_summary, sum);
        atomicMax(d_summary + 1, static_cast<unsigned long long>(most));
    }
}

}  // namespace mis
}  // namespace app
}  // namespace gunrock
