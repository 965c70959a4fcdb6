// app/bipartite/bipartite_functor.hpp -- device kernels of the maximum bipartite matching and the Dulmage-Mendelsohn decomposition.
//
// The reference snapshot has no app/bipartite; the shape follows this tree's stepped primitives: BCC's forest
// with its one queue and its one-workgroup device loop, the lane / wave / workgroup row ladder, WaveTicket appends.
//
// A CSR pattern of shape (rows, cols) is the bipartite graph rows -- columns.  A search is side-neutral: it grows a forest of
// alternating paths from all unmatched vertices of the side U over U's adjacency (columns over A^T for the matching and the horizontal
// part; rows over A for the vertical part), claiming vertices of the other side W:
//   level      a frontier u walks its entries w.  An unclaimed matched w is claimed by CAS on pred[w]; its mate joins the next frontier
//              under u's root.  An unclaimed unmatched w is an END: one lane at a time of a tree's wave claims it and posts it with
//              atomicMin into winner[root].  A tree that has a winner stops claiming, so the other trees get the rest.
//   phase      levels until the first one that found an end (or an empty frontier); AugmentKernel then walks pred / mate from every
//              winner back to its root and flips the pairs.  Trees are vertex-disjoint by the CAS: one path per tree needs no repair.
//   the end    a phase without an end: the matching is maximum (Berge) and that forest is the horizontal part.  One more search from
//              the unmatched rows gives the vertical part, CertKernel counts what König's theorem asks of the two.
// A level is a STEP: a wide launch (StepKernel), or one of a stretch of steps inside LoopKernel, one workgroup that puts a fence and a
// barrier between levels and uses agent-scope accesses on what a level leaves for the next.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace bipartite {

enum { BIPARTITE_AUTO = 0, BIPARTITE_LANE = 1, BIPARTITE_WAVE = 2, BIPARTITE_BLOCK = 3 };  // "strategy"; 1 .. 3 are the regimes
enum { BIPARTITE_HORIZONTAL = 0, BIPARTITE_SQUARE = 1, BIPARTITE_VERTICAL = 2 };           // row_part / col_part
enum { BIPARTITE_MAXIMUM = 0, BIPARTITE_CAPPED = 1 };                                      // how an Enact ended

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / util::kWaveSize;
constexpr int kFree = -1;               // pred[]: not claimed; mate[]: unmatched
constexpr int kNone = 0x7FFFFFFF;       // winner[]: the tree has no end yet
constexpr int kBlockMinRow = 2048;      // "block_min_row": a column of this many entries and more is walked by its workgroup
constexpr int kHubSlots = 64;           // the long columns a workgroup lists per level; the ones beyond are a wave's
constexpr int kCertWaveRow = 64;        // CertKernel, the checks and the builds: a row this long is walked by the whole wave

using oprtr::kLoopMaxSteps;
using oprtr::kLoopThreads;
using oprtr::Ld;
using oprtr::Limits;
using oprtr::Narrow;
using oprtr::St;
using oprtr::TileFor;

// the 32-bit words the kernels and the host share
enum {
    W_TAIL = 0,  // queue tickets handed out in this search
    W_ENTRIES,   // the entries of the vertices queued in this search, modulo 2^32
    W_FOUND,     // ends claimed in this search
    W_AUG,       // paths flipped since the Reset
    W_GREEDY,    // pairs of the greedy start
    W_BAD,       // CheckStartKernel: the start matching is none
    W_COUNT = 8
};
// the 64-bit counts, read back once behind the certificate
enum {
    C_BAD_PAIRS = 0,  // mates that are not mutual, out of range or no entry of the matrix
    C_UNCOVERED,      // entries the cover misses, vertices in both the horizontal and the vertical part, ends of the vertical search
    C_COVER,          // |cover|
    C_SIZE,           // matched rows
    C_REGIME,         // three words: the frontier vertices walked by a lane, a wave, a workgroup
    C_PART = C_REGIME + 3,  // six words: rows then columns in the horizontal, square, vertical part
    C_COUNT = 16
};

// where the read-backs land in the enactor's pinned buffer
constexpr size_t kPinnedWords = 0;                                    // W_COUNT x 4 bytes
constexpr size_t kPinnedFront = 32;                                   // a Front
constexpr size_t kPinnedCounts = 64;                                  // C_COUNT x 8 bytes
constexpr size_t kPinnedSquare = kPinnedCounts + 8 * C_COUNT;         // two ints: k and the arcs of the square graph
constexpr size_t kPinnedBytes = kPinnedSquare + 16;

// which way a frontier vertex with `len` entries is walked (len > 0)
__host__ __device__ __forceinline__ int Regime(int len, int strategy, int wave_min_row, int block_min_row)
{
    if (strategy != BIPARTITE_AUTO) return strategy;
    if (len >= block_min_row && len >= wave_min_row) return BIPARTITE_BLOCK;
    return len >= wave_min_row ? BIPARTITE_WAVE : BIPARTITE_LANE;
}

// one search: U's side of the graph and both mate arrays as that side sees them
struct Ctx {
    const int *ro, *ci;   // the adjacency of U: n_u rows with entries in [0, n_w)
    int *mate_u, *mate_w;
    int *pred;            // per w: the u that claimed it, or kFree
    int *root;            // per u in the forest: the root of its tree
    int *winner;          // per root: the smallest end of its tree, or kNone
    int *queue;           // every u of the forest once, level by level; the roots first
    unsigned *words;
    unsigned long long *counts;
    int n_u, n_w, cap;    // cap: the room of queue
    int strategy, wave_min_row, block_min_row;
};

// a search's next level; the host and LoopKernel carry the same
struct Front {
    int level;
    unsigned head, tail;
    unsigned entries_seen;  // W_ENTRIES when the level was complete
    unsigned step_entries;  // entries of [head, tail)
    unsigned found;         // W_FOUND when the level was complete
};
static_assert(sizeof(Front) <= kPinnedCounts - kPinnedFront, "the pinned layout");

struct Tally {
    unsigned entries = 0;  // entries of the vertices this lane queued
    unsigned found = 0;    // ends this lane claimed
    unsigned regime[3] = {0, 0, 0};
};

__device__ __forceinline__ void Flush(Tally &t, const Ctx &c)
{
    const unsigned entries = util::WaveSum(t.entries), found = util::WaveSum(t.found);
    const unsigned r0 = util::WaveSum(t.regime[0]), r1 = util::WaveSum(t.regime[1]), r2 = util::WaveSum(t.regime[2]);
    if (util::LaneId() == 0) {
        if (entries) atomicAdd(c.words + W_ENTRIES, entries);
        if (found) atomicAdd(c.words + W_FOUND, found);
        if (r0) atomicAdd(c.counts + C_REGIME, static_cast<unsigned long long>(r0));
        if (r1) atomicAdd(c.counts + C_REGIME + 1, static_cast<unsigned long long>(r1));
        if (r2) atomicAdd(c.counts + C_REGIME + 2, static_cast<unsigned long long>(r2));
    }
    t = Tally();
}

// All lanes of the wave call; the lanes with `hit` append m under root r: one atomic on the ticket word per wave.  A vertex joins a
// forest once, so a position stays under cap; the test keeps a mistake elsewhere from turning into a store outside the queue.
template <bool FRESH>
__device__ __forceinline__ void Append(const Ctx &c, bool hit, int m, int r, Tally &t)
{
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const unsigned pos = oprtr::WaveTicket(c.words + W_TAIL, mask);
    if (hit) {
        St<FRESH>(c.root + m, r);
        if (pos < static_cast<unsigned>(c.cap)) St<FRESH>(c.queue + pos, m);
        t.entries += static_cast<unsigned>(c.ro[m + 1] - c.ro[m]);
    }
}

// One entry per lane: u of tree r reaches w (valid lanes).  SHARED: the whole wave walks one u, so its ends are claimed one lane at
// a time and the walk stops at the first that holds (else: every lane walks its own u, and an end is its own tree's).  Returns
// whether this lane's tree has its winner now.
template <bool FRESH, bool SHARED>
__device__ __forceinline__ bool Reach(const Ctx &c, bool valid, int u, int r, int w, Tally &t)
{
    bool claimed = false, end = false, won = false;
    int m = kFree;
    if (valid && Ld<FRESH>(c.pred + w) == kFree) {  // (a stale plain read can only say "not claimed": the CAS decides)
        m = c.mate_w[w];
        if (m >= 0) claimed = atomicCAS(c.pred + w, kFree, u) == kFree;
        else end = true;
    }
    if (SHARED) {
        unsigned long long ends = __ballot(end);
        while (ends && !won) {  // (wave-uniform)
            const int leader = __ffsll(static_cast<long long>(ends)) - 1;
            int ok = 0;
            if (static_cast<int>(util::LaneId()) == leader && atomicCAS(c.pred + w, kFree, u) == kFree) {
                atomicMin(c.winner + r, w);
                ++t.found;
                ok = 1;
            }
            won = __shfl(ok, leader, util::kWaveSize) != 0;
            ends &= ends - 1;
        }
    } else if (end && atomicCAS(c.pred + w, kFree, u) == kFree) {
        atomicMin(c.winner + r, w);
        ++t.found;
        won = true;
    }
    Append<FRESH>(c, claimed, m, r, t);
    return won;
}

// one u by all of `nwaves` waves (1: the wave's own walk), wave `wave` of them taking every nwaves-th 64 entries
template <bool FRESH>
__device__ __forceinline__ void WalkShared(const Ctx &c, int u, int b, int e, int wave, int nwaves, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    const int r = Ld<FRESH>(c.root + u);
    for (int from = b + wave * util::kWaveSize; from < e; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        if (__hip_atomic_load(c.winner + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kNone) break;
        const int i = from + lane;
        if (Reach<FRESH, true>(c, i < e, u, r, i < e ? c.ci[i] : 0, t)) break;
    }
}

// 64 queue entries by one wave: lane `lane` holds u (or -1).  Short rows by their lane, which looks at its tree's winner before the
// row and again every 16 entries; the others by the whole wave one after the other; the BLOCK regime's go to the workgroup's list
// s_hubs (s_hub_count of them, at most kHubSlots: the rest is a wave's).
template <bool FRESH>
__device__ __forceinline__ void Tile(const Ctx &c, int u, int *s_hubs, int *s_hub_count, Tally &t)
{
    int b = 0, e = 0, regime = 0;
    if (u >= 0) {
        b = c.ro[u];
        e = c.ro[u + 1];
        if (e > b) regime = Regime(e - b, c.strategy, c.wave_min_row, c.block_min_row);
    }
    if (regime == BIPARTITE_BLOCK) {
        const int at = atomicAdd(s_hub_count, 1);
        if (at < kHubSlots) s_hubs[at] = u;
        else regime = BIPARTITE_WAVE;
    }
    if (regime) ++t.regime[regime - 1];
    const bool own = regime == BIPARTITE_LANE;
    unsigned long long todo = __ballot(regime == BIPARTITE_WAVE);

    int longest = own ? e - b : 0;
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        const int other = __shfl_xor(longest, o, util::kWaveSize);
        longest = other > longest ? other : longest;
    }
    int r = 0;
    bool going = own;
    if (own) {
        r = Ld<FRESH>(c.root + u);
        going = __hip_atomic_load(c.winner + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kNone;
    }
    for (int j = 0; j < longest; ++j) {  // (wave-uniform)
        if (going && (j & 15) == 15) going = __hip_atomic_load(c.winner + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kNone;
        const bool valid = going && b + j < e;
        if (Reach<FRESH, false>(c, valid, u, r, valid ? c.ci[b + j] : 0, t)) going = false;
    }
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const int lb = __shfl(b, leader, util::kWaveSize), le = __shfl(e, leader, util::kWaveSize), lu = __shfl(u, leader, util::kWaveSize);
        WalkShared<FRESH>(c, lu, lb, le, 0, 1, t);
        todo &= todo - 1;
    }
}

// level = queue[head, tail), `tile` entries per wave at a time; then the workgroup's long columns.  Every thread of the workgroup
// calls (two barriers inside).
template <bool FRESH>
__device__ __forceinline__ void RunLevel(const Ctx &c, long long head, long long tail, int tile, long long wave0, long long nwaves, int *s_hubs,
                                         int *s_hub_count, Tally &t)
{
    const int lane = static_cast<int>(util::LaneId());
    if (tail > c.cap) tail = c.cap;
    for (long long from = head + wave0 * tile; from < tail; from += nwaves * tile) {  // (wave-uniform)
        const long long i = from + lane;
        int u = -1;
        if (lane < tile && i < tail) u = Ld<FRESH>(c.queue + i);
        Tile<FRESH>(c, u, s_hubs, s_hub_count, t);
    }
    __syncthreads();
    const int hubs = *s_hub_count < kHubSlots ? *s_hub_count : kHubSlots;
    const int wave = static_cast<int>(threadIdx.x) / util::kWaveSize, block_waves = static_cast<int>(blockDim.x) / util::kWaveSize;
    for (int h = 0; h < hubs; ++h) {  // (uniform over the workgroup)
        const int u = s_hubs[h];
        WalkShared<FRESH>(c, u, c.ro[u], c.ro[u + 1], wave, block_waves, t);
    }
    __syncthreads();
    if (threadIdx.x == 0) *s_hub_count = 0;
}

// ---------------- the wide form and the device loop ----------------

static __global__ __launch_bounds__(kThreads) void StepKernel(Ctx c, unsigned head, unsigned tail, int tile)
{
    __shared__ int s_hubs[kHubSlots];
    __shared__ int s_hub_count;
    if (threadIdx.x == 0) s_hub_count = 0;
    __syncthreads();
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    Tally t;
    RunLevel<false>(c, head, tail, tile, wave0, nwaves, s_hubs, &s_hub_count, t);
    Flush(t, c);
}

// One workgroup searches level after level while each is narrow and none has found an end (stop_on_end; the vertical search goes
// on).  Every step ends in a barrier behind a fence, the words are read with agent-scope loads by every thread, and a second barrier
// keeps the next step's atomics behind those reads.  Uniform control flow: every thread carries the same Front.
static __global__ __launch_bounds__(kLoopThreads) void LoopKernel(Ctx c, Front s, Limits lim, int stop_on_end, Front *d_front)
{
    __shared__ int s_hubs[kHubSlots];
    __shared__ int s_hub_count;
    if (threadIdx.x == 0) s_hub_count = 0;
    __syncthreads();
    const long long wave0 = threadIdx.x / util::kWaveSize, nwaves = kLoopThreads / util::kWaveSize;
    const int *words = reinterpret_cast<const int *>(c.words);
    Tally t;
    for (int step = 0; step < lim.max_steps && s.head < s.tail && !(stop_on_end && s.found) && Narrow(s.tail - s.head, s.step_entries, lim); ++step) {
        const int tile = TileFor(static_cast<long long>(s.tail - s.head), nwaves, s.step_entries);
        RunLevel<true>(c, s.head, s.tail, tile, wave0, nwaves, s_hubs, &s_hub_count, t);
        Flush(t, c);
        __threadfence();
        __syncthreads();
        const unsigned tail = static_cast<unsigned>(Ld<true>(words + W_TAIL));
        const unsigned entries = static_cast<unsigned>(Ld<true>(words + W_ENTRIES));
        const unsigned found = static_cast<unsigned>(Ld<true>(words + W_FOUND));
        ++s.level;
        s.head = s.tail;
        s.tail = tail;
        s.step_entries = entries - s.entries_seen;
        s.entries_seen = entries;
        s.found = found;
        __syncthreads();
    }
    if (threadIdx.x == 0) *d_front = s;
}

// ---------------- around the levels ----------------

// The start of a search: nothing claimed, the words of the search at 0 (by the host, before), every unmatched u a root in the queue.
static __global__ __launch_bounds__(kThreads) void RootsKernel(Ctx c)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long first = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (long long w = first; w < c.n_w; w += stride) c.pred[w] = kFree;
    Tally t;
    const long long padded = (static_cast<long long>(c.n_u) + util::kWaveSize - 1) / util::kWaveSize * util::kWaveSize;
    for (long long u = first; u < padded; u += stride) {  // (wave-uniform: 256 divides the stride)
        const bool is_root = u < c.n_u && c.mate_u[u] < 0;
        if (is_root) c.winner[u] = kNone;
        Append<false>(c, is_root, static_cast<int>(u), static_cast<int>(u), t);
    }
    Flush(t, c);
}

// One lane per root (queue[0, roots)): a tree with a winner flips the path from it back to the root.  The walk reads what the level
// kernels left in L2, so its loads are agent-scope; `cap` + 1 steps bound it whatever it reads.
static __global__ __launch_bounds__(kThreads) void AugmentKernel(Ctx c, unsigned roots)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned flipped = 0;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < roots && i < c.cap; i += stride) {
        const int r = c.queue[i];
        int w = Ld<true>(c.winner + r);
        if (w == kNone) continue;
        ++flipped;
        for (int guard = 0; guard <= c.cap; ++guard) {
            const int u = Ld<true>(c.pred + w);
            if (u < 0 || u >= c.n_u) break;
            const int before = Ld<true>(c.mate_u + u);
            St<true>(c.mate_w + w, u);
            St<true>(c.mate_u + u, w);
            if (before < 0) break;  // (u is the root)
            w = before;
        }
    }
    flipped = util::WaveSum(flipped);
    if (util::LaneId() == 0 && flipped) atomicAdd(c.words + W_AUG, flipped);
}

// The forest of the search that just ended is the part `value`: every claimed w and every queued u.  A vertex that is in another
// part already (the horizontal one, when the vertical is marked) stays there and is counted.
static __global__ __launch_bounds__(kThreads) void MarkKernel(Ctx c, unsigned tail, int value, int *part_u, int *part_w)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long first = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned twice = 0;
    for (long long w = first; w < c.n_w; w += stride)
        if (c.pred[w] != kFree) {
            if (part_w[w] != BIPARTITE_SQUARE) ++twice;
            else part_w[w] = value;
        }
    for (long long i = first; i < tail && i < c.cap; i += stride) {
        const int u = c.queue[i];
        if (part_u[u] != BIPARTITE_SQUARE) ++twice;
        else part_u[u] = value;
    }
    twice = util::WaveSum(twice);
    if (util::LaneId() == 0 && twice) atomicAdd(c.counts + C_UNCOVERED, static_cast<unsigned long long>(twice));
}

// ---------------- the start ----------------

// the matrix both ways, the mates as rows and columns see them
struct Sides {
    const int *ro, *ci;  // A
    int *mate_row, *mate_col;
    int rows, cols;
};

// 64 rows by one wave, a row of kCertWaveRow entries and more by all of it: f(row, entry index, valid) is called by every lane of the
// wave together for the long rows, and by a lane alone for its own short row
template <typename Short, typename Long>
__device__ __forceinline__ void ForRows(const int *ro, long long rows, Short on_short, Long on_long)
{
    const int lane = static_cast<int>(util::LaneId());
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    for (long long from = wave0 * util::kWaveSize; from < rows; from += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long row = from + lane;
        int b = 0, e = 0;
        if (row < rows) {
            b = ro[row];
            e = ro[row + 1];
        }
        const bool wide = e - b >= kCertWaveRow;
        unsigned long long todo = __ballot(wide);
        if (row < rows && !wide) on_short(static_cast<int>(row), b, e);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            on_long(static_cast<int>(from) + leader, __shfl(b, leader, util::kWaveSize), __shfl(e, leader, util::kWaveSize), lane);
            todo &= todo - 1;
        }
    }
}

// does row [b, e) hold column `wanted`?  by a lane / by the wave
__device__ __forceinline__ bool RowHas(const int *ci, int b, int e, int wanted)
{
    bool has = false;
    for (int i = b; i < e; ++i) has |= ci[i] == wanted;
    return has;
}
__device__ __forceinline__ bool RowHasWave(const int *ci, int b, int e, int wanted, int lane)
{
    bool has = false;
    for (int i = b + lane; i < e; i += util::kWaveSize) has |= ci[i] == wanted;
    return __ballot(has) != 0;
}

// A start matching (mate_row given, mate_col all kFree before): every mate in range and an entry of its row, no column twice.
// words[W_BAD] counts what is not.
static __global__ __launch_bounds__(kThreads) void CheckStartKernel(Sides s, unsigned *words)
{
    auto take = [&](int row, int m, bool in_range, bool has) {
        if (m == kFree) return;
        if (!in_range || !has || atomicCAS(s.mate_col + m, kFree, row) != kFree) atomicAdd(words + W_BAD, 1u);
    };
    ForRows(
        s.ro, s.rows,
        [&](int row, int b, int e) {
            const int m = s.mate_row[row];
            const bool in_range = m >= 0 && m < s.cols;
            take(row, m, in_range, in_range && RowHas(s.ci, b, e, m));
        },
        [&](int row, int b, int e, int lane) {
            const int m = s.mate_row[row];
            const bool in_range = m >= 0 && m < s.cols;
            const bool has = RowHasWave(s.ci, b, e, m, lane);
            if (lane == 0) take(row, m, in_range, in_range && has);
        });
}

// The greedy start: every unmatched row claims its first free column, a short row by its lane, a long one by the whole wave, 64
// entries at a time and the free ones among them one lane after the other.  Which row gets a column two rows want is the schedule's.
static __global__ __launch_bounds__(kThreads) void GreedyKernel(Sides s, unsigned *words)
{
    unsigned pairs = 0;
    auto is_free = [&](int col) { return __hip_atomic_load(s.mate_col + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kFree; };
    ForRows(
        s.ro, s.rows,
        [&](int row, int b, int e) {
            if (s.mate_row[row] != kFree) return;
            for (int i = b; i < e; ++i) {
                const int col = s.ci[i];
                if (!is_free(col) || atomicCAS(s.mate_col + col, kFree, row) != kFree) continue;
                s.mate_row[row] = col;
                ++pairs;
                break;
            }
        },
        [&](int row, int b, int e, int lane) {
            if (s.mate_row[row] != kFree) return;  // (wave-uniform)
            for (int from = b; from < e; from += util::kWaveSize) {  // (wave-uniform)
                const int i = from + lane;
                const int col = i < e ? s.ci[i] : 0;
                unsigned long long open = __ballot(i < e && is_free(col));
                int done = 0;
                while (open && !done) {
                    const int leader = __ffsll(static_cast<long long>(open)) - 1;
                    int ok = 0;
                    if (lane == leader && atomicCAS(s.mate_col + col, kFree, row) == kFree) {
                        s.mate_row[row] = col;
                        ++pairs;
                        ok = 1;
                    }
                    done = __shfl(ok, leader, util::kWaveSize);
                    open &= open - 1;
                }
                if (done) break;
            }
        });
    pairs = util::WaveSum(pairs);
    if (util::LaneId() == 0 && pairs) atomicAdd(words + W_GREEDY, pairs);
}

// ---------------- the certificate ----------------

// One pass over the entries and the mates.  Always: the mates are mutual and every pair is an entry (C_BAD_PAIRS), the matched rows
// (C_SIZE).  With the parts (a run that ended BIPARTITE_MAXIMUM): cover = {rows not vertical} + {columns vertical} as row_cover /
// col_cover, its size (C_COVER), the entries it misses (C_UNCOVERED) and the six part sizes.
static __global__ __launch_bounds__(kThreads) void CertKernel(Sides s, const int *row_part, const int *col_part, unsigned char *row_cover,
                                                              unsigned char *col_cover, int with_parts, unsigned long long *counts)
{
    unsigned bad = 0, uncovered = 0, cover = 0, size = 0;
    unsigned part[6] = {0, 0, 0, 0, 0, 0};
    auto row_head = [&](int row, int m, bool *mutual, bool *covers) {
        *mutual = m >= 0 && m < s.cols && s.mate_col[m] == row;
        *covers = with_parts && row_part[row] != BIPARTITE_VERTICAL;
    };
    auto row_tail = [&](int row, int m, bool mutual, bool has, bool covers) {
        if (m != kFree) {
            ++size;
            if (!mutual || !has) ++bad;
        }
        if (with_parts) {
            row_cover[row] = covers ? 1 : 0;
            cover += covers ? 1u : 0u;
            ++part[row_part[row]];
        }
    };
    ForRows(
        s.ro, s.rows,
        [&](int row, int b, int e) {
            const int m = s.mate_row[row];
            bool mutual, covers, has = false;
            row_head(row, m, &mutual, &covers);
            for (int i = b; i < e; ++i) {
                const int col = s.ci[i];
                has |= col == m;
                if (with_parts && !covers && col_part[col] != BIPARTITE_VERTICAL) ++uncovered;
            }
            row_tail(row, m, mutual, has, covers);
        },
        [&](int row, int b, int e, int lane) {
            const int m = s.mate_row[row];
            bool mutual, covers, has = false;
            row_head(row, m, &mutual, &covers);
            for (int i = b + lane; i < e; i += util::kWaveSize) {
                const int col = s.ci[i];
                has |= col == m;
                if (with_parts && !covers && col_part[col] != BIPARTITE_VERTICAL) ++uncovered;
            }
            has = __ballot(has) != 0;
            if (lane == 0) row_tail(row, m, mutual, has, covers);
        });
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long col = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; col < s.cols; col += stride) {
        const int m = s.mate_col[col];
        if (m != kFree && !(m >= 0 && m < s.rows && s.mate_row[m] == col)) ++bad;
        if (with_parts) {
            const bool covers = col_part[col] == BIPARTITE_VERTICAL;
            col_cover[col] = covers ? 1 : 0;
            cover += covers ? 1u : 0u;
            ++part[3 + col_part[col]];
        }
    }
    auto post = [&](int word, unsigned value) {
        value = util::WaveSum(value);
        if (util::LaneId() == 0 && value) atomicAdd(counts + word, static_cast<unsigned long long>(value));
    };
    post(C_BAD_PAIRS, bad);
    post(C_UNCOVERED, uncovered);
    post(C_COVER, cover);
    post(C_SIZE, size);
    for (int i = 0; i < 6; ++i) post(C_PART + i, part[i]);
}

// ---------------- the contracted square part ----------------

// flag[row] = the row is in the square part (flag[rows] = 0: the scan's total lands there)
static __global__ __launch_bounds__(kThreads) void SquareFlagKernel(const int *row_part, long long rows, unsigned *flag)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i <= rows; i += stride)
        flag[i] = i < rows && row_part[i] == BIPARTITE_SQUARE ? 1u : 0u;
}

// FILL false: count[local(r)] = the entries of square row r in square columns (count[k] = 0), map[local(r)] = r.
// FILL true: the arcs local(r) -> local(mate_col[c]) from offsets[local(r)] on, in the row's order.
template <bool FILL>
static __global__ __launch_bounds__(kThreads) void SquareRowsKernel(Sides s, const int *row_part, const int *col_part, const int *local, unsigned *count,
                                                                    int *map, const int *offsets, int *arcs)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long row = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; row <= s.rows; row += stride) {
        if (row == s.rows) {
            if (!FILL) count[local[row]] = 0u;
            continue;
        }
        if (row_part[row] != BIPARTITE_SQUARE) continue;
        const int at = local[row];
        int n = FILL ? offsets[at] : 0;
        for (int i = s.ro[row]; i < s.ro[row + 1]; ++i) {
            const int col = s.ci[i];
            if (col_part[col] != BIPARTITE_SQUARE) continue;
            if (FILL) arcs[n] = local[s.mate_col[col]];
            ++n;
        }
        if (!FILL) {
            count[at] = static_cast<unsigned>(n);
            map[at] = static_cast<int>(row);
        }
    }
}

}  // namespace bipartite
}  // namespace app
}  // namespace gunrock
