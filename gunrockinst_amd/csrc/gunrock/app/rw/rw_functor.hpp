// app/rw/rw_functor.hpp -- random walks: the definition (host and device) and the kernels.
//
// The reference snapshot has no app/rw.  A walk is defined so that every output is an integer with one value:
//
//   Graph.  The CSR as given: directed, self-loops and duplicate entries kept (a duplicate arc is twice as likely).  Weights are
//   optional, int32, >= 0.  Init keeps a device copy with every row sorted by (column, weight) and an inclusive int64 prefix sum of
//   the weights per row; every choice indexes the SORTED row, so a walk does not depend on the order of the entries within a row.
//
//   Draw(seed, walk, step, t) = Mix(seed ^ Mix((walk << 32) | (step << 8) | t)), Mix the splitmix64 finaliser (graphio/splitmix.hpp);
//   walk < 2^31, step < 2^24, t < 2^8.
//
//   First-order choice at v, sorted row of d entries, draw r.  Unweighted: d == 0 ends the walk, else k = ((r >> 32) * d) >> 32.
//   Weighted: T the row's weight total, T == 0 ends the walk, else t = (r * T) >> 64 (the full 128-bit product) and k the smallest
//   index whose inclusive prefix exceeds t, by bisection: a zero-weight entry is never chosen.
//
//   Step s of walk w (s = 0 .. length - 1) at v, having come from p (none at s = 0), biases (b_return, b_in, b_out) in 0 .. 65535.
//   The three equal, or s = 0: the first-order choice with Draw(seed, w, s, 0).  Otherwise, amax the largest bias, for
//   j = 0 .. tries - 1: the candidate x is the first-order choice with Draw(seed, w, s, 2j); its bias b is b_return if x == p, b_in
//   if x occurs in the sorted out-row of p (bisection), else b_out; accept if ((Draw(seed, w, s, 2j + 1) >> 32) * amax) >> 32 < b.
//   If no try accepts, the candidate of the last try is taken (a forced fallback).
//
//   Outputs.  walks: int32, num_walks x (length + 1), row w starts with starts[w], -1 behind the end of a walk; lengths: the vertices
//   in the row; visits: int64 per vertex, its occurrences in walks; steps: the steps taken.
//
// Kernels.  One launch walks every walker from start to end, one lane per walker, walkers in a grid-stride loop of waves.  LANE stores
// every vertex where it belongs (one 4-byte store per step, the 64 lanes of a wave a row apart).  TILE stages 64 walkers x 16 steps
// per wave in LDS (row stride 17 ints: the per-step writes of the 64 lanes fall into distinct banks) and flushes a tile with 16-byte
// stores, four lanes per walker row, so a store instruction writes 16 whole 64-byte segments.  The rows of the device array are
// pitched to 16 entries for that; the padding is never written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include <gunrock/app/rw/rw_draw.hpp>
#include <gunrock/graphio/splitmix.hpp>
#include <gunrock/oprtr/lds_table.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace rw {

enum { RW_AUTO = 0, RW_LANE = 1, RW_TILE = 2 };

constexpr int kRwThreads = 256;
constexpr int kRwWaves = kRwThreads / 64;
constexpr int kTileSteps = 16;              // entries of a row in one tile: 64 bytes
constexpr int kTileStride = kTileSteps + 1;  // ints between the rows of a tile in LDS
constexpr int kMaxLength = (1 << 24) - 1;
constexpr int kMaxBias = 65535;
constexpr int kMaxTries = 128;
constexpr int kDefaultTries = 32;

// words of the kernels
enum { W_STEPS = 0, W_ENDED = 1, W_TRIES = 2, W_FORCED = 3, W_COUNT = 4 };

// ---------------- the definition (Draw, MulHigh, ChooseUniform and ChooseWeighted: rw_draw.hpp) ----------------

// x occurs in the ascending row[0 .. d - 1]
GRX_HOST_DEVICE inline bool RowHolds(const int *row, int d, int x)
{
    int lo = 0, hi = d;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (row[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < d && row[lo] == x;
}

// the entries a device row of `length + 1` vertices takes: a multiple of 16, so that every row starts 64-byte aligned
GRX_HOST_DEVICE inline long long Pitch(long long length) { return (length + 1 + (kTileSteps - 1)) / kTileSteps * kTileSteps; }

struct Ctx {
    const int *ro;
    const int *ci;            // rows sorted by (column, weight)
    const long long *prefix;  // per entry, the inclusive weight prefix of its row; null when the walk is unweighted
    const int *starts;
    int *walks;
    int *lengths;
    unsigned long long *words;
    long long num_walks;
    long long pitch;
    uint64_t seed;
    int length;
    int b_return, b_in, b_out, amax;
    int biased;  // the three biases are not equal
    int tries;
};

struct Tally {
    unsigned long long steps = 0, ended = 0, tries = 0, forced = 0;
};

// the first-order choice at the row [b, e): an index into the row, or -1 when the walk ends here
__device__ __forceinline__ int Choose(const Ctx &c, int b, int e, uint64_t r)
{
    const int d = e - b;
    if (d == 0) return -1;
    if (!c.prefix) return ChooseUniform(r, d);
    if (c.prefix[e - 1] == 0) return -1;
    return ChooseWeighted(r, c.prefix + b, d);
}

// the vertex behind step s of walk w at v (from p), or -1
__device__ __forceinline__ int Step(const Ctx &c, uint64_t w, int s, int v, int p, Tally &t)
{
    const int b = c.ro[v], e = c.ro[v + 1];
    int k = Choose(c, b, e, Draw(c.seed, w, static_cast<uint64_t>(s), 0));
    if (k < 0) return -1;
    if (!c.biased || s == 0) return c.ci[b + k];
    const int pb = c.ro[p], pd = c.ro[p + 1] - pb;
    int x = 0;
    bool accepted = false;
    int j = 0;
    for (; j < c.tries && !accepted; ++j) {
        if (j) k = Choose(c, b, e, Draw(c.seed, w, static_cast<uint64_t>(s), static_cast<uint64_t>(2 * j)));
        x = c.ci[b + k];
        const int bias = x == p ? c.b_return : RowHolds(c.ci + pb, pd, x) ? c.b_in : c.b_out;
        const uint64_t a = ((Draw(c.seed, w, static_cast<uint64_t>(s), static_cast<uint64_t>(2 * j + 1)) >> 32) * static_cast<uint64_t>(c.amax)) >> 32;
        accepted = a < static_cast<uint64_t>(bias);
    }
    t.tries += static_cast<unsigned long long>(j);
    if (!accepted) ++t.forced;
    return x;
}

// every lane of the wave calls
__device__ __forceinline__ void Publish(const Ctx &c, const Tally &t)
{
    const unsigned long long steps = util::WaveSum(t.steps), ended = util::WaveSum(t.ended), tries = util::WaveSum(t.tries),
                             forced = util::WaveSum(t.forced);
    if (util::LaneId() == 0) {
        if (steps) atomicAdd(c.words + W_STEPS, steps);
        if (ended) atomicAdd(c.words + W_ENDED, ended);
        if (tries) atomicAdd(c.words + W_TRIES, tries);
        if (forced) atomicAdd(c.words + W_FORCED, forced);
    }
}

// ---------------- LANE ----------------

__global__ __launch_bounds__(kRwThreads) void LaneKernel(Ctx c)
{
    const long long stride = static_cast<long long>(gridDim.x) * kRwThreads;
    Tally t;
    for (long long w = static_cast<long long>(blockIdx.x) * kRwThreads + threadIdx.x; w < c.num_walks; w += stride) {
        int *row = c.walks + w * c.pitch;
        int v = c.starts[w], p = -1, count = 1;
        row[0] = v;
        for (int s = 0; s < c.length; ++s) {
            int next = -1;
            if (v >= 0) {
                next = Step(c, static_cast<uint64_t>(w), s, v, p, t);
                if (next >= 0) ++count;
            }
            row[s + 1] = next;
            p = v;
            v = next;
        }
        c.lengths[w] = count;
        t.steps += static_cast<unsigned long long>(count - 1);
        if (count <= c.length) ++t.ended;
    }
    Publish(c, t);
}

// ---------------- TILE ----------------

__global__ __launch_bounds__(kRwThreads) void TileKernel(Ctx c)
{
    __shared__ int s_tiles[kRwWaves][64 * kTileStride];
    const unsigned lane = util::LaneId();
    int *tile = s_tiles[threadIdx.x / 64];
    const long long wave0 = static_cast<long long>(blockIdx.x) * kRwWaves + threadIdx.x / 64;
    const long long nwaves = static_cast<long long>(gridDim.x) * kRwWaves;
    const long long groups = (c.num_walks + 63) / 64;
    const int columns = c.length + 1;
    Tally t;
    for (long long g = wave0; g < groups; g += nwaves) {  // (wave-uniform: every lane of a wave stays in the loop)
        const long long w = g * 64 + lane;
        const bool mine = w < c.num_walks;
        int v = mine ? c.starts[w] : -1, p = -1, count = mine ? 1 : 0;
        for (int first = 0; first < columns; first += kTileSteps) {
            const int valid = columns - first < kTileSteps ? columns - first : kTileSteps;  // columns of this tile
            for (int j = 0; j < valid; ++j) {
                const int s = first + j - 1;  // the step that gives this column; column 0 is the start vertex
                if (s >= 0) {
                    int next = -1;
                    if (v >= 0) {
                        next = Step(c, static_cast<uint64_t>(w), s, v, p, t);
                        if (next >= 0) ++count;
                    }
                    p = v;
                    v = next;
                }
                tile[lane * kTileStride + j] = v;
            }
            oprtr::lds::WaveLdsSync();
            // four lanes a row, 16 rows an instruction.  Unrolled on purpose: it costs 30 VGPRs (94, occupancy 5), and the kernel
            // at 64 VGPRs and occupancy 8 was 12 to 15 % slower in the weighted and biased modes
            const int part = static_cast<int>(lane & 3u) * 4;
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int r = pass * 16 + static_cast<int>(lane >> 2);
                const long long wr = g * 64 + r;
                if (wr < c.num_walks && part < valid) {
                    const int *src = tile + r * kTileStride + part;
                    int *dst = c.walks + wr * c.pitch + first + part;
                    if (part + 4 <= valid) {
                        *reinterpret_cast<int4 *>(dst) = make_int4(src[0], src[1], src[2], src[3]);
                    } else {
                        for (int i = 0; part + i < valid; ++i) dst[i] = src[i];
                    }
                }
            }
            oprtr::lds::WaveLdsSync();
        }
        if (mine) {
            c.lengths[w] = count;
            t.steps += static_cast<unsigned long long>(count - 1);
            if (count <= c.length) ++t.ended;
        }
    }
    Publish(c, t);
}

// ---------------- visits ----------------

__global__ void VisitsKernel(const int *walks, long long num_walks, int columns, long long pitch, unsigned long long *visits)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long total = num_walks * columns;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int v = walks[i / columns * pitch + i % columns];
        if (v >= 0) atomicAdd(visits + v, 1ull);
    }
}

}  // namespace rw
}  // namespace app
}  // namespace gunrock
