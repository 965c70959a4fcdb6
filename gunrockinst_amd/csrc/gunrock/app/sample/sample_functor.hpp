// app/sample/sample_functor.hpp -- neighbourhood sampling: the definition (host and device) and the kernels.
//
// The reference snapshot has no app/sample.  A sample is defined so that every output is an integer with one value (DESIGN.md 3.24;
// include/gunrock/gunrock_mi355x.h has the whole text).  In short: the rows are sorted by (column, weight, entry); the picks of a
// vertex v expanded at hop h are positions of its sorted row -- all of them (fanout -1, or replace = 0 and d <= f), Robert Floyd's
// subset over Draw(seed, v, h, s) (replace = 0, d > f), or f first-order choices of rw (replace = 1) -- and the distinct new columns
// of a hop take the next local ids in ascending vertex id.
//
// Kernels, per hop.  CountKernel: the picks of every frontier row (scanned into the rows' offsets by the caller).  LaneKernel or
// GroupKernel: the picks themselves, cols[] (still vertex ids) and eids[], and one bitmap bit per column without a local id.
// LongRowKernel: the rows a fanout of -1 found longer than "long_row", a workgroup per chunk.  BitCountKernel / FillKernel: the
// bitmap's set bits, counted per word, scanned by the caller, and written out as the new vertices in ascending id.  RelabelKernel:
// the hop's cols[] from vertex ids to local ids.  No atomic places an edge or decides an id: the only atomics set bitmap bits, append
// to the list of long rows (whose order nothing reads) and add up the counters.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include <gunrock/app/rw/rw_draw.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace sample {

enum { SAMPLE_AUTO = 0, SAMPLE_LANE = 1, SAMPLE_GROUP = 2 };

constexpr int kSampleThreads = 256;
constexpr int kSampleWaves = kSampleThreads / 64;
constexpr int kMaxFanout = 64;
constexpr int kMaxHops = 16;
constexpr int kAllNeighbours = -1;     // the fanout that takes whole rows
constexpr int kCopyGroup = 16;         // lanes of a group under the fanout -1
constexpr int kDefaultLongRow = 4096;
constexpr int kMinLongRow = 8;
constexpr int kSampleTooLarge = -4;    // GRX_SAMPLE_TOO_LARGE
constexpr long long kMaxEdgeLimit = 2147483647ll;

// words of the kernels: per hop the rows with drawn picks, the rows copied whole and the long rows
enum { W_SAMPLED = 0, W_COPIED = kMaxHops, W_LONG = 2 * kMaxHops, W_COUNT = 3 * kMaxHops };

// ---------------- the definition ----------------

// Draw(seed, v, hop, s) is rw's Draw(seed, walk = v, step = hop, t = s)
GRX_HOST_DEVICE inline uint64_t Draw(uint64_t seed, int v, int hop, int s)
{
    return rw::Draw(seed, static_cast<uint64_t>(v), static_cast<uint64_t>(hop), static_cast<uint64_t>(s));
}

GRX_HOST_DEVICE inline bool ValidFanout(int f) { return f == kAllNeighbours || (f >= 1 && f <= kMaxFanout); }

// whether the picks of a row of d entries under the fanout f are the whole row in order
GRX_HOST_DEVICE inline bool WholeRow(int d, int f, int replace) { return f == kAllNeighbours || (!replace && d <= f); }

// the picks of a row of d entries; `total`: the row's weight total when weighted, anything positive else
GRX_HOST_DEVICE inline int PickCount(int d, int f, int replace, long long total)
{
    if (f == kAllNeighbours) return d;
    if (!replace) return d < f ? d : f;
    return d == 0 || total <= 0 ? 0 : f;
}

// the lanes of a group: the power of two with f <= g <= 64
GRX_HOST_DEVICE inline int GroupWidth(int f)
{
    if (f == kAllNeighbours) return kCopyGroup;
    int g = 1;
    while (g < f) g <<= 1;
    return g;
}

// slot s of Floyd's subset of f out of d > f positions: the candidate, before the collision rule
GRX_HOST_DEVICE inline int FloydCandidate(uint64_t seed, int v, int hop, int s, int d, int f)
{
    const int i = d - f + s;
    return static_cast<int>(((Draw(seed, v, hop, s) >> 32) * static_cast<uint64_t>(i + 1)) >> 32);
}

// the f picks, in slot order: the candidate, unless it equals an earlier pick of the row; then i = d - f + s
GRX_HOST_DEVICE inline void FloydPicks(uint64_t seed, int v, int hop, int d, int f, int *picks)
{
    for (int s = 0; s < f; ++s) {
        int t = FloydCandidate(seed, v, hop, s, d, f);
        for (int j = 0; j < s; ++j)
            if (picks[j] == t) {
                t = d - f + s;
                break;
            }
        picks[s] = t;
    }
}

// ---------------- the kernels ----------------

struct Ctx {
    const int *ro;            // the sorted copy
    const int *ci;
    const int *ent;           // per sorted position, the caller's entry
    const long long *prefix;  // per entry, the inclusive weight prefix of its row; null unless the sample is weighted
    const int *vertices;      // of every local id
    const unsigned long long *row_base;  // per frontier row, its first edge within the hop
    long long *offsets;
    int *cols;
    int *eids;  // null when the entries are not gathered
    const int *local;
    unsigned *bitmap;
    int *long_rows;  // the frontier rows left to LongRowKernel
    unsigned long long *words;
    long long first;      // local id of the frontier's first vertex
    long long count;      // frontier vertices
    long long edge_base;  // edges before this hop
    uint64_t seed;
    int hop, f, replace, long_row;
};

static __global__ void CountKernel(const int *ro, const long long *prefix, const int *vertices, long long first, long long cap,
                                   const unsigned long long *d_count, long long count, int hop, int f, int replace, unsigned *counts,
                                   unsigned long long *words)
{
    // the frontier's size: the caller's, or what the renumbering of the hop before left on the device
    long long n = d_count ? static_cast<long long>(*d_count) : count;
    if (n > cap) n = cap;  // (cap bounds it: the arrays hold no more)
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned long long sampled = 0, copied = 0;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i <= cap; i += stride) {
        unsigned c = 0;
        if (i < n) {
            const int v = vertices[first + i];
            const int b = ro[v], d = ro[v + 1] - b;
            c = static_cast<unsigned>(PickCount(d, f, replace, prefix && d ? prefix[b + d - 1] : 1));
            if (WholeRow(d, f, replace)) ++copied;
            else if (c) ++sampled;
        }
        counts[i] = c;
    }
    sampled = util::WaveSum(sampled);
    copied = util::WaveSum(copied);
    if (util::LaneId() == 0) {
        if (sampled) atomicAdd(words + W_SAMPLED + hop, sampled);
        if (copied) atomicAdd(words + W_COPIED + hop, copied);
    }
}

// one sampled edge: position k of the sorted copy into slot `at`
__device__ __forceinline__ void Emit(const Ctx &c, long long at, int k)
{
    const int col = c.ci[k];
    c.cols[at] = col;
    if (c.eids) c.eids[at] = c.ent[k];
    if (c.local[col] < 0) {
        // a bit only goes from 0 to 1 while a hop's sampler runs, so a set bit read here is set, and a stale 0 costs one atomic
        // more: a hub's bit is set once, not once per pick of it
        unsigned *word = c.bitmap + (col >> 5);
        const unsigned bit = 1u << (col & 31);
        if (!(*word & bit)) atomicOr(word, bit);
    }
}

// position of a choice with replacement in the row [b, b + d), d > 0 (weighted: a positive total)
__device__ __forceinline__ int Choice(const Ctx &c, int b, int d, uint64_t r)
{
    return c.prefix ? rw::ChooseWeighted(r, c.prefix + b, d) : rw::ChooseUniform(r, d);
}

__device__ __forceinline__ bool RowHasPicks(const Ctx &c, int b, int d) { return d > 0 && (!c.prefix || c.prefix[b + d - 1] > 0); }

// ---------------- LANE: a lane per frontier vertex, its picks in an LDS strip [slot][thread] ----------------

// the bytes of LaneKernel's strip: f slots of a workgroup's threads where picks are drawn without replacement, nothing else
GRX_HOST_DEVICE inline size_t LaneStripBytes(int f, int replace)
{
    return f == kAllNeighbours || replace ? 0 : sizeof(int) * static_cast<size_t>(f) * kSampleThreads;
}

__global__ __launch_bounds__(kSampleThreads) void LaneKernel(Ctx c)
{
    extern __shared__ int s_strip[];  // LaneStripBytes(c.f, c.replace)
    int(*s_picks)[kSampleThreads] = reinterpret_cast<int(*)[kSampleThreads]>(s_strip);
    const long long stride = static_cast<long long>(gridDim.x) * kSampleThreads;
    const int tid = threadIdx.x;
    for (long long i = static_cast<long long>(blockIdx.x) * kSampleThreads + tid; i < c.count; i += stride) {
        const int v = c.vertices[c.first + i];
        const int b = c.ro[v], d = c.ro[v + 1] - b;
        const long long out = c.edge_base + static_cast<long long>(c.row_base[i]);
        c.offsets[c.first + i] = out;
        if (WholeRow(d, c.f, c.replace)) {
            if (c.f == kAllNeighbours && d > c.long_row) {
                c.long_rows[atomicAdd(c.words + W_LONG + c.hop, 1ull)] = static_cast<int>(i);
            } else {
                for (int k = 0; k < d; ++k) Emit(c, out + k, b + k);
            }
        } else if (!c.replace) {
            for (int s = 0; s < c.f; ++s) {
                int t = FloydCandidate(c.seed, v, c.hop, s, d, c.f);
                bool seen = false;
                for (int j = 0; j < s; ++j) seen |= s_picks[j][tid] == t;
                if (seen) t = d - c.f + s;
                s_picks[s][tid] = t;
                Emit(c, out + s, b + t);
            }
        } else if (RowHasPicks(c, b, d)) {
            for (int s = 0; s < c.f; ++s) Emit(c, out + s, b + Choice(c, b, d, Draw(c.seed, v, c.hop, s)));
        }
    }
}

// ---------------- GROUP: g lanes per frontier vertex, 64 / g vertices per wave ----------------

__global__ __launch_bounds__(kSampleThreads) void GroupKernel(Ctx c, int g)
{
    const int lane = static_cast<int>(util::LaneId());
    const int sub = lane & (g - 1), head = lane - sub, per_wave = 64 / g;
    const long long wave0 = static_cast<long long>(blockIdx.x) * kSampleWaves + threadIdx.x / 64;
    const long long nwaves = static_cast<long long>(gridDim.x) * kSampleWaves;
    const long long tiles = (c.count + per_wave - 1) / per_wave;
    for (long long tile = wave0; tile < tiles; tile += nwaves) {  // (wave-uniform: every lane of a wave stays in the loop)
        const long long i = tile * per_wave + lane / g;
        const bool mine = i < c.count;
        int v = 0, b = 0, d = 0;
        long long out = 0;
        if (mine) {
            v = c.vertices[c.first + i];
            b = c.ro[v];
            d = c.ro[v + 1] - b;
            out = c.edge_base + static_cast<long long>(c.row_base[i]);
            if (sub == 0) c.offsets[c.first + i] = out;
        }
        const bool whole = WholeRow(d, c.f, c.replace);
        if (c.f != kAllNeighbours && !c.replace) {
            // Floyd's subset: every lane its own slot's candidate at once, then f - 1 rounds; in round s lane s of the group holds
            // its resolved pick, and every later lane whose candidate equals it takes its own i instead (an i is above every
            // earlier pick, so a lane that moved once never matches again)
            const bool drawn = mine && !whole && sub < c.f;
            int pick = drawn ? FloydCandidate(c.seed, v, c.hop, sub, d, c.f) : -1 - sub;
            for (int s = 0; s + 1 < c.f; ++s) {  // (c.f is uniform: no lane leaves in front of the cross-lane read)
                const int fixed = __shfl(pick, head + s, 64);
                if (drawn && sub > s && pick == fixed) pick = d - c.f + sub;
            }
            if (drawn) Emit(c, out + sub, b + pick);
        } else if (c.f != kAllNeighbours) {
            if (mine && sub < c.f && RowHasPicks(c, b, d)) Emit(c, out + sub, b + Choice(c, b, d, Draw(c.seed, v, c.hop, sub)));
        }
        if (mine && whole) {
            if (c.f == kAllNeighbours && d > c.long_row) {
                if (sub == 0) c.long_rows[atomicAdd(c.words + W_LONG + c.hop, 1ull)] = static_cast<int>(i);
            } else {
                for (int k = sub; k < d; k += g) Emit(c, out + k, b + k);
            }
        }
    }
}

// the listed rows in chunks of long_row entries, chunk j of the list's running count to workgroup j mod the grid
__global__ __launch_bounds__(kSampleThreads) void LongRowKernel(Ctx c)
{
    const long long rows = static_cast<long long>(c.words[W_LONG + c.hop]);
    long long chunk = 0;
    for (long long r = 0; r < rows; ++r) {  // (the same for every workgroup)
        const long long i = c.long_rows[r];
        const int v = c.vertices[c.first + i];
        const int b = c.ro[v], d = c.ro[v + 1] - b;
        const long long out = c.edge_base + static_cast<long long>(c.row_base[i]);
        for (int from = 0; from < d; from += c.long_row, ++chunk) {
            if (chunk % gridDim.x != blockIdx.x) continue;
            const int to = d - from < c.long_row ? d : from + c.long_row;
            for (int k = from + static_cast<int>(threadIdx.x); k < to; k += kSampleThreads) Emit(c, out + k, b + k);
        }
    }
}

// ---------------- renumbering ----------------

static __global__ void BitCountKernel(const unsigned *bitmap, long long words32, unsigned *counts)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long w = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; w < words32; w += stride)
        counts[w] = static_cast<unsigned>(__popc(bitmap[w]));
}

// the set bits in ascending order take the local ids from `first` on; the bits are cleared
static __global__ void FillKernel(unsigned *bitmap, long long words32, const unsigned long long *base, long long first, int *vertices, int *local)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long w = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; w < words32; w += stride) {
        unsigned bits = bitmap[w];
        if (!bits) continue;
        bitmap[w] = 0;
        long long id = first + static_cast<long long>(base[w]);
        while (bits) {
            const int v = static_cast<int>(w * 32) + (__ffs(bits) - 1);
            bits &= bits - 1;
            vertices[id] = v;
            local[v] = static_cast<int>(id);
            ++id;
        }
    }
}

// offsets[first .. first + n] = edges, n the caller's `count` or *d_new: the rows of a new frontier are empty until a hop expands them
static __global__ void EmptyRowsKernel(long long *offsets, long long first, const unsigned long long *d_new, long long count, long long edges)
{
    const long long n = d_new ? static_cast<long long>(*d_new) : count;
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i <= n; i += stride) offsets[first + i] = edges;
}

static __global__ void RelabelKernel(int *cols, long long from, long long to, const int *local)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = from + static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < to; e += stride) cols[e] = local[cols[e]];
}

// ---------------- Reset ----------------

static __global__ void ClearLocalKernel(const int *vertices, long long count, int *local)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) local[vertices[i]] = -1;
}

static __global__ void SeedLocalKernel(const int *vertices, long long count, int *local)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) local[vertices[i]] = static_cast<int>(i);
}

}  // namespace sample
}  // namespace app
}  // namespace gunrock
