// app/sm/sm_functor.hpp -- kernels of subgraph matching: the work bound, the bins, the depth-first enumeration, the division.
//
// The reference snapshot has no working app/sm; the shape follows app/clique.  G is the mirrored neighbour CSR of
// graphio::PairGraph::Rows (rows ascending by id, no self-loops, no duplicates), `src` the row of every entry, `deg` the row lengths,
// `labels` one int32 per vertex or NULL (all 0).  The plan (sm_plan.hpp) comes by value.
//
// A work item is an entry (v, u) of the CSR, read as f(order[0]) = v and f(order[1]) = u.  BinKernel tests what levels 0 and 1 ask
// (label, degree, lt / gt) and appends the entry to the list of its regime; for q = 2 the item is the occurrence and is credited
// there.  EnumerateKernel<Q, G>: a group of G lanes (8 or 64) owns an item and runs the search below it.  Level l streams the row of
// its anchor -- the image of a level in must[l], the one with the shortest row -- G entries at a time; every lane tests its
// candidate (label, degree, distinct from the earlier images, lt / gt, adjacency to the other must levels and non-adjacency to the
// mustnot levels by bisecting the shorter of the two rows); a ballot gives the survivors.  The last level adds the popcount; above
// it the group descends into the survivors one at a time.  The state of a level -- the chunk, the survivor mask, the cursor -- is
// locals of Search<L>, which the template unrolls: no array is indexed at run time, nothing is kept in LDS or in global scratch.
// Credits as in app/clique: +1 on count[c] for a last-level survivor, the number found beneath a vertex fixed above when its level
// is left, the item's subtotal onto the total once.  Integer adds commute: both group widths write the same arrays.
// No kernel waits on another workgroup; every loop is bounded by a row length or by Q.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/sm/sm_plan.hpp>
#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace sm {

typedef unsigned long long Count;

enum { SM_AUTO = 0, SM_GROUP8 = 1, SM_WAVE = 2 };

constexpr int kGroupMaxRow = 16;  // default "group_max_row" (by reasoning)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / util::kWaveSize;

// d_words
enum { W_ITEMS8 = 0, W_ITEMS64 = 1, W_BAD = 2, W_COUNT = 4 };
// d_counters
enum { C_TOTAL = 0, C_STREAMED = 1, C_BISECTIONS = 2, C_COUNT = 4 };

struct Graph {
    const int *ro, *ci, *src;
    const unsigned *deg;
    const int *labels;  // or NULL
    int nodes;
    long long entries;  // 2M
};

__device__ __forceinline__ bool LabelFits(const Graph &g, int v, int plabel) { return plabel == kWildcard || (g.labels ? g.labels[v] : 0) == plabel; }

// ---------------- the work bound ----------------

// h[parent][v] *= sum over u in N(v) of h[child][u]: one edge of the anchor tree, leaf to root
static __global__ void BoundRowKernel(Graph g, const double *d_child, double *d_parent)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < g.nodes; v += stride) {
        double s = 0;
        for (int e = g.ro[v]; e < g.ro[v + 1]; ++e) s += d_child[g.ci[e]];
        d_parent[v] *= s;
    }
}

// *d_bound += sum of h[root][v]
static __global__ void BoundSumKernel(const double *d_root, long long nodes, double *d_bound)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    double s = 0;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) s += d_root[v];
    s = util::WaveSum(s);
    if (util::LaneId() == 0 && s > 0) atomicAdd(d_bound, s);
}

// d_src[e] = the row of entry e, d_deg[v] = the length of row v, *d_longest = the longest; one thread per vertex
static __global__ void RowOfEntryKernel(const int *d_ro, long long nodes, int *d_src, unsigned *d_deg, unsigned *d_longest)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    unsigned longest = 0;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int begin = d_ro[v], end = d_ro[v + 1];
        for (int e = begin; e < end; ++e) d_src[e] = static_cast<int>(v);
        d_deg[v] = static_cast<unsigned>(end - begin);
        longest = longest > static_cast<unsigned>(end - begin) ? longest : static_cast<unsigned>(end - begin);
    }
    if (longest) atomicMax(d_longest, longest);
}

// ---------------- binning ----------------

__host__ __device__ __forceinline__ int RegimeOf(unsigned len_a, unsigned len_b, int strategy, int group_max_row)
{
    if (strategy != SM_AUTO) return strategy;
    const unsigned longer = len_a > len_b ? len_a : len_b;
    return longer <= static_cast<unsigned>(group_max_row) ? SM_GROUP8 : SM_WAVE;
}

// The entries that pass levels 0 and 1 go to the list of their regime; with q = 2 they are the occurrences: credited here.
static __global__ void BinKernel(Graph g, PlanLevels plan, int strategy, int group_max_row, int per_vertex, int *d_items8, int *d_items64,
                                 unsigned *d_words, Count *d_count, Count *d_counters)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const Level l0 = plan.level[0], l1 = plan.level[1];
    const long long rounds = (g.entries + stride - 1) / stride;  // every lane of a wave makes as many rounds: the ballots are whole
    long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (long long r = 0; r < rounds; ++r, e += stride) {
        bool ok = e < g.entries;
        int v = 0, u = 0, regime = SM_GROUP8;
        if (ok) {
            v = g.src[e];
            u = g.ci[e];
            const unsigned dv = g.deg[v], du = g.deg[u];
            ok = dv >= static_cast<unsigned>(l0.min_degree) && du >= static_cast<unsigned>(l1.min_degree) && LabelFits(g, v, l0.plabel) &&
                 LabelFits(g, u, l1.plabel) && !((l1.lt & 1u) && u >= v) && !((l1.gt & 1u) && u <= v);
            regime = RegimeOf(dv, du, strategy, group_max_row);
        }
        if (plan.q == 2) {
            const unsigned long long mask = __ballot(ok);
            if (!mask) continue;
            if (ok && per_vertex) {
                atomicAdd(d_count + v, 1ull);
                atomicAdd(d_count + u, 1ull);
            }
            if (util::LaneId() == 0) atomicAdd(d_counters + C_TOTAL, static_cast<Count>(__popcll(mask)));
            continue;
        }
        {
            const bool hit = ok && regime == SM_GROUP8;
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                const unsigned pos = oprtr::WaveTicket(d_words + W_ITEMS8, mask);
                if (hit) d_items8[pos] = static_cast<int>(e);
            }
        }
        {
            const bool hit = ok && regime == SM_WAVE;
            const unsigned long long mask = __ballot(hit);
            if (mask) {
                const unsigned pos = oprtr::WaveTicket(d_words + W_ITEMS64, mask);
                if (hit) d_items64[pos] = static_cast<int>(e);
            }
        }
    }
}

// ---------------- the enumeration ----------------

// a -- b in G: the shorter of the two rows bisected for the other vertex, at most 32 steps
__device__ __forceinline__ bool Adjacent(const Graph &g, int a, unsigned len_a, int b, unsigned len_b)
{
    const int row = len_a <= len_b ? a : b, x = len_a <= len_b ? b : a;
    int lo = g.ro[row];
    const int end = g.ro[row + 1];
    int hi = end;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (g.ci[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < end && g.ci[lo] == x;
}

// What a group carries down the levels.  img[] and len[] are indexed by constants only (the levels are unrolled).
template <int Q>
struct Walk {
    int img[Q];
    unsigned len[Q];  // the row lengths of the images
    unsigned long long streamed, bisections;
};

// The search at level L below the images of levels 0 .. L - 1: returns what the group found, the same in all its lanes.
// `sub` is the lane within its group, `shift` the group's first lane.
template <int Q, int G, int L>
__device__ __forceinline__ Count Search(const Graph &g, const PlanLevels &plan, Walk<Q> &w, const int sub, const int shift, const int per_vertex,
                                        Count *d_count)
{
    if constexpr (L >= Q) {
        return 0;
    } else {
        const Level lv = plan.level[L];
        // the anchor: the must level whose image has the shortest row
        int anchor = 0, at = 0;
        unsigned alen = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < L; ++j)
            if ((lv.must >> j & 1u) && w.len[j] < alen) {
                anchor = w.img[j];
                alen = w.len[j];
                at = j;
            }
        const int base = g.ro[anchor];
        const int end = static_cast<int>(alen);
        Count found = 0;
        for (int cursor = 0; cursor < end; cursor += G) {
            const int idx = cursor + sub;
            bool ok = idx < end;
            int c = -1;
            unsigned clen = 0;
            if (ok) {
                c = g.ci[base + idx];
                clen = g.deg[c];
                ++w.streamed;
                ok = clen >= static_cast<unsigned>(lv.min_degree) && LabelFits(g, c, lv.plabel);
            }
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const int other = w.img[j];
                ok = ok && c != other && !((lv.lt >> j & 1u) && c >= other) && !((lv.gt >> j & 1u) && c <= other);
            }
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const bool must = lv.must >> j & 1u, mustnot = lv.mustnot >> j & 1u;
                if (ok && j != at && (must || mustnot)) {
                    ++w.bisections;
                    ok = Adjacent(g, c, clen, w.img[j], w.len[j]) == must;
                }
            }
            const unsigned long long ballot = __ballot(ok);
            unsigned long long mask = G == 64 ? ballot : (ballot >> shift) & ((1ull << (G & 63)) - 1ull);
            if constexpr (L == Q - 1) {
                found += static_cast<Count>(__popcll(mask));
                if (ok && per_vertex) atomicAdd(d_count + c, 1ull);
            } else {
                while (mask) {
                    const int bit = __ffsll(static_cast<long long>(mask)) - 1;
                    mask &= mask - 1ull;
                    w.img[L] = __shfl(c, shift + bit, util::kWaveSize);
                    w.len[L] = __shfl(clen, shift + bit, util::kWaveSize);
                    const Count below = Search<Q, G, L + 1>(g, plan, w, sub, shift, per_vertex, d_count);
                    if (below && per_vertex && sub == 0) atomicAdd(d_count + w.img[L], below);
                    found += below;
                }
            }
        }
        return found;
    }
}

// One group of G lanes per item of d_items[0 .. *d_item_count), group-stride.  Q >= 3.
template <int Q, int G>
__launch_bounds__(kThreads) static __global__ void EnumerateKernel(Graph g, PlanLevels plan, const int *d_items, const unsigned *d_item_count,
                                                                    int per_vertex, Count *d_count, Count *d_counters)
{
    constexpr int kGroups = util::kWaveSize / G;
    const int lane = static_cast<int>(util::LaneId());
    const int sub = lane % G, shift = lane - sub;
    const long long items = *d_item_count;
    const long long stride = static_cast<long long>(gridDim.x) * kWaves * kGroups;
    Walk<Q> w;
    w.streamed = w.bisections = 0;
    Count total = 0;
    for (long long i = (static_cast<long long>(blockIdx.x) * kWaves + threadIdx.x / util::kWaveSize) * kGroups + lane / G; i < items; i += stride) {
        const int e = d_items[i];
        w.img[0] = g.src[e];
        w.img[1] = g.ci[e];
        w.len[0] = g.deg[w.img[0]];
        w.len[1] = g.deg[w.img[1]];
        const Count found = Search<Q, G, 2>(g, plan, w, sub, shift, per_vertex, d_count);
        if (found && sub == 0) {
            if (per_vertex) {
                atomicAdd(d_count + w.img[0], found);
                atomicAdd(d_count + w.img[1], found);
            }
            total += found;
        }
    }
    // (all lanes are here again)
    total = util::WaveSum(total);
    const unsigned long long streamed = util::WaveSum(w.streamed), bisections = util::WaveSum(w.bisections);
    if (lane == 0) {
        if (total) atomicAdd(d_counters + C_TOTAL, total);
        if (streamed) atomicAdd(d_counters + C_STREAMED, streamed);
        if (bisections) atomicAdd(d_counters + C_BISECTIONS, bisections);
    }
}

// ---------------- the division ----------------

// Without symmetry breaking every occurrence was found `aut` times: count[] and the total divided, W_BAD set by a remainder
static __global__ void FinishKernel(Count *d_count, long long nodes, Count *d_counters, unsigned aut, unsigned *d_words)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    bool bad = false;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v <= nodes; v += stride) {
        Count *at = v < nodes ? d_count + v : d_counters + C_TOTAL;
        const Count x = *at;
        bad |= x % aut != 0;
        *at = x / aut;
    }
    if (bad) d_words[W_BAD] = 1u;
}

}  // namespace sm
}  // namespace app
}  // namespace gunrock
