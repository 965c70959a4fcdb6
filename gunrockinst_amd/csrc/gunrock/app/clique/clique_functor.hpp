// app/clique/clique_functor.hpp -- kernels of k-clique counting (k = 3 .. 6): the rank-aware orientation, the bins, the LDS
// bit-matrix rows and the list rows.
//
// The reference snapshot has no app/clique; the shape follows app/tc.  The oriented CSR (clique_problem.hpp) holds every edge of the
// simple undirected graph once, from the endpoint with the smaller (rank, peel round, d, id) to the larger, rows ascending by id.  Under a total
// order a k-clique appears exactly once: at its smallest member u, as a (k - 1)-clique of the DAG that N+(u) induces, its members
// m1 -> m2 -> ... -> m(k-1) in the order.  Two regimes, picked per row u by its length r (BinKernel):
//   bitmap  one workgroup per row: R = N+(u) staged in LDS, then the r x ceil(r / 32)-word bit matrix B, bit j of row i set iff R[j]
//           is in N+(R[i]) (waves stream N+(R[i]) with coalesced loads, every lane bisects the staged R, LDS atomic OR).  A wave takes
//           a first member i and holds a bit row as one word per lane: P1 = B[i], P(l+1) = P(l) & B[j] for every set bit j of P(l),
//           iterated wave-uniformly, the row of a level in one VGPR (r <= 1024 here, a wave holds 2048 bits); the last level is a
//           popcount.  Credits go to 64-bit LDS counters, one per entry of R: +1 per clique for every set bit of the last P, the count
//           found under it for a member fixed above; flushed with one global atomic per non-zero counter, u's credit one per row.
//   list    one single-wave workgroup per oriented edge (u, v): S1 = N+(u) ^ N+(v) as a sorted list into the workgroup's slab of
//           global scratch, S(l+1) = S(l) ^ N+(m) for every m of S(l) by bisection of N+(m), compacted in order with a ballot; the
//           last level is the list's length.  Credits are global 64-bit atomics.  Any row length.
// Integer adds commute: both regimes write the same arrays.
#pragma once

#include <hip/hip_runtime.h>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // (only TC's build kernels and its bisection are used here)
#include <gunrock/app/tc/tc_functor.hpp>
#pragma clang diagnostic pop
#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace clique {

using tc::Count;
using tc::LowerBound;
using tc::Oriented;

enum { CLIQUE_AUTO = 0, CLIQUE_BITMAP = 1, CLIQUE_LIST = 2 };

constexpr int kMinK = 3, kMaxK = 6;
constexpr int kBitmapThreads = 256;  // 4 waves per row (not measured)
constexpr int kBitmapWaves = kBitmapThreads / util::kWaveSize;
constexpr int kBitmapRows = 512;      // default "bitmap_rows": B takes 32 KiB (not measured)
constexpr int kBitmapRowsMin = 32;
constexpr int kBitmapRowsMax = 1024;  // B takes 128 KiB of the CU's 160
constexpr int kListThreads = util::kWaveSize;

// dynamic LDS of the bitmap kernel for rows of up to `cap` entries: the counters, the ids, the matrix
__host__ __device__ __forceinline__ size_t BitmapLdsBytes(int cap)
{
    return sizeof(Count) * static_cast<size_t>(cap) + sizeof(int) * static_cast<size_t>(cap) +
           sizeof(unsigned) * static_cast<size_t>(cap) * static_cast<size_t>((cap + 31) / 32);
}

// ---------------- the build ----------------

// tc::OrientKernel with the rank in front: every kept edge points from the endpoint with the smaller (rank, round, d, id).
// Without a rank (d_rank and d_round NULL) the keys are PairGraph's sorted ones with their keep flags and positions; with one they
// are its compacted canonical keys (d_keep and d_pos NULL) and d_round holds the peel rounds of RankPeel*Kernel.
static __global__ void RankOrientKernel(const unsigned long long *d_keys, const unsigned *d_keep, const unsigned long long *d_pos, long long count,
                                        int col_bits, const int *d_rank, const unsigned *d_round, const unsigned *d_deg,
                                        unsigned long long *d_okeys, unsigned *d_outdeg)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (d_keep && !d_keep[i]) continue;
        const unsigned long long k = d_keys[i];
        const unsigned a = static_cast<unsigned>(k >> col_bits), b = static_cast<unsigned>(k & mask);  // a < b
        const int ra = d_rank ? d_rank[a] : 0, rb = d_rank ? d_rank[b] : 0;
        const unsigned ta = d_round ? d_round[a] : 0u, tb = d_round ? d_round[b] : 0u;
        const bool a_first = ra != rb ? ra < rb : ta != tb ? ta < tb : d_deg[a] <= d_deg[b];  // all equal: the smaller id, a
        const unsigned s = a_first ? a : b, t = a_first ? b : a;
        d_okeys[d_pos ? d_pos[i] : static_cast<unsigned long long>(i)] = (static_cast<unsigned long long>(s) << col_bits) | t;
        atomicAdd(d_outdeg + s, 1u);
    }
}

// The peel that breaks ties of the rank.  live(v) = the neighbours of v whose rank is not smaller; v leaves in the first round at
// whose start live(v) <= max(rank[v], 0), and takes one off live(w) of every neighbour w of its own rank that is still there.
// A vertex that left in round t has at most max(rank, 0) neighbours behind it in the order (rank, round, d, id): the ones of
// higher rank, and of its own rank the ones that left in its round or later.  With core numbers as the rank every vertex leaves
// (the shell of core c is what the peel of the c-core removes at level c), so no out-row exceeds the degeneracy; with all ranks
// equal and <= 0 only isolated vertices leave and the order is TC's (d, id).  A vertex that never leaves keeps round UINT_MAX.
// ro / ci: the mirrored neighbour CSR of PairGraph::Rows.  One wave per vertex.
constexpr unsigned kNeverPeeled = 0xFFFFFFFFu;

static __global__ void RankPeelInitKernel(const int *d_ro, const int *d_ci, const int *d_rank, int nodes, int *d_live, unsigned *d_round,
                                          int *d_list, int *d_list_count)
{
    const unsigned lane = util::LaneId();
    const long long waves = static_cast<long long>(gridDim.x) * (blockDim.x / util::kWaveSize);
    for (long long v = static_cast<long long>(blockIdx.x) * (blockDim.x / util::kWaveSize) + threadIdx.x / util::kWaveSize; v < nodes; v += waves) {
        const int r = d_rank[v];
        int live = 0;
        for (int e = d_ro[v] + static_cast<int>(lane); e < d_ro[v + 1]; e += util::kWaveSize) live += d_rank[d_ci[e]] >= r ? 1 : 0;
        live = util::WaveSum(live);
        if (lane == 0) {
            const bool leaves = live <= (r > 0 ? r : 0);
            d_live[v] = live;
            d_round[v] = leaves ? 0u : kNeverPeeled;
            if (leaves) d_list[atomicAdd(d_list_count, 1)] = static_cast<int>(v);
        }
    }
}

// the vertices of d_list left in `round`; those they push to their threshold leave in round + 1
static __global__ void RankPeelRoundKernel(const int *d_ro, const int *d_ci, const int *d_rank, const int *d_list, int list_count, unsigned round,
                                           int *d_live, unsigned *d_round, int *d_next, int *d_next_count)
{
    const unsigned lane = util::LaneId();
    const int waves = gridDim.x * (blockDim.x / util::kWaveSize);
    for (int i = blockIdx.x * (blockDim.x / util::kWaveSize) + threadIdx.x / util::kWaveSize; i < list_count; i += waves) {
        const int v = d_list[i];
        const int r = d_rank[v];
        for (int e = d_ro[v] + static_cast<int>(lane); e < d_ro[v + 1]; e += util::kWaveSize) {
            const int w = d_ci[e];
            if (d_rank[w] != r || util::LoadAgent(d_round + w) <= round) continue;  // another rank, or gone already
            if (atomicSub(d_live + w, 1) - 1 == (r > 0 ? r : 0)) {  // the one decrement that reaches the threshold
                d_round[w] = round + 1;
                d_next[atomicAdd(d_next_count, 1)] = w;
            }
        }
    }
}

// d_bound[k - 3] += C(d+(u), k - 1) over every row, k = 3 .. 6, in float64
static __global__ void BoundKernel(const int *d_oro, long long nodes, double *d_bound)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    double sum[4] = {0, 0, 0, 0};
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const double d = static_cast<double>(d_oro[v + 1] - d_oro[v]);
        double c = d;  // C(d, 1)
        for (int j = 2; j <= 5; ++j) {
            c = d >= j ? c * (d - (j - 1)) / j : 0.0;
            sum[j - 2] += c;  // C(d, j) bounds k = j + 1
        }
    }
    for (int i = 0; i < 4; ++i) {
        const double s = util::WaveSum(sum[i]);
        if (util::LaneId() == 0 && s > 0) atomicAdd(d_bound + i, s);
    }
}

// ---------------- binning ----------------

__host__ __device__ __forceinline__ int RegimeOf(int len, int strategy, int bitmap_rows)
{
    if (strategy == CLIQUE_LIST) return CLIQUE_LIST;
    const int limit = strategy == CLIQUE_BITMAP ? kBitmapRowsMax : bitmap_rows;
    return len <= limit ? CLIQUE_BITMAP : CLIQUE_LIST;
}

// d_words[0]: bitmap rows listed; [1]: oriented edges listed for the list regime; [2]: their rows; [3]: the bitmap rows' edges.
// A row of fewer than min_len = k - 1 entries is nobody's: a clique found at u has its other k - 1 members in N+(u).
static __global__ void BinKernel(const int *d_oro, int nodes, int min_len, int strategy, int bitmap_rows, int *d_bitmap_rows, int *d_list_edges,
                                 int *d_words)
{
    const int stride = gridDim.x * blockDim.x;
    for (long long u = blockIdx.x * blockDim.x + threadIdx.x; u < nodes; u += stride) {
        const int ub = d_oro[u], len = d_oro[u + 1] - ub;
        if (len < min_len) continue;
        if (RegimeOf(len, strategy, bitmap_rows) == CLIQUE_BITMAP) {
            d_bitmap_rows[atomicAdd(d_words, 1)] = static_cast<int>(u);
            atomicAdd(d_words + 3, len);
        } else {
            const int at = atomicAdd(d_words + 1, len);
            atomicAdd(d_words + 2, 1);
            for (int i = 0; i < len; ++i) d_list_edges[at + i] = ub + i;
        }
    }
}

// ---------------- the bitmap regime ----------------

// The (REMAIN)-member completions of the candidates p (this lane's word of the bit row; lanes beyond `words` hold 0).  Returns the
// count in every lane; credits every member it fixes.  ands: bit-row ANDs, counted by lane 0.
template <int REMAIN>
__device__ __forceinline__ Count BitDescend(unsigned p, const unsigned *s_bits, int words, unsigned lane, Count *s_cnt, Count &ands)
{
    if constexpr (REMAIN == 1) {
        const unsigned c = util::WaveSum(static_cast<unsigned>(__popc(p)));
        for (unsigned w = p; w; w &= w - 1) atomicAdd(&s_cnt[lane * 32 + (__ffs(w) - 1)], 1ull);
        return c;
    } else {
        Count sum = 0;
        for (int w = 0; w < words; ++w) {
            unsigned word = __shfl(p, w, util::kWaveSize);  // the same in every lane: the loop is wave-uniform
            for (; word; word &= word - 1) {
                const int j = w * 32 + (__ffs(word) - 1);
                const unsigned q = lane < static_cast<unsigned>(words) ? p & s_bits[j * words + lane] : 0u;
                ++ands;
                if (!__ballot(q != 0)) continue;
                const Count c = BitDescend<REMAIN - 1>(q, s_bits, words, lane, s_cnt, ands);
                if (c && lane == 0) atomicAdd(&s_cnt[j], c);
                sum += c;
            }
        }
        return sum;
    }
}

// One workgroup per listed row; dynamic LDS: BitmapLdsBytes(cap), every listed row has at most cap entries.
// d_counters[0] cliques, [1] bit-row ANDs
template <int K>
static __global__ __launch_bounds__(kBitmapThreads) void BitmapKernel(Oriented g, const int *d_rows, const int *d_row_count, int cap, Count *d_cliques,
                                                                      Count *d_counters)
{
    extern __shared__ Count s_dyn64[];
    __shared__ Count s_row_sum;
    __shared__ int s_next;
    Count *s_cnt = s_dyn64;
    int *s_ids = reinterpret_cast<int *>(s_cnt + cap);
    unsigned *s_bits = reinterpret_cast<unsigned *>(s_ids + cap);
    const unsigned lane = util::LaneId();
    const int wave = threadIdx.x / util::kWaveSize;
    const int rows = *d_row_count;
    Count total = 0, ands = 0;  // total: thread 0 only; ands: lane 0 of every wave
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const int u = d_rows[r];
        const int ub = g.ro[u], len = g.ro[u + 1] - ub;
        const int words = (len + 31) / 32;
        if (threadIdx.x == 0) {
            s_row_sum = 0;
            s_next = 0;
        }
        for (int i = threadIdx.x; i < len; i += kBitmapThreads) {
            s_ids[i] = g.ci[ub + i];
            s_cnt[i] = 0;
        }
        for (int i = threadIdx.x; i < len * words; i += kBitmapThreads) s_bits[i] = 0;
        __syncthreads();
        // B: wave per row i, N+(R[i]) streamed, every entry looked up in R
        for (int i = wave; i < len; i += kBitmapWaves) {
            const int v = s_ids[i];
            const int vb = g.ro[v], ve = g.ro[v + 1];
            for (int e = vb + static_cast<int>(lane); e < ve; e += util::kWaveSize) {
                const int x = g.ci[e];
                const int at = LowerBound(s_ids, 0, len, x);
                if (at < len && s_ids[at] == x) atomicOr(&s_bits[i * words + (at >> 5)], 1u << (at & 31));
            }
        }
        __syncthreads();
        // the (K - 1)-cliques of the DAG B: first members handed out one at a time
        Count wave_sum = 0;
        while (true) {
            int i = 0;
            if (lane == 0) i = atomicAdd(&s_next, 1);
            i = __shfl(i, 0, util::kWaveSize);
            if (i >= len) break;
            const unsigned p = lane < static_cast<unsigned>(words) ? s_bits[i * words + lane] : 0u;
            if (!__ballot(p != 0)) continue;
            const Count c = BitDescend<K - 2>(p, s_bits, words, lane, s_cnt, ands);
            if (c && lane == 0) atomicAdd(&s_cnt[i], c);
            wave_sum += c;
        }
        if (lane == 0 && wave_sum) atomicAdd(&s_row_sum, wave_sum);
        __syncthreads();
        for (int i = threadIdx.x; i < len; i += kBitmapThreads) {
            const Count c = s_cnt[i];
            if (c) atomicAdd(d_cliques + s_ids[i], c);
        }
        if (threadIdx.x == 0 && s_row_sum) {
            atomicAdd(d_cliques + u, s_row_sum);
            total += s_row_sum;
        }
        __syncthreads();  // the staged row, the matrix and the two words are reused
    }
    if (threadIdx.x == 0 && total) atomicAdd(d_counters, total);
    if (lane == 0 && ands) atomicAdd(d_counters + 1, ands);
}

// ---------------- the list regime ----------------

// out = the entries of `in` found in row [vb, ve) of the oriented graph, in order; returns their number (in every lane).
// One wave; `out` is read by the whole wave afterwards: the barrier of the one-wave workgroup orders its stores before those loads.
__device__ __forceinline__ int ListIntersect(const int *in, int in_len, const int *ci, int vb, int ve, int *out, unsigned lane, Count &lookups)
{
    int out_len = 0;
    for (int base = 0; base < in_len; base += util::kWaveSize) {
        const int at = base + static_cast<int>(lane);
        bool hit = false;
        int x = 0;
        if (at < in_len) {
            x = in[at];
            const int pos = LowerBound(ci, vb, ve, x);
            hit = pos < ve && ci[pos] == x;
        }
        const unsigned long long mask = __ballot(hit);
        if (hit) out[out_len + static_cast<int>(util::RankInMask(mask))] = x;
        out_len += __popcll(mask);
    }
    lookups += static_cast<Count>(in_len);
    __syncthreads();
    return out_len;
}

// The (REMAIN)-member completions of the candidate list; credits every member it fixes.  `slab`: room for the lists below.
template <int REMAIN>
__device__ __forceinline__ Count ListDescend(const Oriented &g, const int *cand, int len, int *slab, int slab_stride, unsigned lane, Count *d_cliques,
                                             Count &lookups)
{
    if constexpr (REMAIN == 1) {
        for (int i = static_cast<int>(lane); i < len; i += util::kWaveSize) atomicAdd(d_cliques + cand[i], 1ull);
        return static_cast<Count>(len);
    } else {
        Count sum = 0;
        for (int t = 0; t < len; ++t) {
            const int m = cand[t];
            const int next_len = ListIntersect(cand, len, g.ci, g.ro[m], g.ro[m + 1], slab, lane, lookups);
            if (next_len == 0) continue;
            const Count c = ListDescend<REMAIN - 1>(g, slab, next_len, slab + slab_stride, slab_stride, lane, d_cliques, lookups);
            if (c && lane == 0) atomicAdd(d_cliques + m, c);
            sum += c;
            __syncthreads();  // the slab's list is written again
        }
        return sum;
    }
}

// One single-wave workgroup per listed oriented edge; d_slabs: (K - 2) * slab_stride ints per workgroup, slab_stride >= every
// out-row.  d_counters[0] cliques, [2] list look-ups
template <int K>
static __global__ __launch_bounds__(kListThreads) void ListKernel(Oriented g, const int *d_edges, const int *d_edge_count, int *d_slabs, int slab_stride,
                                                                  Count *d_cliques, Count *d_counters)
{
    const unsigned lane = util::LaneId();
    const int edges = *d_edge_count;
    int *slab = d_slabs + static_cast<size_t>(blockIdx.x) * (K - 2) * static_cast<size_t>(slab_stride);
    Count total = 0, lookups = 0;
    for (int i = blockIdx.x; i < edges; i += gridDim.x) {
        const int e = d_edges[i];
        const int u = g.src[e], v = g.ci[e];
        const int ub = g.ro[u];
        const int len = ListIntersect(g.ci + ub, g.ro[u + 1] - ub, g.ci, g.ro[v], g.ro[v + 1], slab, lane, lookups);
        if (len) {
            const Count c = ListDescend<K - 2>(g, slab, len, slab + slab_stride, slab_stride, lane, d_cliques, lookups);
            if (c && lane == 0) {
                atomicAdd(d_cliques + v, c);
                atomicAdd(d_cliques + u, c);
            }
            total += c;
        }
        __syncthreads();
    }
    if (lane == 0) {
        if (total) atomicAdd(d_counters, total);
        if (lookups) atomicAdd(d_counters + 2, lookups);
    }
}

}  // namespace clique
}  // namespace app
}  // namespace gunrock
