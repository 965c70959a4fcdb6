// app/tc/tc_functor.hpp -- kernels of triangle counting: the build of the oriented graph and the sorted-set intersections.
//
// The reference snapshot has no app/tc (later Gunrock releases do); the shape follows this tree's primitives.
// The oriented CSR (tc_problem.hpp) holds every edge of the simple undirected graph once, from the endpoint with the smaller
// (d, id) to the larger, rows ascending by id.  A triangle {a, b, c} ordered by (d, id) appears exactly once as the oriented edge
// (a, b) plus the common out-neighbour c.  The work item is an oriented edge (u, v), the work |N+(u) ^ N+(v)|, and a hit w
// credits u, v and w.  Three regimes, picked per row u by its length (tc_enactor.hpp bins):
//   lane    one lane per oriented edge; the shorter row is looked up in the longer one (monotone binary search), or the two are
//           merged when their lengths are close.  w: one global atomic per hit; v: one per edge; u: a segmented wave reduction over
//           the lanes that share u, one atomic per segment.
//   LDS     one workgroup per row u: N+(u) is staged in LDS with one counter per entry; wave j streams N+(v_j) with coalesced loads,
//           each lane looks its entry up in the staged row.  w's credit is an LDS atomic on w's counter, v's credit (v is entry j
//           of the same row) one LDS atomic per edge after a wave reduction; the counters are flushed with one global atomic per
//           non-zero entry, u's credit with one per row.
//   global  the same walk for a row that does not fit the staging budget: the look-ups go to N+(u) in global memory (L2),
//           w's credit is a global atomic per hit, v's one per edge, u's one per row.
// The total is reduced per workgroup.  Integer adds commute: every regime writes the same arrays.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace tc {

typedef unsigned long long Count;

enum { TC_AUTO = 0, TC_LANE = 1, TC_LDS = 2, TC_GLOBAL = 3 };

constexpr int kTcThreads = 256;
constexpr int kTcWaves = kTcThreads / util::kWaveSize;
constexpr int kLaneMaxRow = 32;       // automatic: rows up to this length go to the lane regime
constexpr int kLdsEntries = 4096;     // default staging budget, entries (8 bytes each: the id and its counter)
constexpr int kLdsEntriesMax = 8192;  // 64 KiB of dynamic LDS

struct Oriented {
    const int *ro;   // [nodes + 1]
    const int *ci;   // [M] ascending inside a row
    const int *src;  // [M] the row of every entry
};

// ---------------- the build (the keys, their sort and the keep flags are graphio/pair_graph.hpp's) ----------------

// d_deg[v] += the kept keys with an end at v
static __global__ void DegreeKernel(const unsigned long long *d_keys, const unsigned *d_keep, long long count, int col_bits, unsigned *d_deg)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (!d_keep[i]) continue;
        const unsigned long long k = d_keys[i];
        atomicAdd(d_deg + static_cast<unsigned>(k >> col_bits), 1u);
        atomicAdd(d_deg + static_cast<unsigned>(k & mask), 1u);
    }
}

// every kept edge points from the endpoint with the smaller (d, id); its key (src << col_bits) | dst lands at its rank
static __global__ void OrientKernel(const unsigned long long *d_keys, const unsigned *d_keep, const unsigned long long *d_pos, long long count,
                                    int col_bits, const unsigned *d_deg, unsigned long long *d_okeys, unsigned *d_outdeg)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (!d_keep[i]) continue;
        const unsigned long long k = d_keys[i];
        const unsigned a = static_cast<unsigned>(k >> col_bits), b = static_cast<unsigned>(k & mask);  // a < b
        const bool a_first = d_deg[a] <= d_deg[b];  // equal degrees: the smaller id, a
        const unsigned s = a_first ? a : b, t = a_first ? b : a;
        d_okeys[d_pos[i]] = (static_cast<unsigned long long>(s) << col_bits) | t;
        atomicAdd(d_outdeg + s, 1u);
    }
}

static __global__ void EmitOrientedKernel(const unsigned long long *d_okeys, long long count, int col_bits, int *d_oci, int *d_osrc)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        const unsigned long long k = d_okeys[i];
        d_oci[i] = static_cast<int>(k & mask);
        d_osrc[i] = static_cast<int>(k >> col_bits);
    }
}

// d_out[0] = sum over v of C(d(v), 2) (64-bit), d_out[1] = the largest out-row
static __global__ void RowSummaryKernel(const unsigned *d_deg, const int *d_oro, long long nodes, Count *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    Count wedges = 0, most = 0;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const Count d = d_deg[v];
        wedges += d * (d > 0 ? d - 1 : 0) / 2;
        const Count len = static_cast<Count>(d_oro[v + 1] - d_oro[v]);
        most = len > most ? len : most;
    }
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        wedges += __shfl_xor(wedges, o, util::kWaveSize);
        const Count other = __shfl_xor(most, o, util::kWaveSize);
        most = other > most ? other : most;
    }
    if (util::LaneId() == 0) {
        if (wedges) atomicAdd(d_out, wedges);
        atomicMax(d_out + 1, most);
    }
}

// coeff[v] = 2 t / (d (d - 1)) as one double division of two exact integers; 0 where d < 2
static __global__ void ClusteringKernel(const Count *d_tri, const unsigned *d_deg, long long nodes, double *d_coeff)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const Count d = d_deg[v];
        d_coeff[v] = d < 2 ? 0.0 : static_cast<double>(2 * d_tri[v]) / static_cast<double>(d * (d - 1));
    }
}

// ---------------- binning ----------------

__host__ __device__ __forceinline__ int RegimeOf(int len, int strategy, int lane_max, int lds_entries)
{
    if (strategy == TC_LANE) return TC_LANE;
    if (strategy == TC_GLOBAL) return TC_GLOBAL;
    if (strategy == TC_AUTO && len <= lane_max) return TC_LANE;
    return len <= lds_entries ? TC_LDS : TC_GLOBAL;  // (a forced LDS regime still cannot stage a row beyond the budget)
}

// d_words[0], [1]: lengths of the LDS and the global row lists; [2]: rows left to the lane regime.  Empty rows are nobody's.
static __global__ void BinKernel(const int *d_oro, int nodes, int strategy, int lane_max, int lds_entries, int *d_lds_rows, int *d_global_rows,
                                 int *d_words)
{
    const int stride = gridDim.x * blockDim.x;
    int lanes = 0;
    for (long long u = blockIdx.x * blockDim.x + threadIdx.x; u < nodes; u += stride) {
        const int len = d_oro[u + 1] - d_oro[u];
        if (len == 0) continue;
        const int regime = RegimeOf(len, strategy, lane_max, lds_entries);
        if (regime == TC_LANE) ++lanes;
        else if (regime == TC_LDS) d_lds_rows[atomicAdd(d_words, 1)] = static_cast<int>(u);
        else d_global_rows[atomicAdd(d_words + 1, 1)] = static_cast<int>(u);
    }
    lanes = util::WaveSum(lanes);
    if (util::LaneId() == 0 && lanes) atomicAdd(d_words + 2, lanes);
}

// ---------------- the intersections ----------------

// first index in [lo, hi) of p with p[i] >= x
template <typename Ptr>
__device__ __forceinline__ int LowerBound(Ptr p, int lo, int hi, int x)
{
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (p[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// d_counters[0] triangles, [1] row entries streamed through a look-up or a merge step
static __global__ __launch_bounds__(kTcThreads) void LaneKernel(Oriented g, long long oriented_edges, int lane_max, Count *d_tri, Count *d_counters)
{
    __shared__ Count s_sum[2];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const unsigned lane = util::LaneId();
    const long long stride = static_cast<long long>(gridDim.x) * kTcThreads;
    Count total = 0, probed = 0;
    for (long long base = static_cast<long long>(blockIdx.x) * kTcThreads; base < oriented_edges; base += stride) {  // (uniform: the shuffles below)
        const long long e = base + threadIdx.x;
        int u = -1;
        unsigned c = 0;
        if (e < oriented_edges) {
            u = g.src[e];
            int ab = g.ro[u], ae = g.ro[u + 1];
            if (ae - ab <= lane_max) {
                const int v = g.ci[e];
                int bb = g.ro[v], be = g.ro[v + 1];
                if (ae - ab > be - bb) {  // A = the shorter row
                    int t = ab; ab = bb; bb = t;
                    t = ae; ae = be; be = t;
                }
                const int la = ae - ab, lb = be - bb;
                if (la > 0) {
                    const int steps = 32 - __clz(lb);  // of a bisection of B
                    if (la + lb <= la * steps) {       // merge
                        int i = ab, j = bb;
                        int x = g.ci[i], y = g.ci[j];
                        while (true) {
                            if (x == y) {
                                ++c;
                                atomicAdd(d_tri + x, 1ull);
                            }
                            const bool step_i = x <= y, step_j = y <= x;
                            if (step_i) { if (++i == ae) break; x = g.ci[i]; }
                            if (step_j) { if (++j == be) break; y = g.ci[j]; }
                        }
                        probed += static_cast<Count>((i - ab) + (j - bb));
                    } else {                           // look every entry of A up in B, from where the last one ended
                        int lo = bb;
                        for (int i = ab; i < ae && lo < be; ++i) {
                            const int x = g.ci[i];
                            lo = LowerBound(g.ci, lo, be, x);
                            if (lo < be && g.ci[lo] == x) {
                                ++c;
                                atomicAdd(d_tri + x, 1ull);
                                ++lo;
                            }
                        }
                        probed += static_cast<Count>(la);
                    }
                    if (c) atomicAdd(d_tri + v, static_cast<Count>(c));
                }
            }
        }
        // u's credit: the lanes of one u are neighbours (entries are in row order): segmented inclusive sum, its last lane adds
        unsigned s = c;
#pragma unroll
        for (int o = 1; o < util::kWaveSize; o <<= 1) {
            const unsigned t = __shfl_up(s, o, util::kWaveSize);
            const int tu = __shfl_up(u, o, util::kWaveSize);
            if (lane >= static_cast<unsigned>(o) && tu == u) s += t;
        }
        const int next_u = __shfl_down(u, 1, util::kWaveSize);
        if ((lane == util::kWaveSize - 1 || next_u != u) && s) atomicAdd(d_tri + u, static_cast<Count>(s));
        total += c;
    }
    total = util::WaveSum(total);
    probed = util::WaveSum(probed);
    if (lane == 0) {
        if (total) atomicAdd(&s_sum[0], total);
        if (probed) atomicAdd(&s_sum[1], probed);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_sum[threadIdx.x]) atomicAdd(d_counters + threadIdx.x, s_sum[threadIdx.x]);
}

// One workgroup per listed row.  STAGED: dynamic LDS holds lds_entries ids and lds_entries counters (every listed row fits).
template <bool STAGED>
static __global__ __launch_bounds__(kTcThreads) void RowKernel(Oriented g, const int *d_rows, const int *d_row_count, int lds_entries, Count *d_tri,
                                                               Count *d_counters)
{
    extern __shared__ int s_dyn[];
    __shared__ unsigned s_row_hits;
    int *s_ids = s_dyn;
    unsigned *s_cnt = reinterpret_cast<unsigned *>(s_dyn + lds_entries);
    const unsigned lane = util::LaneId();
    const int wave = threadIdx.x / util::kWaveSize;
    const int rows = *d_row_count;
    Count total = 0, probed = 0;  // total: thread 0 only; probed: lane 0 of every wave
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const int u = d_rows[r];
        const int ub = g.ro[u], len = g.ro[u + 1] - ub;
        if (threadIdx.x == 0) s_row_hits = 0;
        if (STAGED)
            for (int i = threadIdx.x; i < len; i += kTcThreads) {
                s_ids[i] = g.ci[ub + i];
                s_cnt[i] = 0;
            }
        __syncthreads();
        unsigned wave_hits = 0;
        for (int j = wave; j < len; j += kTcWaves) {
            const int v = STAGED ? s_ids[j] : g.ci[ub + j];
            const int vb = g.ro[v], ve = g.ro[v + 1];
            unsigned c = 0;
            for (int k = vb + static_cast<int>(lane); k < ve; k += util::kWaveSize) {
                const int x = g.ci[k];
                if (STAGED) {
                    const int at = LowerBound(s_ids, 0, len, x);
                    if (at < len && s_ids[at] == x) {
                        ++c;
                        atomicAdd(&s_cnt[at], 1u);
                    }
                } else {
                    const int at = LowerBound(g.ci, ub, ub + len, x);
                    if (at < ub + len && g.ci[at] == x) {
                        ++c;
                        atomicAdd(d_tri + x, 1ull);
                    }
                }
            }
            c = util::WaveSum(c);
            if (lane == 0) {
                probed += static_cast<Count>(ve - vb);
                if (c) {
                    if (STAGED) atomicAdd(&s_cnt[j], c);
                    else atomicAdd(d_tri + v, static_cast<Count>(c));
                }
            }
            wave_hits += c;
        }
        if (lane == 0 && wave_hits) atomicAdd(&s_row_hits, wave_hits);
        __syncthreads();
        if (STAGED)
            for (int i = threadIdx.x; i < len; i += kTcThreads) {
                const unsigned c = s_cnt[i];
                if (c) atomicAdd(d_tri + s_ids[i], static_cast<Count>(c));
            }
        if (threadIdx.x == 0 && s_row_hits) {
            atomicAdd(d_tri + u, static_cast<Count>(s_row_hits));
            total += s_row_hits;
        }
        __syncthreads();  // the staged row and s_row_hits are reused
    }
    if (threadIdx.x == 0 && total) atomicAdd(d_counters, total);
    if (lane == 0 && probed) atomicAdd(d_counters + 1, probed);
}

}  // namespace tc
}  // namespace app
}  // namespace gunrock
