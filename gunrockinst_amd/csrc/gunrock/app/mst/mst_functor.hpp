// app/mst/mst_functor.hpp -- device kernels of the Borůvka minimum spanning forest.
//
// Stands for the reference's MST functors (gunrock/app/mst/mst_functor.cuh:33-620: SuccFunctor, EdgeFunctor, MarkFunctor,
// CyRmFunctor, PJmpFunctor, EgRmFunctor, ...), which the reference chains through advance / filter launches with a
// sort-and-renumber contraction in between (mst_enactor.cuh:564-640).  Here a round is five plain kernels over a compacted
// list of the surviving inter-component entries:
//   minimum  best[c] = the smallest key of an entry leaving component c: 64-bit atomic minima, pre-reduced inside the wave,
//            over the CSR rows in round 1 of a mirrored input (RowMinKernel + CanonicalKernel), over the list otherwise (ListMinKernel)
//   hook     every root follows its best entry and marks it selected; a mutual pair keeps the smaller id as root
//            (the reference's S(S(u)) = u rule, mst_enactor.cuh:452-498)
//   flatten  pointer jumping until every vertex points at its root (JumpKernel, as CC's PtrJump)
//   filter   relabel the entries to their roots, drop those inside one component, compact with the device-wide scan
// The key ((uint32)w ^ 0x80000000) << 32 | e orders the entries by (w as signed int32, then CSR index e): a strict total
// order, so the forest is unique and every choice below is deterministic.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace mst {

constexpr unsigned long long kNoEdge = ~0ull;  // (never a real key: e < 2^31)

__device__ __forceinline__ unsigned long long MstKey(int w, long long e)
{
    return (static_cast<unsigned long long>(static_cast<unsigned>(w) ^ 0x80000000u) << 32) | static_cast<unsigned>(e);
}
__device__ __forceinline__ int KeyWeight(unsigned long long k) { return static_cast<int>(static_cast<unsigned>(k >> 32) ^ 0x80000000u); }
__device__ __forceinline__ int KeyEdge(unsigned long long k) { return static_cast<int>(static_cast<unsigned>(k)); }

// position of `wanted` in the sorted row `row`, or -1 (callers only ask when the exact symmetry test has passed: it is there)
__device__ __forceinline__ int RowFind(const int *d_row_offsets, const int *d_cols, int row, int wanted)
{
    int lo = d_row_offsets[row];
    const int end = d_row_offsets[row + 1];
    int hi = end;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (d_cols[mid] < wanted) lo = mid + 1; else hi = mid;
    }
    return lo < end && d_cols[lo] == wanted ? lo : -1;
}

// d_bad = 1 when an entry (f, t), f < t, has a mirror of a different weight (exact symmetry already holds: the mirror exists)
static __global__ void MirrorWeightKernel(const int *d_row_offsets, const int *d_cols, const int *d_weights, const int *d_froms,
                                          long long edges, int *d_bad)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    bool bad = false;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        const int f = d_froms[e], t = d_cols[e];
        if (f >= t) continue;
        const int mirror = RowFind(d_row_offsets, d_cols, t, f);
        bad |= mirror < 0 || d_weights[mirror] != d_weights[e];
    }
    if (__ballot(bad) && util::LaneId() == 0) *d_bad = 1;
}

// atomicMin(best[target], key) for every lane, one atomic per run of equal targets: a segmented minimum towards the run's
// first lane (a lane combines with the lane `off` above it only when both name the same target, so what it holds is always
// a minimum over lanes of its own target, and a run's first lane ends up with the whole run).  A plain read skips the atomic
// when the slot already holds a smaller key (slots only decrease; a stale read only costs the atomic).
__device__ __forceinline__ void SegmentedAtomicMin(unsigned long long *d_best, int target, unsigned long long key)
{
    const int lane = static_cast<int>(util::LaneId());
#pragma unroll
    for (int off = 1; off < util::kWaveSize; off <<= 1) {
        const unsigned long long k = __shfl_down(key, off, util::kWaveSize);
        const int t = __shfl_down(target, off, util::kWaveSize);
        if (lane + off < util::kWaveSize && t == target && k < key) key = k;
    }
    const int prev = __shfl_up(target, 1, util::kWaveSize);
    if (target >= 0 && (lane == 0 || prev != target) && d_best[target] > key) atomicMin(d_best + target, key);
}

// ---- round 1 of a mirrored input with equal mirror weights: best[v] = the smallest key over row v ----
// Only the f < t copy of an edge is a candidate (it lies in the earlier row, so it always has the smaller key).  Row v is
// sorted by column, so among the entries of one weight the column order IS the order of their canonical copies (those to
// u < v lie in row u, before row v, in increasing u; those to u > v are row v's own, in increasing u): the row minimum picks
// the right neighbour, and only the winner is translated to its canonical index, by one binary search in row u
// (CanonicalKernel).  The minimum itself is entry-parallel (RowMinKernel): a lane per entry, one pre-reduced atomic per run of
// one row inside a wave.  Measured at scale-22: a lane per short row and a wave per long row took 10.5 ms, because R-MAT puts
// its hubs at the low ids and a few waves walked most of the entries alone.
static __global__ void RowMinKernel(const int *d_froms, const int *d_cols, const int *d_weights, long long edges, unsigned long long *d_best)
{
    const unsigned lane = util::LaneId();
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    for (long long base = wave0 * util::kWaveSize; base < edges; base += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = base + lane;
        int target = -1;
        unsigned long long key = kNoEdge;
        if (i < edges) {
            const int f = d_froms[i];
            if (d_cols[i] != f) {
                target = f;
                key = MstKey(d_weights[i], i);
            }
        }
        SegmentedAtomicMin(d_best, target, key);
    }
}
static __global__ void CanonicalKernel(const int *d_row_offsets, const int *d_cols, long long nodes, unsigned long long *d_best)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const unsigned long long best = d_best[v];
        if (best == kNoEdge) continue;
        const int u = d_cols[KeyEdge(best)];
        const int mirror = u < static_cast<int>(v) ? RowFind(d_row_offsets, d_cols, u, static_cast<int>(v)) : -1;
        if (mirror >= 0) d_best[v] = (best & 0xFFFFFFFF00000000ull) | static_cast<unsigned>(mirror);
    }
}

// rounds >= 2 (and round 1 of any other input): best[cu] and best[cv] over the list of inter-component entries
static __global__ void ListMinKernel(const int *d_cu, const int *d_cv, const unsigned long long *d_key, long long len,
                                     unsigned long long *d_best)
{
    const unsigned lane = util::LaneId();
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / util::kWaveSize;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / util::kWaveSize;
    for (long long base = wave0 * util::kWaveSize; base < len; base += nwaves * util::kWaveSize) {  // (wave-uniform)
        const long long i = base + lane;
        int cu = -1, cv = -1;
        unsigned long long key = kNoEdge;
        if (i < len) { cu = d_cu[i]; cv = d_cv[i]; key = d_key[i]; }
        SegmentedAtomicMin(d_best, cu, key);
        SegmentedAtomicMin(d_best, cv, key);
    }
}

// Every root v with an outgoing entry follows it: parent_out[v] = the root at its other end, selected[e] = 1.  In a mutual
// pair (both roots chose the same entry -- under a strict order the only cycle there is) the smaller id stays root.  Reads
// only parent_in (flattened: every vertex points at its root), so no hook is seen by another in the same launch.  Every
// hooking root adds one forest edge: d_totals = {forest weight, forest edges}, summed in registers and LDS and added with one
// pair of atomics per workgroup (one pair per wave and loop step was 130 k same-address atomics at scale-22: ~10 ms).
constexpr int kHookThreads = 256;
static __global__ __launch_bounds__(kHookThreads) void HookKernel(const int *d_parent_in, int *d_parent_out, const unsigned long long *d_best,
                                                                  const int *d_froms, const int *d_cols, long long nodes, int *d_selected,
                                                                  unsigned long long *d_totals)
{
    __shared__ long long s_sum[2][kHookThreads / util::kWaveSize];
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    long long weight = 0, hooked = 0;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int p = d_parent_in[v];
        int out = p;
        if (p == static_cast<int>(v)) {
            const unsigned long long k = d_best[v];
            if (k != kNoEdge) {
                const int e = KeyEdge(k);
                const int a = d_parent_in[d_froms[e]], b = d_parent_in[d_cols[e]];
                const int o = a == static_cast<int>(v) ? b : a;
                if (!(d_best[o] == k && static_cast<int>(v) < o)) {
                    out = o;
                    weight += KeyWeight(k);
                    hooked += 1;
                }
                d_selected[e] = 1;
            }
        }
        d_parent_out[v] = out;
    }
    for (int o = util::kWaveSize / 2; o > 0; o >>= 1) {
        weight += __shfl_xor(weight, o, util::kWaveSize);
        hooked += __shfl_xor(hooked, o, util::kWaveSize);
    }
    const int wave = threadIdx.x / util::kWaveSize;
    if (util::LaneId() == 0) { s_sum[0][wave] = weight; s_sum[1][wave] = hooked; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kHookThreads / util::kWaveSize; ++w) { weight += s_sum[0][w]; hooked += s_sum[1][w]; }
        if (hooked) {
            atomicAdd(d_totals, static_cast<unsigned long long>(weight));  // (two's complement: negative weights wrap correctly)
            atomicAdd(d_totals + 1, static_cast<unsigned long long>(hooked));
        }
    }
}

// pointer jumping, up to kJumpHops parents per sweep (every value read on the way is an ancestor: same fixed point as one hop);
// d_changed = 1 when a sweep moved a pointer
constexpr int kJumpHops = 8;
static __global__ void JumpKernel(int *d_parent, long long nodes, int *d_changed)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    bool changed = false;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int p = d_parent[v];
        int r = p;
#pragma unroll 1
        for (int hop = 0; hop < kJumpHops; ++hop) {
            const int up = d_parent[r];
            if (up == r) break;
            r = up;
        }
        if (r != p) {
            d_parent[v] = r;
            changed = true;
        }
    }
    if (__ballot(changed) && util::LaneId() == 0) *d_changed = 1;
}

// ---- filter: keep[i] = the entry joins two different components (relabelled to their roots); flags[len] = 0 closes the scan ----
// From the CSR (the first list): an entry is a candidate unless it is a self-loop or -- mirrored input with equal weights --
// the later copy (f > t) of its edge.
static __global__ void FlagCsrKernel(const int *d_froms, const int *d_cols, const int *d_parent, long long edges, int lower_only,
                                     unsigned *d_flags)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i <= edges; i += stride) {
        unsigned keep = 0;
        if (i < edges) {
            const int f = d_froms[i], t = d_cols[i];
            keep = f != t && (!lower_only || f < t) && d_parent[f] != d_parent[t];
        }
        d_flags[i] = keep;
    }
}
static __global__ void ScatterCsrKernel(const int *d_froms, const int *d_cols, const int *d_weights, const int *d_parent,
                                        const unsigned *d_flags, const unsigned *d_pos, long long edges, int *d_cu, int *d_cv,
                                        unsigned long long *d_key)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < edges; i += stride) {
        if (!d_flags[i]) continue;
        const unsigned at = d_pos[i];
        d_cu[at] = d_parent[d_froms[i]];
        d_cv[at] = d_parent[d_cols[i]];
        d_key[at] = MstKey(d_weights[i], i);
    }
}
// From the previous list: relabel in place, flag the entries that still cross components
static __global__ void FlagListKernel(int *d_cu, int *d_cv, const int *d_parent, long long len, unsigned *d_flags)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i <= len; i += stride) {
        unsigned keep = 0;
        if (i < len) {
            const int cu = d_parent[d_cu[i]], cv = d_parent[d_cv[i]];
            keep = cu != cv;
            if (keep) { d_cu[i] = cu; d_cv[i] = cv; }
        }
        d_flags[i] = keep;
    }
}
static __global__ void ScatterListKernel(const int *d_cu, const int *d_cv, const unsigned long long *d_key, const unsigned *d_flags,
                                         const unsigned *d_pos, long long len, int *d_out_cu, int *d_out_cv, unsigned long long *d_out_key)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < len; i += stride) {
        if (!d_flags[i]) continue;
        const unsigned at = d_pos[i];
        d_out_cu[at] = d_cu[i];
        d_out_cv[at] = d_cv[i];
        d_out_key[at] = d_key[i];
    }
}

}  // namespace mst
}  // namespace app
}  // namespace gunrock
