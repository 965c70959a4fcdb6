// graphio/pair_graph.hpp -- the simple undirected graph of a CSR, built on the device, and the check that a CSR is one.
//
// Every primitive that reads its input as the simple undirected graph G (u and v are neighbours when either row holds the other;
// self-loops ignored; unsorted rows, duplicates and one-way entries allowed) builds the same thing with the radix sort and the scan
// of device_sort.hpp / device_csr.hpp.  PairGraph is that build, in steps a caller can stop between:
//   Keys      one key (min << cb | max) per CSR entry, self-loops as the sentinel; sorted; duplicates flagged off: d_sorted, d_keep.
//             (Reserve + SortKeys are its halves, for a caller that writes keys of its own into sort.Keys().)
//   CountKept the flags scanned into d_pos; the number of kept keys, read from behind the scan's tile offsets (the one read-back)
//   Pairs     CountKept, then the kept keys compacted: the M canonical pairs src[e] < dst[e] in (src, dst) order, and their keys
//             d_ckeys, which stay until the object goes
//   Rows      the same pairs keyed (max << cb | min) and sorted: the lower parts of the rows; both key arrays bisected per vertex give
//             d(v) and, scanned, the offsets ro[]; row v = its lower neighbours, then its upper ones: ci[] ascending by id, eid[] the
//             pair of every entry, 2M entries
// The object owns everything it allocates and frees it when it goes, so every early return of a caller is clean; what a caller
// keeps it takes over with Take().  DeviceScratch is the same for one array of a caller's own, BuildEvents for the HIP events a
// build times itself with.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/graphio/device_sort.hpp>
#include <gunrock/util/device_array.hpp>

namespace gunrock {
namespace graphio {

inline int PairGrid(long long work)
{
    long long blocks = (work + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;  // 256 CUs x 8 workgroups, grid-stride the rest
    return static_cast<int>(blocks);
}

// d_bad = 1 unless row_offsets[0] = 0, row_offsets[nodes] = edges, the offsets never decrease and every column is a vertex
static __global__ void ValidateCsrKernel(const int *d_row_offsets, const int *d_cols, long long nodes, long long edges, int *d_bad)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long count = nodes > edges ? nodes : edges;
    bool bad = false;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i <= count; i += stride) {
        if (i < nodes) bad |= d_row_offsets[i] > d_row_offsets[i + 1];
        if (i == 0) bad |= d_row_offsets[0] != 0 || d_row_offsets[nodes] != edges;
        if (i < edges) {
            const int t = d_cols[i];
            bad |= t < 0 || t >= nodes;
        }
    }
    if (__ballot(bad) && util::LaneId() == 0) *d_bad = 1;
}

// one key per CSR entry: (min << col_bits) | max, or the sentinel for a self-loop.  The row of entry e is found by bisection of the
// offsets (validated: non-decreasing, from 0 to edges).
static __global__ void EdgeKeysKernel(const int *d_row_offsets, const int *d_cols, int nodes, long long edges, int col_bits,
                                      unsigned long long sentinel, unsigned long long *d_keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        int lo = 0, hi = nodes;  // first index in [0, nodes] whose offset exceeds e (offsets[nodes] = edges > e)
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (d_row_offsets[mid] > e) hi = mid; else lo = mid + 1;
        }
        const unsigned r = static_cast<unsigned>(lo - 1), c = static_cast<unsigned>(d_cols[e]);
        const unsigned a = r < c ? r : c, b = r < c ? c : r;
        d_keys[e] = (a == b) ? sentinel : ((static_cast<unsigned long long>(a) << col_bits) | b);
    }
}

// the kept keys (a << cb | b) in order: the canonical edges
static __global__ void CanonicalKernel(const unsigned long long *d_keys, const unsigned *d_keep, const unsigned long long *d_pos, long long count,
                                       int col_bits, unsigned long long *d_ckeys, int *d_src, int *d_dst)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (!d_keep[i]) continue;
        const unsigned long long key = d_keys[i], at = d_pos[i];
        d_ckeys[at] = key;
        d_src[at] = static_cast<int>(key >> col_bits);
        d_dst[at] = static_cast<int>(key & mask);
    }
}

// the same edges keyed (b << cb | a): sorted, they are the lower parts of the rows
static __global__ void SwapKeysKernel(const unsigned long long *d_ckeys, long long edges, int col_bits, unsigned long long *d_out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; e < edges; e += stride) {
        const unsigned long long key = d_ckeys[e];
        d_out[e] = ((key & mask) << col_bits) | (key >> col_bits);
    }
}

// first index in [0, n) of keys with keys[i] >= x
__device__ __forceinline__ long long KeyLowerBound(const unsigned long long *keys, long long n, unsigned long long x)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// for v = 0 .. nodes: up[v] = the edges (a, .) with a < v, low[v] = the edges (., b) with b < v; d(v) for v < nodes (deg[nodes] = 0)
static __global__ void RowStartsKernel(const unsigned long long *d_ckeys, const unsigned long long *d_skeys, long long edges, long long nodes,
                                       int col_bits, int *d_up, int *d_low)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v <= nodes; v += stride) {
        const unsigned long long x = static_cast<unsigned long long>(v) << col_bits;
        d_up[v] = static_cast<int>(KeyLowerBound(d_ckeys, edges, x));
        d_low[v] = static_cast<int>(KeyLowerBound(d_skeys, edges, x));
    }
}

static __global__ void DegreesKernel(const int *d_up, const int *d_low, long long nodes, unsigned *d_deg)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v <= nodes; v += stride)
        d_deg[v] = v < nodes ? static_cast<unsigned>((d_up[v + 1] - d_up[v]) + (d_low[v + 1] - d_low[v])) : 0u;
}

// row v = its lower neighbours ascending (the edges (., v) in the order of the swapped keys), then its upper ones (the edges
// (v, .) in canonical order): ascending by id without a sort of the rows
static __global__ void FillRowsKernel(const unsigned long long *d_ckeys, const unsigned long long *d_skeys, long long edges, int col_bits,
                                      const int *d_up, const int *d_low, const int *d_ro, int *d_ci, int *d_eid)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << col_bits) - 1ull;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < edges; i += stride) {
        {
            const unsigned long long key = d_ckeys[i];
            const int a = static_cast<int>(key >> col_bits), b = static_cast<int>(key & mask);
            const long long at = static_cast<long long>(d_ro[a]) + (d_low[a + 1] - d_low[a]) + (i - d_up[a]);
            d_ci[at] = b;
            d_eid[at] = static_cast<int>(i);
        }
        {
            const unsigned long long key = d_skeys[i];
            const int b = static_cast<int>(key >> col_bits), a = static_cast<int>(key & mask);
            const long long at = static_cast<long long>(d_ro[b]) + (i - d_low[b]);
            d_ci[at] = a;
            d_eid[at] = static_cast<int>(KeyLowerBound(d_ckeys, edges, (static_cast<unsigned long long>(a) << col_bits) | static_cast<unsigned>(b)));
        }
    }
}

// Is it a CSR of `nodes` vertices and `edges` entries?  d_flag: one device word of the caller's; one read-back.
inline hipError_t DeviceValidateCsr(const int *d_row_offsets, const int *d_cols, long long nodes, long long edges, int *d_flag, hipStream_t stream,
                                    bool *bad)
{
    hipError_t retval = hipSuccess;
    int flag = 0;
    GR_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), stream), "DeviceValidateCsr memset failed");
    hipLaunchKernelGGL(ValidateCsrKernel, dim3(PairGrid((nodes > edges ? nodes : edges) + 1)), dim3(256), 0, stream, d_row_offsets, d_cols, nodes,
                       edges, d_flag);
    GR_CHECK(hipGetLastError(), "ValidateCsrKernel launch failed");
    GR_CHECK(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, stream), "DeviceValidateCsr read-back failed");
    GR_CHECK(hipStreamSynchronize(stream), "DeviceValidateCsr read-back sync failed");
    *bad = flag != 0;
    return retval;
}

// the caller takes the array over: the owner it came from forgets it
template <typename T>
inline T *Take(T *&p)
{
    T *taken = p;
    p = nullptr;
    return taken;
}

// one device array that goes with its scope
template <typename T>
using DeviceScratch = util::DeviceArray<T>;

// the HIP events of a build that times itself: destroyed on every path out
struct BuildEvents {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    BuildEvents() = default;
    BuildEvents(const BuildEvents &) = delete;
    BuildEvents &operator=(const BuildEvents &) = delete;
    ~BuildEvents()
    {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
    hipError_t Create(int count)
    {
        hipError_t retval = hipSuccess;
        for (int i = 0; i < count; ++i) GR_CHECK(hipEventCreate(&ev[i]), "BuildEvents hipEventCreate failed");
        return retval;
    }
    hipError_t Record(int i, hipStream_t stream) { return util::GRError(hipEventRecord(ev[i], stream), "BuildEvents hipEventRecord failed", __FILE__, __LINE__); }
    // (both events have been reached: the caller has synchronised)
    hipError_t Elapsed(int from, int to, double *ms)
    {
        hipError_t retval = hipSuccess;
        float t = 0;
        GR_CHECK(hipEventElapsedTime(&t, ev[from], ev[to]), "BuildEvents hipEventElapsedTime failed");
        *ms = t;
        return retval;
    }
};

struct PairGraph {
    long long nodes = 0;
    long long count = 0;  // keys
    long long pairs = 0;  // M, after Pairs
    int col_bits = 1, key_bits = 2;  // key_bits <= 62
    unsigned long long sentinel = 3;  // min = max = 2^cb - 1: never a pair
    DeviceKeySort sort;
    unsigned long long *d_sorted = nullptr;  // the sorted keys (one of sort's buffers, until Rows sorts again)
    // scratch
    unsigned *d_keep = nullptr, *d_deg = nullptr;
    unsigned long long *d_pos = nullptr, *d_sums = nullptr, *d_ckeys = nullptr;
    int *d_up = nullptr, *d_low = nullptr;
    // the result, until taken
    int *d_src = nullptr, *d_dst = nullptr, *d_ro = nullptr, *d_ci = nullptr, *d_eid = nullptr;

    explicit PairGraph(long long nodes_) : nodes(nodes_)
    {
        while ((1ll << col_bits) < nodes) ++col_bits;
        key_bits = 2 * col_bits;
        sentinel = (1ull << key_bits) - 1ull;
    }
    PairGraph(const PairGraph &) = delete;
    PairGraph &operator=(const PairGraph &) = delete;
    ~PairGraph()
    {
        void *bufs[] = {d_keep, d_deg, d_pos, d_sums, d_ckeys, d_up, d_low, d_src, d_dst, d_ro, d_ci, d_eid};
        for (void *b : bufs)
            if (b) util::GRError(hipFree(b), "PairGraph hipFree failed", __FILE__, __LINE__);
    }

    // room for count_ > 0 keys, once; the caller writes them to sort.Keys()
    hipError_t Reserve(long long count_)
    {
        hipError_t retval = hipSuccess;
        count = count_;
        GR_CHECK(hipMalloc(&d_keep, sizeof(unsigned) * static_cast<size_t>(count)), "PairGraph hipMalloc failed");
        GR_CHECK(sort.Reserve(count), "PairGraph sort scratch failed");
        return retval;
    }

    hipError_t SortKeys(hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(sort.Sort(count, key_bits, stream, &d_sorted), "PairGraph key sort failed");
        hipLaunchKernelGGL(FlagKernel, dim3(PairGrid(count)), dim3(256), 0, stream, d_sorted, count, sentinel, d_keep);
        GR_CHECK(hipGetLastError(), "FlagKernel launch failed");
        return retval;
    }

    // (a validated CSR; without an entry there is nothing to do, here and in the steps behind)
    hipError_t Keys(const int *d_row_offsets, const int *d_cols, long long edges, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        if (edges < 1) return retval;
        if ((retval = Reserve(edges))) return retval;
        hipLaunchKernelGGL(EdgeKeysKernel, dim3(PairGrid(edges)), dim3(256), 0, stream, d_row_offsets, d_cols, static_cast<int>(nodes), edges,
                           col_bits, sentinel, sort.Keys());
        GR_CHECK(hipGetLastError(), "EdgeKeysKernel launch failed");
        return SortKeys(stream);
    }

    // d_sums has room for a scan of the keys and for one of nodes + 1 words
    hipError_t CountKept(hipStream_t stream, long long *kept)
    {
        hipError_t retval = hipSuccess;
        *kept = 0;
        if (count < 1) return retval;
        const long long scan_words = count > nodes + 1 ? count : nodes + 1;
        GR_CHECK(hipMalloc(&d_pos, sizeof(unsigned long long) * static_cast<size_t>(count)), "PairGraph hipMalloc failed");
        GR_CHECK(hipMalloc(&d_sums, sizeof(unsigned long long) * static_cast<size_t>(ScanScratchWords(scan_words))), "PairGraph hipMalloc failed");
        GR_CHECK(DeviceExclusiveScan<unsigned long long>(d_keep, d_pos, count, d_sums, stream), "PairGraph flag scan failed");
        unsigned long long total = 0;  // ScanSumsKernel leaves it behind the tile offsets
        const long long scan_tiles = (count + kScanTile - 1) / kScanTile;
        GR_CHECK(hipMemcpyAsync(&total, d_sums + scan_tiles, sizeof(total), hipMemcpyDeviceToHost, stream), "PairGraph read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "PairGraph read-back sync failed");
        *kept = static_cast<long long>(total);
        return retval;
    }

    // hipErrorInvalidValue when 2M is no int: every offset of the 2M entries is one
    hipError_t Pairs(hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        long long kept = 0;
        if ((retval = CountKept(stream, &kept))) return retval;
        if (2 * kept > 0x7FFFFFFFll) return hipErrorInvalidValue;
        pairs = kept;
        if (pairs < 1) return retval;
        const size_t ms = static_cast<size_t>(pairs);
        GR_CHECK(hipMalloc(&d_ckeys, sizeof(unsigned long long) * ms), "PairGraph hipMalloc failed");
        GR_CHECK(hipMalloc(&d_src, sizeof(int) * ms), "PairGraph hipMalloc d_src failed");
        GR_CHECK(hipMalloc(&d_dst, sizeof(int) * ms), "PairGraph hipMalloc d_dst failed");
        hipLaunchKernelGGL(CanonicalKernel, dim3(PairGrid(count)), dim3(256), 0, stream, d_sorted, d_keep, d_pos, count, col_bits, d_ckeys, d_src,
                           d_dst);
        GR_CHECK(hipGetLastError(), "CanonicalKernel launch failed");
        return retval;
    }

    // ro[] is there (all 0) without a pair too; ci[] and eid[] only with one
    hipError_t Rows(hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        const size_t n1 = static_cast<size_t>(nodes > 0 ? nodes : 1), ms = static_cast<size_t>(pairs);
        GR_CHECK(hipMalloc(&d_ro, sizeof(int) * (n1 + 1)), "PairGraph hipMalloc d_ro failed");
        GR_CHECK(hipMemsetAsync(d_ro, 0, sizeof(int) * (n1 + 1), stream), "PairGraph memset failed");
        if (pairs < 1) return retval;
        GR_CHECK(hipMalloc(&d_ci, sizeof(int) * 2 * ms), "PairGraph hipMalloc d_ci failed");
        GR_CHECK(hipMalloc(&d_eid, sizeof(int) * 2 * ms), "PairGraph hipMalloc d_eid failed");
        GR_CHECK(hipMalloc(&d_up, sizeof(int) * (n1 + 1)), "PairGraph hipMalloc failed");
        GR_CHECK(hipMalloc(&d_low, sizeof(int) * (n1 + 1)), "PairGraph hipMalloc failed");
        GR_CHECK(hipMalloc(&d_deg, sizeof(unsigned) * (n1 + 1)), "PairGraph hipMalloc failed");
        // (the sort's buffers are free again: the canonical keys are in their own array)
        hipLaunchKernelGGL(SwapKeysKernel, dim3(PairGrid(pairs)), dim3(256), 0, stream, d_ckeys, pairs, col_bits, sort.Keys());
        GR_CHECK(hipGetLastError(), "SwapKeysKernel launch failed");
        unsigned long long *d_skeys = nullptr;
        d_sorted = nullptr;
        GR_CHECK(sort.Sort(pairs, key_bits, stream, &d_skeys), "PairGraph key sort failed");
        hipLaunchKernelGGL(RowStartsKernel, dim3(PairGrid(nodes + 1)), dim3(256), 0, stream, d_ckeys, d_skeys, pairs, nodes, col_bits, d_up, d_low);
        GR_CHECK(hipGetLastError(), "RowStartsKernel launch failed");
        hipLaunchKernelGGL(DegreesKernel, dim3(PairGrid(nodes + 1)), dim3(256), 0, stream, d_up, d_low, nodes, d_deg);
        GR_CHECK(hipGetLastError(), "DegreesKernel launch failed");
        GR_CHECK(DeviceExclusiveScan<int>(d_deg, d_ro, nodes + 1, d_sums, stream), "PairGraph offset scan failed");
        hipLaunchKernelGGL(FillRowsKernel, dim3(PairGrid(pairs)), dim3(256), 0, stream, d_ckeys, d_skeys, pairs, col_bits, d_up, d_low, d_ro, d_ci,
                           d_eid);
        GR_CHECK(hipGetLastError(), "FillRowsKernel launch failed");
        return retval;
    }
};

}  // namespace graphio
}  // namespace gunrock
