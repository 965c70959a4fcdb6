// graphio/relabel.hpp -- a copy of a CSR renumbered hub-first, edgeless-last (BFS, DESIGN §3.3 k).
//
// The vertices are split into three tiers and each tier keeps the caller's order (a stable partition):
//   tier 0: hubs, degree >= T, where T is the smallest threshold that leaves at most `max_hubs` vertices in the tier;
//   tier 1: every other vertex that has edges;
//   tier 2: the vertices without edges.
// Because the partition is stable, a vertex's new id follows from two bit masks and two prefix counts per 64-vertex word of
// the caller's numbering (RelabelView::NewId): no id table is needed to go from the caller's numbering to the new one, and a
// pass in caller order reads the new-numbered arrays almost in order (tier 1 is the bulk of every word).  new -> old is
// built only on request (predecessor values).
//
// The copy keeps every CSR entry of the input, self-loops and duplicate entries included, so every vertex keeps its degree.
// Rows are sorted by new column id (hub neighbours first).  The build is deterministic: one radix sort of the full
// (new row, new column) keys.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/graphio/device_csr.hpp>
#include <gunrock/graphio/device_sort.hpp>
#include <gunrock/util/device_array.hpp>

namespace gunrock {
namespace graphio {

// device-side view of the renumbering (by-value kernel argument)
struct RelabelView {
    const unsigned long long *d_hub = nullptr;   // per 64-vertex word of the caller's numbering: tier-0 bits
    const unsigned long long *d_edge = nullptr;  // tier-1 bits
    const unsigned *d_base0 = nullptr;           // tier-0 vertices before the word
    const unsigned *d_base1 = nullptr;           // tier-1 vertices before the word
    long long hubs = 0;                          // tier-0 size
    long long with_edges = 0;                    // tier-0 + tier-1 size

    __device__ __forceinline__ long long NewId(long long v) const
    {
        const long long w = v >> 6;
        const unsigned long long low = (1ull << (v & 63)) - 1ull;
        const unsigned long long h = d_hub[w], e = d_edge[w];
        if ((h >> (v & 63)) & 1ull) return d_base0[w] + __popcll(h & low);
        if ((e >> (v & 63)) & 1ull) return hubs + d_base1[w] + __popcll(e & low);
        return with_edges + (v - d_base0[w] - d_base1[w] - __popcll((h | e) & low));
    }
};

// per-block LDS histogram of the small degrees, global atomics for the rest
constexpr int kRelabelLdsBins = 1024;
static __global__ __launch_bounds__(256) void DegreeHistogramKernel(const int *d_row_offsets, long long nodes, int max_degree, unsigned *d_hist)
{
    __shared__ unsigned bins[kRelabelLdsBins];
    for (int i = threadIdx.x; i < kRelabelLdsBins; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        int d = d_row_offsets[v + 1] - d_row_offsets[v];
        d = d < 0 ? 0 : (d > max_degree ? max_degree : d);
        if (d < kRelabelLdsBins) atomicAdd(&bins[d], 1u);
        else atomicAdd(d_hist + d, 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kRelabelLdsBins && i <= max_degree; i += blockDim.x)
        if (bins[i]) atomicAdd(d_hist + i, bins[i]);
}

static __global__ void MaxDegreeKernel(const int *d_row_offsets, long long nodes, int *d_max)
{
    int best = 0;
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const int d = d_row_offsets[v + 1] - d_row_offsets[v];
        best = d > best ? d : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_down(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(d_max, best);
}

// one wave per 64-vertex word: the tier masks and the tier-0 / tier-1 counts of the word
static __global__ void TierMaskKernel(const int *d_row_offsets, long long nodes, long long words64, int threshold,
                                      unsigned long long *d_hub, unsigned long long *d_edge, unsigned *d_count0, unsigned *d_count1)
{
    const unsigned lane = threadIdx.x & 63;
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / 64;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / 64;
    for (long long w = wave0; w < words64; w += nwaves) {
        const long long v = w * 64 + lane;
        const int d = v < nodes ? d_row_offsets[v + 1] - d_row_offsets[v] : 0;
        const unsigned long long h = __ballot(d > 0 && d >= threshold);
        const unsigned long long e = __ballot(d > 0 && d < threshold);
        if (lane == 0) {
            d_hub[w] = h;
            d_edge[w] = e;
            d_count0[w] = static_cast<unsigned>(__popcll(h));
            d_count1[w] = static_cast<unsigned>(__popcll(e));
        }
    }
}

// new degree per new id (the scan input of the new row offsets) and, on request, new -> old
static __global__ void RelabelDegreesKernel(RelabelView map, const int *d_row_offsets, long long nodes, unsigned *d_new_degree, int *d_old_of_new)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long v = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; v < nodes; v += stride) {
        const long long x = map.NewId(v);
        d_new_degree[x] = static_cast<unsigned>(d_row_offsets[v + 1] - d_row_offsets[v]);
        if (d_old_of_new) d_old_of_new[x] = static_cast<int>(v);
    }
}

// key of every entry, at the entry's own position: (new row << col_bits) | new column.  One wave per 64 rows (short rows by
// their lane, long rows by the whole wave).
static __global__ void RelabelKeysKernel(RelabelView map, const int *d_row_offsets, const int *d_cols, long long nodes, int col_bits,
                                         unsigned long long *d_keys)
{
    const unsigned lane = threadIdx.x & 63;
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / 64;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / 64;
    const long long groups = (nodes + 63) / 64;
    for (long long g = wave0; g < groups; g += nwaves) {
        const long long v = g * 64 + lane;
        int b = 0, e = 0;
        unsigned long long row = 0;
        if (v < nodes) {
            b = d_row_offsets[v];
            e = d_row_offsets[v + 1];
            row = static_cast<unsigned long long>(map.NewId(v)) << col_bits;
        }
        const bool long_row = (e - b) > 16;
        if (!long_row)
            for (int i = b; i < e; ++i) d_keys[i] = row | static_cast<unsigned long long>(map.NewId(d_cols[i]));
        unsigned long long todo = __ballot(long_row);
        while (todo) {
            const int leader = __ffsll(static_cast<long long>(todo)) - 1;
            const int lb = __shfl(b, leader, 64), le = __shfl(e, leader, 64);
            const unsigned long long lrow = __shfl(row, leader, 64);
            for (int i = lb + static_cast<int>(lane); i < le; i += 64) d_keys[i] = lrow | static_cast<unsigned long long>(map.NewId(d_cols[i]));
            todo &= todo - 1;
        }
    }
}

static __global__ void RelabelColsKernel(const unsigned long long *d_sorted, long long edges, unsigned long long col_mask, int *d_cols)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < edges; i += stride)
        d_cols[i] = static_cast<int>(d_sorted[i] & col_mask);
}

// Owns the renumbered CSR and the renumbering.  Host copies of the per-word masks and bases map single ids (the source of
// a search) without a device round trip.
struct RelabelledCsr {
    long long nodes = 0, edges = 0, words64 = 0;
    util::DeviceArray<int> d_row_offsets, d_cols;
    util::DeviceArray<int> d_old_of_new;  // only when built with predecessors
    util::DeviceArray<unsigned long long> d_hub, d_edge;
    util::DeviceArray<unsigned> d_base0, d_base1;
    long long hubs = 0, with_edges = 0;
    int threshold = 0;
    float build_ms = 0.f;
    size_t bytes = 0;  // device memory held
    std::vector<unsigned long long> h_hub, h_edge;
    std::vector<unsigned> h_base0, h_base1;

    bool Ready() const { return d_row_offsets != nullptr; }
    RelabelView View() const
    {
        RelabelView m;
        m.d_hub = d_hub;
        m.d_edge = d_edge;
        m.d_base0 = d_base0;
        m.d_base1 = d_base1;
        m.hubs = hubs;
        m.with_edges = with_edges;
        return m;
    }
    long long NewId(long long v) const
    {
        const long long w = v >> 6;
        const unsigned long long low = (1ull << (v & 63)) - 1ull;
        const unsigned long long h = h_hub[w], e = h_edge[w];
        if ((h >> (v & 63)) & 1ull) return h_base0[w] + __builtin_popcountll(h & low);
        if ((e >> (v & 63)) & 1ull) return hubs + h_base1[w] + __builtin_popcountll(e & low);
        return with_edges + (v - h_base0[w] - h_base1[w] - __builtin_popcountll((h | e) & low));
    }

    void Release()
    {
        d_row_offsets.Free();
        d_cols.Free();
        d_old_of_new.Free();
        d_hub.Free();
        d_edge.Free();
        d_base0.Free();
        d_base1.Free();
        bytes = 0;
    }

    // Build the copy of the CSR (d_row_offsets[nodes + 1], d_cols[edges]) with at most max_hubs hubs.  Synchronous.
    hipError_t Build(long long nodes_, long long edges_, const int *d_ro, const int *d_ci, long long max_hubs, bool old_of_new,
                     hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        Release();
        nodes = nodes_;
        edges = edges_;
        words64 = (nodes + 63) / 64 + 1;  // (one spare word: NewId of the last id reads its own word only)
        hipEvent_t t0 = nullptr, t1 = nullptr;
        GR_CHECK(hipEventCreate(&t0), "hipEventCreate failed");
        GR_CHECK(hipEventCreate(&t1), "hipEventCreate failed");
        GR_CHECK(hipEventRecord(t0, stream), "hipEventRecord failed");

        // 1. threshold: the smallest T >= 1 with at most max_hubs vertices of degree >= T (degree histogram)
        util::DeviceArray<int> d_max;
        GR_CHECK(d_max.Alloc(1), "RelabelledCsr scratch failed");
        GR_CHECK(hipMemsetAsync(d_max, 0, sizeof(int), stream), "RelabelledCsr memset failed");
        const unsigned grid = 2048;
        if (nodes > 0) {
            hipLaunchKernelGGL(MaxDegreeKernel, dim3(grid), dim3(256), 0, stream, d_ro, nodes, d_max);
            GR_CHECK(hipGetLastError(), "MaxDegreeKernel launch failed");
        }
        int max_degree = 0;
        GR_CHECK(hipMemcpyAsync(&max_degree, d_max, sizeof(int), hipMemcpyDeviceToHost, stream), "RelabelledCsr read failed");
        GR_CHECK(hipStreamSynchronize(stream), "RelabelledCsr sync failed");
        d_max.Free();
        std::vector<unsigned> hist(static_cast<size_t>(max_degree) + 1, 0u);
        {
            util::DeviceArray<unsigned> d_hist;
            GR_CHECK(d_hist.Alloc(hist.size()), "RelabelledCsr scratch failed");
            GR_CHECK(hipMemsetAsync(d_hist, 0, sizeof(unsigned) * hist.size(), stream), "RelabelledCsr memset failed");
            if (nodes > 0) {
                hipLaunchKernelGGL(DegreeHistogramKernel, dim3(grid), dim3(256), 0, stream, d_ro, nodes, max_degree, d_hist);
                GR_CHECK(hipGetLastError(), "DegreeHistogramKernel launch failed");
            }
            GR_CHECK(hipMemcpyAsync(hist.data(), d_hist, sizeof(unsigned) * hist.size(), hipMemcpyDeviceToHost, stream), "RelabelledCsr read failed");
            GR_CHECK(hipStreamSynchronize(stream), "RelabelledCsr sync failed");
        }
        threshold = max_degree + 1;  // no hubs
        for (long long above = 0, d = max_degree; d >= 1; --d) {
            above += hist[static_cast<size_t>(d)];
            if (above > max_hubs) break;
            threshold = static_cast<int>(d);
        }

        // 2. tier masks, per-word counts, prefix counts
        GR_CHECK(d_hub.Alloc(static_cast<size_t>(words64)), "RelabelledCsr d_hub failed");
        GR_CHECK(d_edge.Alloc(static_cast<size_t>(words64)), "RelabelledCsr d_edge failed");
        GR_CHECK(d_base0.Alloc(static_cast<size_t>(words64)), "RelabelledCsr d_base0 failed");
        GR_CHECK(d_base1.Alloc(static_cast<size_t>(words64)), "RelabelledCsr d_base1 failed");
        util::DeviceArray<unsigned> d_counts;
        util::DeviceArray<unsigned long long> d_sums;
        const long long scan_n = (nodes + 1 > 2 * words64) ? nodes + 1 : 2 * words64;
        GR_CHECK(d_counts.Alloc(static_cast<size_t>(scan_n)), "RelabelledCsr scratch failed");
        GR_CHECK(d_sums.Alloc(static_cast<size_t>(ScanScratchWords(scan_n))), "RelabelledCsr scratch failed");
        {
            long long g = (words64 + 3) / 4;
            if (g > 4096) g = 4096;
            hipLaunchKernelGGL(TierMaskKernel, dim3(static_cast<unsigned>(g)), dim3(256), 0, stream, d_ro, nodes, words64, threshold, d_hub, d_edge,
                               d_counts, d_counts + words64);
            GR_CHECK(hipGetLastError(), "TierMaskKernel launch failed");
        }
        GR_CHECK(DeviceExclusiveScan<unsigned>(d_counts, d_base0, words64, d_sums, stream), "RelabelledCsr tier-0 scan failed");
        GR_CHECK(DeviceExclusiveScan<unsigned>(d_counts + words64, d_base1, words64, d_sums, stream), "RelabelledCsr tier-1 scan failed");
        h_hub.resize(static_cast<size_t>(words64));
        h_edge.resize(static_cast<size_t>(words64));
        h_base0.resize(static_cast<size_t>(words64));
        h_base1.resize(static_cast<size_t>(words64));
        GR_CHECK(hipMemcpyAsync(h_hub.data(), d_hub, sizeof(unsigned long long) * words64, hipMemcpyDeviceToHost, stream), "RelabelledCsr read failed");
        GR_CHECK(hipMemcpyAsync(h_edge.data(), d_edge, sizeof(unsigned long long) * words64, hipMemcpyDeviceToHost, stream), "RelabelledCsr read failed");
        GR_CHECK(hipMemcpyAsync(h_base0.data(), d_base0, sizeof(unsigned) * words64, hipMemcpyDeviceToHost, stream), "RelabelledCsr read failed");
        GR_CHECK(hipMemcpyAsync(h_base1.data(), d_base1, sizeof(unsigned) * words64, hipMemcpyDeviceToHost, stream), "RelabelledCsr read failed");
        GR_CHECK(hipStreamSynchronize(stream), "RelabelledCsr sync failed");
        hubs = static_cast<long long>(h_base0[words64 - 1]) + __builtin_popcountll(h_hub[words64 - 1]);
        with_edges = hubs + static_cast<long long>(h_base1[words64 - 1]) + __builtin_popcountll(h_edge[words64 - 1]);
        const RelabelView map = View();

        // 3. new row offsets (every entry kept: the degrees do not change) and new -> old
        GR_CHECK(d_row_offsets.Alloc(static_cast<size_t>(nodes + 1)), "RelabelledCsr d_row_offsets failed");
        GR_CHECK(hipMemsetAsync(d_counts, 0, sizeof(unsigned) * static_cast<size_t>(nodes + 1), stream), "RelabelledCsr memset failed");
        if (old_of_new)
            GR_CHECK(d_old_of_new.Alloc(static_cast<size_t>(nodes)), "RelabelledCsr d_old_of_new failed");
        if (nodes > 0) {
            hipLaunchKernelGGL(RelabelDegreesKernel, dim3(grid), dim3(256), 0, stream, map, d_ro, nodes, d_counts, d_old_of_new);
            GR_CHECK(hipGetLastError(), "RelabelDegreesKernel launch failed");
        }
        GR_CHECK(DeviceExclusiveScan<int>(d_counts, d_row_offsets, nodes + 1, d_sums, stream), "RelabelledCsr offsets scan failed");

        // 4. columns: sort the (new row, new column) keys of all entries
        GR_CHECK(d_cols.Alloc(static_cast<size_t>(edges)), "RelabelledCsr d_cols failed");
        if (edges > 0) {
            int col_bits = 1;
            while ((1ll << col_bits) < nodes) ++col_bits;
            DeviceKeySort sorter;
            GR_CHECK(sorter.Reserve(edges), "RelabelledCsr sort reserve failed");
            hipLaunchKernelGGL(RelabelKeysKernel, dim3(8192), dim3(256), 0, stream, map, d_ro, d_ci, nodes, col_bits, sorter.Keys());
            GR_CHECK(hipGetLastError(), "RelabelKeysKernel launch failed");
            unsigned long long *sorted = nullptr;
            GR_CHECK(sorter.Sort(edges, 2 * col_bits, stream, &sorted), "RelabelledCsr sort failed");
            hipLaunchKernelGGL(RelabelColsKernel, dim3(8192), dim3(256), 0, stream, sorted, edges, (1ull << col_bits) - 1ull, d_cols);
            GR_CHECK(hipGetLastError(), "RelabelColsKernel launch failed");
            GR_CHECK(hipStreamSynchronize(stream), "RelabelledCsr sort sync failed");
        }
        GR_CHECK(hipEventRecord(t1, stream), "hipEventRecord failed");
        GR_CHECK(hipEventSynchronize(t1), "hipEventSynchronize failed");
        GR_CHECK(hipEventElapsedTime(&build_ms, t0, t1), "hipEventElapsedTime failed");
        GR_CHECK(hipEventDestroy(t0), "hipEventDestroy failed");
        GR_CHECK(hipEventDestroy(t1), "hipEventDestroy failed");
        bytes = sizeof(int) * static_cast<size_t>(nodes + 1 + edges + (old_of_new ? nodes : 0)) + (2 * sizeof(unsigned long long) + 2 * sizeof(unsigned)) * words64;
        return retval;
    }
};

}  // namespace graphio
}  // namespace gunrock
