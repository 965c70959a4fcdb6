// app/rw/rw_build.hpp -- the kernels of the sorted copy RwProblem builds (rw_problem.hpp says what they build), on their own so that
// the neighbourhood sampler (app/sample) ranks its rows with the same ones.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace app {
namespace rw {

// ---------------- build kernels ----------------

static __global__ void NegativeWeightKernel(const int *d_w, long long m, int *d_bad)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride)
        if (d_w[i] < 0) *d_bad = 1;
}

// the row of entry i: the last row whose offset is <= i (rows without entries are stepped over)
__device__ __forceinline__ int RowOf(const int *ro, int nodes, long long i)
{
    int lo = 0, hi = nodes;  // ro[lo] <= i < ro[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (ro[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A: (weight << eb | entry)
static __global__ void WeightKeysKernel(const int *w, long long m, int eb, unsigned long long *keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride)
        keys[i] = (static_cast<unsigned long long>(w[i]) << eb) | static_cast<unsigned long long>(i);
}

// B: (column << eb | rank in A)
static __global__ void ColumnKeysKernel(const unsigned long long *a, const int *ci, long long m, int eb, unsigned long long *keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long r = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; r < m; r += stride)
        keys[r] = (static_cast<unsigned long long>(ci[a[r] & ((1ull << eb) - 1)]) << eb) | static_cast<unsigned long long>(r);
}

// C: (row << eb | rank in B)
static __global__ void RowKeysKernel(const unsigned long long *a, const unsigned long long *b, const int *ro, int nodes, long long m, int eb,
                                     unsigned long long *keys)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << eb) - 1;
    for (long long q = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; q < m; q += stride) {
        const long long entry = static_cast<long long>(a[b[q] & mask] & mask);
        keys[q] = (static_cast<unsigned long long>(RowOf(ro, nodes, entry)) << eb) | static_cast<unsigned long long>(q);
    }
}

static __global__ void SortedEntriesKernel(const unsigned long long *a, const unsigned long long *b, const unsigned long long *c, long long m, int eb,
                                           int *ci, int *w)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const unsigned long long mask = (1ull << eb) - 1;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride) {
        const unsigned long long kb = b[c[i] & mask];
        ci[i] = static_cast<int>(kb >> eb);
        w[i] = static_cast<int>(a[kb & mask] >> eb);
    }
}

// one wave a row, 64 entries a round
static __global__ void RowPrefixKernel(const int *ro, const int *w, int nodes, long long *prefix)
{
    const unsigned lane = util::LaneId();
    const long long wave0 = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) / 64;
    const long long nwaves = static_cast<long long>(gridDim.x) * blockDim.x / 64;
    for (long long v = wave0; v < nodes; v += nwaves) {
        const int b = ro[v], e = ro[v + 1];
        long long carry = 0;
        for (int base = b; base < e; base += 64) {  // (wave-uniform bounds)
            const int i = base + static_cast<int>(lane);
            long long x = i < e ? w[i] : 0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long o = __shfl_up(x, d, 64);
                if (static_cast<int>(lane) >= d) x += o;
            }
            if (i < e) prefix[i] = carry + x;
            carry += __shfl(x, 63, 64);
        }
    }
}

inline int BitsFor(long long count)  // bits that hold 0 .. count - 1, at least 1
{
    int bits = 1;
    while ((1ll << bits) < count) ++bits;
    return bits;
}

}  // namespace rw
}  // namespace app
}  // namespace gunrock
