// app/rw/rw_draw.hpp -- the counter-based draw and the two first-order choices of the random walks (rw_functor.hpp has the definition
// they belong to), host and device.  On their own so that the neighbourhood sampler (app/sample) draws and chooses with the same ones.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include <gunrock/graphio/splitmix.hpp>

namespace gunrock {
namespace app {
namespace rw {

GRX_HOST_DEVICE inline uint64_t Draw(uint64_t seed, uint64_t walk, uint64_t step, uint64_t t)
{
    return graphio::Mix64(seed ^ graphio::Mix64((walk << 32) | (step << 8) | t));
}

// the high word of the 128-bit product
GRX_HOST_DEVICE inline uint64_t MulHigh(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

// d > 0
GRX_HOST_DEVICE inline int ChooseUniform(uint64_t r, int d) { return static_cast<int>(((r >> 32) * static_cast<uint64_t>(d)) >> 32); }

// prefix[0 .. d - 1]: the inclusive prefix sums of the row's weights, prefix[d - 1] > 0
GRX_HOST_DEVICE inline int ChooseWeighted(uint64_t r, const long long *prefix, int d)
{
    const long long t = static_cast<long long>(MulHigh(r, static_cast<uint64_t>(prefix[d - 1])));
    int lo = 0, hi = d - 1;  // prefix[hi] > t throughout
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (prefix[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

}  // namespace rw
}  // namespace app
}  // namespace gunrock
