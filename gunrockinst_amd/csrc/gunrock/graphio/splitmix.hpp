// graphio/splitmix.hpp -- the splitmix64 finaliser, once, for the host and the device.
//
// Every counter-based stream of the library is Mix64(seed ^ Mix64(counter)): the seeded R-MAT generator on the host (rmat.hpp) and
// on the device (rmat_device.hpp), and the draws of the random walks (app/rw/rw_functor.hpp).  devgraph._splitmix64 is the same
// function in Python.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GRX_HOST_DEVICE __host__ __device__
#else
#define GRX_HOST_DEVICE
#endif

namespace gunrock {
namespace graphio {

GRX_HOST_DEVICE inline uint64_t Mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

}  // namespace graphio
}  // namespace gunrock
