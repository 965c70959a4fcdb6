// util/device_array.hpp -- one device array and its owner.
//
// A DeviceArray<T> member says "this object allocated the array and frees it": a scope's scratch (graphio::DeviceScratch is this
// type), an array that grows (app::Grown holds one), the long-lived arrays of a problem and its pinned host words (PinnedArray) are
// all this.  A raw T * beside it is borrowed or a view: it points into an owned array, or it is the copy of an owner's pointer
// that a by-value kernel argument carries (the DataSlice of BFS, CC, SSSP, BC and PageRank, util::Frontier, BinPool).  It converts
// to T *, so kernel launches, null tests, pointer arithmetic and copies read as they do with a raw pointer; where a template
// deduces from it or a cast reinterprets it, take .p.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/util/error_utils.hpp>

namespace gunrock {
namespace util {

struct HipMem {
    static hipError_t Malloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t Free(void *p) { return hipFree(p); }
};

// pinned host memory (Flags: hipHostMallocDefault, or hipHostMallocMapped where a kernel writes it): the words a host loop reads
// back or a kernel posts to
template <unsigned Flags>
struct PinnedMem {
    static hipError_t Malloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
    static hipError_t Free(void *p) { return hipHostFree(p); }
};

// Mem: where the array lives.  HipMem unless said: PinnedArray below passes PinnedMem, and the host check of this header
// (tests/host/device_array_check.hip) a counting malloc.
template <typename T, typename Mem = HipMem>
struct DeviceArray {
    T *p = nullptr;

    DeviceArray() = default;
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    DeviceArray(DeviceArray &&other) noexcept : p(other.Release()) {}
    DeviceArray &operator=(DeviceArray &&other) noexcept
    {
        if (this != &other) Adopt(other.Release());
        return *this;
    }
    ~DeviceArray() { Free(); }

    operator T *() const { return p; }
    T *operator->() const { return p; }

    // what it held goes first; a count of 0 is one element, so that an empty graph's arrays are still arrays
    hipError_t Alloc(size_t count)
    {
        Free();
        void *raw = nullptr;
        const hipError_t error = GRError(Mem::Malloc(&raw, sizeof(T) * (count > 0 ? count : 1)), "DeviceArray malloc failed", __FILE__, __LINE__);
        if (!error) p = static_cast<T *>(raw);
        return error;
    }

    // owns an array that another owner gave up (graphio::Take)
    void Adopt(T *raw)
    {
        Free();
        p = raw;
    }

    // ... and gives its own up
    T *Release()
    {
        T *raw = p;
        p = nullptr;
        return raw;
    }

    void Free()
    {
        if (p) GRError(Mem::Free(p), "DeviceArray free failed", __FILE__, __LINE__);
        p = nullptr;
    }
};

template <typename T, unsigned Flags = hipHostMallocDefault>
using PinnedArray = DeviceArray<T, PinnedMem<Flags>>;

}  // namespace util
}  // namespace gunrock
