// graphio/rect_csr.hpp -- a rectangular CSR in device memory and what the families that read one share (the sparse product, §3.26, and
// the bipartite matching, §3.28): its owner, its validation and the padding of its offsets for a transpose over the larger side.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/util/device_array.hpp>
#include <gunrock/util/device_intrinsics.hpp>
#include <gunrock/util/error_utils.hpp>

namespace gunrock {
namespace graphio {

// a CSR of shape (rows, cols) in device memory: the holder's own (freed with it) or the caller's
struct RectCsr {
    util::DeviceArray<int> own_ro, own_ci, own_val;    // the holder's own arrays, when it made them
    int *ro = nullptr, *ci = nullptr, *val = nullptr;  // what the kernels read: those, or the caller's
    int rows = 0, cols = 0, nnz = 0;
    bool set = false;

    void Free() { *this = RectCsr(); }
    // arrays of its own: `offsets` row offsets, nnz_ columns and, with_val, as many values
    hipError_t Own(int rows_, int cols_, int nnz_, size_t offsets, bool with_val)
    {
        hipError_t retval = hipSuccess;
        Free();
        rows = rows_, cols = cols_, nnz = nnz_;
        if ((retval = own_ro.Alloc(offsets))) return retval;
        if ((retval = own_ci.Alloc(static_cast<size_t>(nnz)))) return retval;
        if (with_val && (retval = own_val.Alloc(static_cast<size_t>(nnz)))) return retval;
        ro = own_ro, ci = own_ci, val = own_val;
        return retval;
    }
    hipError_t Upload(int rows_, int cols_, int nnz_, const int *h_ro, const int *h_ci, const int *h_val)
    {
        hipError_t retval = hipSuccess;
        const size_t n1 = static_cast<size_t>(rows_) + 1, m = static_cast<size_t>(nnz_);
        if ((retval = Own(rows_, cols_, nnz_, n1, h_val != nullptr))) return retval;
        GR_CHECK(hipMemcpy(ro, h_ro, sizeof(int) * n1, hipMemcpyHostToDevice), "RectCsr hipMemcpy failed");
        if (m) GR_CHECK(hipMemcpy(ci, h_ci, sizeof(int) * m, hipMemcpyHostToDevice), "RectCsr hipMemcpy failed");
        if (h_val && m) GR_CHECK(hipMemcpy(val, h_val, sizeof(int) * m, hipMemcpyHostToDevice), "RectCsr hipMemcpy failed");
        return retval;
    }
    void Borrow(int rows_, int cols_, int nnz_, int *d_ro, int *d_ci, int *d_val)
    {
        Free();
        rows = rows_, cols = cols_, nnz = nnz_;
        ro = d_ro, ci = d_ci, val = d_val;
    }
};

// *bad = 1 unless ro / ci are a CSR of `rows` rows, `nnz` entries and columns in [0, cols)
static __global__ void ValidateRectKernel(const int *ro, const int *ci, long long rows, long long nnz, int cols, unsigned long long *bad_word)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    const long long count = rows + 1 > nnz ? rows + 1 : nnz;
    bool bad = false;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (i <= rows) {
            const long long at = ro[i];
            bad |= at < 0 || at > nnz || (i == 0 && at != 0) || (i == rows && at != nnz);
            if (i < rows) bad |= at > ro[i + 1];
        }
        if (i < nnz) {
            const int j = ci[i];
            bad |= j < 0 || j >= cols;
        }
    }
    if (__ballot(bad) && util::LaneId() == 0) *bad_word = 1ull;
}

// offsets of `rows` rows as offsets of `padded` >= rows rows, the added ones empty
static __global__ void PadOffsetsKernel(const int *ro, long long rows, long long padded, int nnz, int *out)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i <= padded; i += stride) out[i] = i <= rows ? ro[i] : nnz;
}

}  // namespace graphio
}  // namespace gunrock
