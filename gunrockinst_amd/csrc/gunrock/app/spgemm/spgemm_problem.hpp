// app/spgemm/spgemm_problem.hpp -- device data of the sparse product C = A B.
//
// The reference snapshot has no app/spgemm.  The operands are rectangular and carry values, so the problem keeps its own matrices and
// stream, not ProblemBase's square graph: A (rows x inner) from Init, uploaded or borrowed, validated on the device before anything
// reads through it; the right operand as the option "right" names it --
//   SELF       B = A (rows == inner)
//   TRANSPOSE  B = A^T, built once on the device by graphio::DeviceTransposeCsr and kept; the order inside its rows is whatever that
//              build's atomics gave, which no result depends on
//   GIVEN      B from SetRight, uploaded or borrowed, validated the same way
// -- the per-row work, the row lists and the counts of an Enact, the GLOBAL regime's scratch slots (all 0 between launches) and the
// result C: offsets int32[rows + 1], cols int32[nnz] ascending inside a row, vals int64[nnz].  The result arrays grow with the largest
// result so far and are kept between Enacts.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/spgemm/spgemm_functor.hpp>
#include <gunrock/graphio/device_sort.hpp>
#include <gunrock/graphio/pair_graph.hpp>

namespace gunrock {
namespace app {
namespace spgemm {

// a CSR in device memory: the problem's own (freed with it) or the caller's
using DeviceMat = graphio::RectCsr;
inline Mat View(const DeviceMat &m) { return Mat{m.ro, m.ci, m.val, m.rows, m.cols}; }

struct SpgemmProblem {
    DeviceMat a, given, transposed;
    hipStream_t stream = nullptr;
    DeviceArray<unsigned long long> d_words;  // W_COUNT words of the kernels
    Grown<long long> work, babs;            // w_i per row of A; the sum of |b| per row of B
    Grown<int> lists;                       // 4 x rows
    Grown<unsigned> counts;                 // rows + 1: the distinct columns per row, then 0
    Grown<unsigned long long> sums, scratch;  // the scan's tile sums; the GLOBAL regime's slots
    Grown<int> offsets, cols;               // the result
    Grown<long long> vals;
    int malformed = 0;     // the last Init or SetRight found offsets or columns that are not a CSR
    long long nnz = -1;    // of the last finished Enact, or -1
    int result_cols = 0;   // ... and its number of columns
    bool with_values = false;

    SpgemmProblem() = default;
    SpgemmProblem(const SpgemmProblem &) = delete;
    SpgemmProblem &operator=(const SpgemmProblem &) = delete;
    ~SpgemmProblem()  // (the arrays free themselves)
    {
        if (stream) util::GRError(hipStreamDestroy(stream), "SpgemmProblem hipStreamDestroy failed", __FILE__, __LINE__);
    }

    // is m a CSR?  One kernel, one word read back.
    hipError_t Validate(const DeviceMat &m, bool *bad)
    {
        hipError_t retval = hipSuccess;
        unsigned long long word = 0;
        GR_CHECK(hipMemsetAsync(d_words + W_BAD, 0, sizeof(unsigned long long), stream), "SpgemmProblem memset failed");
        const long long count = m.rows + 1ll > m.nnz ? m.rows + 1ll : m.nnz;
        hipLaunchKernelGGL(graphio::ValidateRectKernel, dim3(CappedGrid((count + 255) / 256, 2048, 0)), dim3(256), 0, stream, m.ro, m.ci,
                           static_cast<long long>(m.rows), static_cast<long long>(m.nnz), m.cols, d_words + W_BAD);
        GR_CHECK(hipGetLastError(), "ValidateKernel launch failed");
        GR_CHECK(hipMemcpyAsync(&word, d_words + W_BAD, sizeof(word), hipMemcpyDeviceToHost, stream), "SpgemmProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "SpgemmProblem sync failed");
        *bad = word != 0;
        return retval;
    }

    hipError_t Admit(DeviceMat &m)
    {
        hipError_t retval = hipSuccess;
        bool bad = false;
        malformed = 0;
        if ((retval = Validate(m, &bad))) return retval;
        malformed = bad;
        if (bad) {
            m.Free();
            return hipErrorInvalidValue;
        }
        m.set = true;
        nnz = -1;
        return retval;
    }

    hipError_t Start()
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "SpgemmProblem hipStreamCreate failed");
        return d_words.Alloc(W_COUNT);
    }

    // One Init per object (grx_spgemm_init refuses a second one).  vals may be NULL.
    hipError_t Init(int rows, int inner, int entries, const int *h_ro, const int *h_ci, const int *h_val)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Start())) return retval;
        if ((retval = a.Upload(rows, inner, entries, h_ro, h_ci, h_val))) return retval;
        return Admit(a);
    }
    hipError_t InitFromDevice(int rows, int inner, int entries, int *d_ro, int *d_ci, int *d_val)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Start())) return retval;
        a.Borrow(rows, inner, entries, d_ro, d_ci, d_val);
        return Admit(a);
    }
    // the right operand of GIVEN (the caller has held its rows against A's inner)
    hipError_t SetRight(int rows, int cols_, int entries, const int *ro, const int *ci, const int *val, bool on_device)
    {
        hipError_t retval = hipSuccess;
        if (on_device) given.Borrow(rows, cols_, entries, const_cast<int *>(ro), const_cast<int *>(ci), const_cast<int *>(val));
        else if ((retval = given.Upload(rows, cols_, entries, ro, ci, val))) return retval;
        return Admit(given);
    }

    // A^T, once: counting sort by column.  DeviceTransposeCsr walks as many rows as it has columns, so the offsets of a wide A are
    // padded with empty rows first; of a tall A the transpose's offsets beyond `inner` rows are the padding.
    hipError_t NeedTransposed()
    {
        hipError_t retval = hipSuccess;
        if (transposed.set) return retval;
        const int n = a.rows > a.cols ? a.rows : a.cols;
        const size_t n1 = static_cast<size_t>(n) + 1;
        if ((retval = transposed.Own(a.cols, a.rows, a.nnz, n1, a.val != nullptr))) return retval;
        graphio::DeviceScratch<int> padded;
        const int *ro = a.ro;
        if (n > a.rows) {
            if ((retval = padded.Alloc(n1))) return retval;
            hipLaunchKernelGGL(graphio::PadOffsetsKernel, dim3(CappedGrid((n + 256) / 256, 2048, 0)), dim3(256), 0, stream, a.ro, static_cast<long long>(a.rows),
                               static_cast<long long>(n), a.nnz, padded.p);
            GR_CHECK(hipGetLastError(), "PadOffsetsKernel launch failed");
            ro = padded.p;
        }
        GR_CHECK(graphio::DeviceTransposeCsr(n, a.nnz, ro, a.ci, transposed.ro, transposed.ci, stream, reinterpret_cast<const unsigned *>(a.val),
                                             reinterpret_cast<unsigned *>(transposed.val)),
                 "SpgemmProblem transpose failed");  // (synchronises: `padded` may go)
        transposed.set = true;
        return retval;
    }

    // no result
    hipError_t Reset()
    {
        nnz = -1;
        return hipSuccess;
    }

    template <typename T>
    hipError_t Read(T *host, const T *device, size_t count)
    {
        if (!host || !count) return hipSuccess;
        return util::GRError(hipMemcpy(host, device, sizeof(T) * count, hipMemcpyDeviceToHost), "SpgemmProblem read failed", __FILE__, __LINE__);
    }
    // Any may be NULL.  h_vals of a pattern_only result is refused by the caller.
    hipError_t Extract(int *h_offsets, int *h_cols, long long *h_vals)
    {
        hipError_t retval = hipSuccess;
        const size_t count = static_cast<size_t>(nnz > 0 ? nnz : 0);
        if ((retval = Read(h_offsets, offsets.p, static_cast<size_t>(a.rows) + 1))) return retval;
        if ((retval = Read(h_cols, cols.p, count))) return retval;
        return Read(h_vals, vals.p, count);
    }
};

}  // namespace spgemm
}  // namespace app
}  // namespace gunrock
