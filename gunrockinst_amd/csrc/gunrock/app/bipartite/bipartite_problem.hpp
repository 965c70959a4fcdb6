// app/bipartite/bipartite_problem.hpp -- device data of the maximum bipartite matching and the Dulmage-Mendelsohn decomposition.
//
// The operand is a rectangular pattern, so the problem keeps its own matrices and stream as SpgemmProblem does (graphio/rect_csr.hpp
// is what the two share; the transpose recipe is SpgemmProblem::NeedTransposed's): A (rows x cols) from Init, uploaded or borrowed,
// validated on the device before anything reads through it, and A^T, built once at Init and kept.  Beside them the two mate arrays, the search's
// arrays (sized for the larger side: the same ones serve the search from the columns and the one from the rows), the parts, the
// cover and -- once asked for -- the contracted square part, which lives as long as the problem.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/bipartite/bipartite_functor.hpp>
#include <gunrock/app/problem_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/graphio/device_sort.hpp>
#include <gunrock/graphio/pair_graph.hpp>
#include <gunrock/graphio/rect_csr.hpp>

namespace gunrock {
namespace app {
namespace bipartite {

constexpr int kBadMatching = -5;  // GRX_BIPARTITE_BAD_MATCHING

struct BipartiteProblem {
    graphio::RectCsr a, t;  // A and A^T
    hipStream_t stream = nullptr;
    DeviceArray<unsigned long long> d_valid;  // ValidateRectKernel's word
    DeviceArray<unsigned> d_words;
    DeviceArray<unsigned long long> d_counts;
    DeviceArray<Front> d_front;
    DeviceArray<int> d_mate_row, d_mate_col, d_row_part, d_col_part;
    DeviceArray<unsigned char> d_row_cover, d_col_cover;
    DeviceArray<int> d_pred, d_root, d_winner, d_queue;  // max(rows, cols) each
    DeviceArray<int> d_local;                            // rows + 1: the square rows before a row
    DeviceArray<int> d_square;                           // two ints: k and the arcs
    Grown<int> sq_ro, sq_ci, sq_map;                     // the contracted square part
    int rows = 0, cols = 0, nnz = 0, larger = 0;
    int malformed = 0;      // Init found offsets or columns that are not a CSR
    int bad_matching = 0;   // the last Reset was given no matching: the start is the empty one
    bool fresh = false;     // a Reset was made and no Enact has run since
    int state = -1;         // BIPARTITE_MAXIMUM / BIPARTITE_CAPPED of the last certified Enact, or -1: no result
    long long size = 0;     // ... and its matching's size
    long long part_size[6] = {0, 0, 0, 0, 0, 0};
    int square_k = -1, square_arcs = 0;  // of the square graph, once built for this result (-1: not)
    double build_ms = 0;    // the transpose

    BipartiteProblem() = default;
    BipartiteProblem(const BipartiteProblem &) = delete;
    BipartiteProblem &operator=(const BipartiteProblem &) = delete;
    ~BipartiteProblem()  // (the arrays free themselves)
    {
        if (stream) util::GRError(hipStreamDestroy(stream), "BipartiteProblem hipStreamDestroy failed", __FILE__, __LINE__);
    }

    Sides DeviceSides() const { return Sides{a.ro, a.ci, d_mate_row.p, d_mate_col.p, rows, cols}; }

    // A^T by SpgemmProblem::NeedTransposed's recipe: the offsets of a wide A padded with empty rows, DeviceTransposeCsr over the
    // larger side
    hipError_t Transpose()
    {
        hipError_t retval = hipSuccess;
        const size_t n1 = static_cast<size_t>(larger) + 1;
        if ((retval = t.Own(cols, rows, nnz, n1, false))) return retval;
        graphio::DeviceScratch<int> padded;
        const int *ro = a.ro;
        if (larger > rows) {
            if ((retval = padded.Alloc(n1))) return retval;
            hipLaunchKernelGGL(graphio::PadOffsetsKernel, dim3(CappedGrid((larger + 256) / 256, 2048, 0)), dim3(256), 0, stream, a.ro,
                               static_cast<long long>(rows), static_cast<long long>(larger), nnz, padded.p);
            GR_CHECK(hipGetLastError(), "PadOffsetsKernel launch failed");
            ro = padded.p;
        }
        GR_CHECK(graphio::DeviceTransposeCsr(larger, nnz, ro, a.ci, t.ro, t.ci, stream), "BipartiteProblem transpose failed");  // (synchronises)
        t.set = true;
        return retval;
    }

    hipError_t Build()
    {
        hipError_t retval = hipSuccess;
        rows = a.rows, cols = a.cols, nnz = a.nnz;
        larger = rows > cols ? rows : cols;
        malformed = 0;
        if ((retval = d_valid.Alloc(1))) return retval;
        GR_CHECK(hipMemsetAsync(d_valid, 0, sizeof(unsigned long long), stream), "BipartiteProblem memset failed");
        const long long count = rows + 1ll > nnz ? rows + 1ll : nnz;
        hipLaunchKernelGGL(graphio::ValidateRectKernel, dim3(CappedGrid((count + 255) / 256, 2048, 0)), dim3(256), 0, stream, a.ro, a.ci,
                           static_cast<long long>(rows), static_cast<long long>(nnz), cols, d_valid.p);
        GR_CHECK(hipGetLastError(), "ValidateRectKernel launch failed");
        unsigned long long word = 0;
        GR_CHECK(hipMemcpyAsync(&word, d_valid.p, sizeof(word), hipMemcpyDeviceToHost, stream), "BipartiteProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "BipartiteProblem sync failed");
        if (word) {
            malformed = 1;
            a.Free();
            return hipErrorInvalidValue;
        }
        a.set = true;

        graphio::BuildEvents ev;
        if ((retval = ev.Create(2))) return retval;
        if ((retval = ev.Record(0, stream))) return retval;
        if ((retval = Transpose())) return retval;
        if ((retval = ev.Record(1, stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "BipartiteProblem sync failed");
        if ((retval = ev.Elapsed(0, 1, &build_ms))) return retval;

        if ((retval = d_words.Alloc(W_COUNT))) return retval;
        if ((retval = d_counts.Alloc(C_COUNT))) return retval;
        if ((retval = d_front.Alloc(1))) return retval;
        if ((retval = d_square.Alloc(2))) return retval;
        DeviceArray<int> *row_arrays[] = {&d_mate_row, &d_row_part}, *col_arrays[] = {&d_mate_col, &d_col_part};
        DeviceArray<int> *search_arrays[] = {&d_pred, &d_root, &d_winner, &d_queue};
        for (DeviceArray<int> *x : row_arrays) if ((retval = x->Alloc(static_cast<size_t>(rows)))) return retval;
        for (DeviceArray<int> *x : col_arrays) if ((retval = x->Alloc(static_cast<size_t>(cols)))) return retval;
        for (DeviceArray<int> *x : search_arrays) if ((retval = x->Alloc(static_cast<size_t>(larger)))) return retval;
        if ((retval = d_local.Alloc(static_cast<size_t>(rows) + 1))) return retval;
        if ((retval = d_row_cover.Alloc(static_cast<size_t>(rows)))) return retval;
        if ((retval = d_col_cover.Alloc(static_cast<size_t>(cols)))) return retval;
        return Reset(nullptr);
    }

    hipError_t Start()
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "BipartiteProblem hipStreamCreate failed");
        return retval;
    }

    // One Init per object (grx_bipartite_init refuses a second one)
    hipError_t Init(int rows_, int cols_, int entries, const int *h_ro, const int *h_ci)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Start())) return retval;
        if ((retval = a.Upload(rows_, cols_, entries, h_ro, h_ci, nullptr))) return retval;
        return Build();
    }
    hipError_t InitFromDevice(int rows_, int cols_, int entries, int *d_ro, int *d_ci)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Start())) return retval;
        a.Borrow(rows_, cols_, entries, d_ro, d_ci, nullptr);
        return Build();
    }

    // The start matching: h_mate_row (a column or -1 per row), checked on the device, or NULL for the empty one.  One that is no
    // matching sets bad_matching and leaves the empty one.
    hipError_t Reset(const int *h_mate_row)
    {
        hipError_t retval = hipSuccess;
        bad_matching = 0;
        state = -1;
        square_k = -1;
        GR_CHECK(hipMemsetAsync(d_words, 0, sizeof(unsigned) * W_COUNT, stream), "BipartiteProblem memset failed");
        GR_CHECK(hipMemsetAsync(d_mate_col, 0xFF, sizeof(int) * static_cast<size_t>(cols), stream), "BipartiteProblem memset failed");
        if (h_mate_row && rows > 0) {
            GR_CHECK(hipMemcpyAsync(d_mate_row, h_mate_row, sizeof(int) * static_cast<size_t>(rows), hipMemcpyHostToDevice, stream),
                     "BipartiteProblem upload failed");
            hipLaunchKernelGGL(CheckStartKernel, GridFor(rows, 0), dim3(kThreads), 0, stream, DeviceSides(), d_words.p);
            GR_CHECK(hipGetLastError(), "CheckStartKernel launch failed");
            unsigned bad = 0;
            GR_CHECK(hipMemcpyAsync(&bad, d_words + W_BAD, sizeof(bad), hipMemcpyDeviceToHost, stream), "BipartiteProblem read-back failed");
            GR_CHECK(hipStreamSynchronize(stream), "BipartiteProblem Reset sync failed");  // (h_mate_row is the caller's again)
            if (bad) {
                bad_matching = 1;
                GR_CHECK(hipMemsetAsync(d_words, 0, sizeof(unsigned) * W_COUNT, stream), "BipartiteProblem memset failed");
                GR_CHECK(hipMemsetAsync(d_mate_col, 0xFF, sizeof(int) * static_cast<size_t>(cols), stream), "BipartiteProblem memset failed");
            }
        }
        if (!h_mate_row || bad_matching)
            GR_CHECK(hipMemsetAsync(d_mate_row, 0xFF, sizeof(int) * static_cast<size_t>(rows), stream), "BipartiteProblem memset failed");
        fresh = true;
        return retval;
    }

    // The contracted square part of the last BIPARTITE_MAXIMUM result, by count, scan and fill: once per result.
    hipError_t SquareGraph()
    {
        hipError_t retval = hipSuccess;
        if (square_k >= 0) return retval;
        const long long n1 = rows + 1ll;
        graphio::DeviceScratch<unsigned> flag, count;
        graphio::DeviceScratch<unsigned long long> sums;
        if ((retval = flag.Alloc(static_cast<size_t>(n1)))) return retval;
        if ((retval = count.Alloc(static_cast<size_t>(n1)))) return retval;
        if ((retval = sums.Alloc(static_cast<size_t>(graphio::ScanScratchWords(n1))))) return retval;
        const dim3 grid = GridFor(n1, 0), block(kThreads);
        hipLaunchKernelGGL(SquareFlagKernel, grid, block, 0, stream, d_row_part.p, static_cast<long long>(rows), flag.p);
        GR_CHECK(hipGetLastError(), "SquareFlagKernel launch failed");
        GR_CHECK(graphio::DeviceExclusiveScan<int>(flag.p, d_local.p, n1, sums.p, stream), "BipartiteProblem scan failed");
        int k = 0;
        GR_CHECK(hipMemcpyAsync(&k, d_local + rows, sizeof(int), hipMemcpyDeviceToHost, stream), "BipartiteProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "BipartiteProblem sync failed");
        if ((retval = sq_ro.Need(static_cast<size_t>(k) + 1))) return retval;
        if ((retval = sq_map.Need(static_cast<size_t>(k)))) return retval;
        hipLaunchKernelGGL(SquareRowsKernel<false>, grid, block, 0, stream, DeviceSides(), d_row_part.p, d_col_part.p, d_local.p, count.p, sq_map.p,
                           static_cast<const int *>(nullptr), static_cast<int *>(nullptr));
        GR_CHECK(hipGetLastError(), "SquareRowsKernel launch failed");
        GR_CHECK(graphio::DeviceExclusiveScan<int>(count.p, sq_ro.p, k + 1ll, sums.p, stream), "BipartiteProblem scan failed");
        int arcs = 0;
        GR_CHECK(hipMemcpyAsync(&arcs, sq_ro.p + k, sizeof(int), hipMemcpyDeviceToHost, stream), "BipartiteProblem read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "BipartiteProblem sync failed");
        if ((retval = sq_ci.Need(static_cast<size_t>(arcs)))) return retval;
        hipLaunchKernelGGL(SquareRowsKernel<true>, grid, block, 0, stream, DeviceSides(), d_row_part.p, d_col_part.p, d_local.p,
                           static_cast<unsigned *>(nullptr), static_cast<int *>(nullptr), sq_ro.p, sq_ci.p);
        GR_CHECK(hipGetLastError(), "SquareRowsKernel launch failed");
        GR_CHECK(hipStreamSynchronize(stream), "BipartiteProblem sync failed");  // (the scratch goes with this scope)
        square_k = k;
        square_arcs = arcs;
        return retval;
    }

    template <typename T>
    hipError_t Read(T *host, const T *device, size_t count)
    {
        if (!host || !count) return hipSuccess;
        return util::GRError(hipMemcpy(host, device, sizeof(T) * count, hipMemcpyDeviceToHost), "BipartiteProblem read failed", __FILE__, __LINE__);
    }
};

}  // namespace bipartite
}  // namespace app
}  // namespace gunrock
