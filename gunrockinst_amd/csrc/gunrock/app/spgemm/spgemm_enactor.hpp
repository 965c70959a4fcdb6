// app/spgemm/spgemm_enactor.hpp -- host side of the sparse product C = A B.
//
// One Enact, three passes, three read-backs.  WorkKernel (behind RowAbsKernel when B has values) leaves the work of every row, the four
// row lists and the bound; the first read-back brings their lengths, the largest w_i and the bound, which are held against int32 and
// `count_limit` before anything else runs (refused: kSpgemmTooLarge, kSpgemmOverflow).  The symbolic kernels of the regimes that have
// rows count the distinct columns; the second read-back is nnz(C), refused beyond INT_MAX before the offsets -- the first array of the
// result -- are written by the scan.  C grows on demand, the numeric kernels fill it, the last read-back brings the counters.  The
// host-side rules -- option ranges, the regimes, LDS bytes, the GLOBAL regime's slots, the refusals -- are SpgemmOptions and the
// __host__ __device__ functions of spgemm_functor.hpp, plain C++ that a host-only program can call.  INSTRUMENT times every kernel with
// HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/table_ladder.hpp>
#include <gunrock/app/spgemm/spgemm_functor.hpp>
#include <gunrock/app/spgemm/spgemm_problem.hpp>
#include <gunrock/graphio/device_csr.hpp>

namespace gunrock {
namespace app {
namespace spgemm {

constexpr int kSpgemmTooLarge = -4;  // GRX_SPGEMM_TOO_LARGE
constexpr int kSpgemmOverflow = -7;  // GRX_SPGEMM_OVERFLOW
constexpr double kCountLimit = 4611686018427387904.0;  // 2^62

// options (grx_spgemm_set_option) and what the host derives from them
struct SpgemmOptions {
    int right = SPGEMM_SELF;
    int strategy = SPGEMM_AUTO;
    int lane_max = kLaneMax;
    int pattern_only = 0;
    double count_limit = kCountLimit;
    ladder::TableOptions table;  // "table_slots", "block_slots", "scratch_mib"

    // 0: set, 1: unknown name, -1: a value out of range
    int Set(const char *name, double value)
    {
        if (!(value == value)) return -1;
        const long long v = Whole(value);
        if (!std::strcmp(name, "right")) {
            if (v < SPGEMM_SELF || v > SPGEMM_GIVEN) return -1;
            right = static_cast<int>(v);
        } else if (!std::strcmp(name, "strategy")) {
            if (v < SPGEMM_AUTO || v > SPGEMM_GLOBAL) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "lane_max")) {
            if (v < 0 || v > kLaneMax) return -1;
            lane_max = static_cast<int>(v);
        } else if (!std::strcmp(name, "pattern_only")) {
            if (v < 0 || v > 1) return -1;
            pattern_only = static_cast<int>(v);
        } else if (!std::strcmp(name, "count_limit")) {
            if (!(value >= 1.0 && value <= kCountLimit)) return -1;
            count_limit = value;
        } else {
            return table.Set(name, value);
        }
        return 0;
    }

    int RegimeOf(long long w) const { return Regime(w, strategy, lane_max, table.table_slots, table.block_slots); }
    // twelve bytes a slot with values, four without: not the eight of the shared options
    size_t SmallLdsBytes(bool values) const { return spgemm::SmallLdsBytes(table.table_slots, values); }
    size_t BlockLdsBytes(bool values) const { return spgemm::BlockLdsBytes(table.block_slots, values); }
    long long Slots(long long grid, long long cols) const { return GlobalSlots(grid, table.scratch_mib, cols); }
    bool Overflows(long long bound) const { return static_cast<double>(bound) >= count_limit; }
};

template <bool INSTRUMENT>
class SpgemmEnactor : public EnactorBase {
   public:
    explicit SpgemmEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    SpgemmOptions options;

    // of the last Enact (host: its launches, read-backs and summed kernel time)
    StepHost<INSTRUMENT> host{"SpgemmEnactor"};
    bool bad_shape = false;  // SELF on a non-square A, GIVEN without a right operand or with other rows than A's inner: nothing ran
    bool too_large = false;  // nnz(C) or the products of a row are beyond int32: no result was written
    bool overflow = false;   // the bound reached count_limit: no result was written
    double bound = 0;
    long long products = 0, max_products = 0, nnz = 0, probes = 0;
    long long regime_rows[4] = {0, 0, 0, 0}, regime_products[4] = {0, 0, 0, 0};  // LANE, WAVE, BLOCK, GLOBAL
    double regime_ms[4] = {0, 0, 0, 0};  // INSTRUMENT: the kernel time of each regime, both passes

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        hipStream_t stream = problem->stream;
        bad_shape = too_large = overflow = false;
        bound = 0;
        products = max_products = nnz = probes = 0;
        for (int r = 0; r < 4; ++r) regime_rows[r] = regime_products[r] = 0, regime_ms[r] = 0;
        if ((retval = host.Begin(0))) return retval;
        problem->nnz = -1;

        // the right operand
        const DeviceMat *right = &problem->a;
        if (options.right == SPGEMM_SELF) {
            bad_shape = problem->a.rows != problem->a.cols;
        } else if (options.right == SPGEMM_GIVEN) {
            right = &problem->given;
            bad_shape = !right->set || right->rows != problem->a.cols;
        } else if (!(retval = problem->NeedTransposed())) {
            right = &problem->transposed;
        }
        if (retval || bad_shape) return retval;

        const long long rows = problem->a.rows, cols = right->cols;
        const size_t n = static_cast<size_t>(rows);
        const bool values = !options.pattern_only;
        if ((retval = problem->offsets.Need(n + 1))) return retval;
        if (rows == 0) {
            GR_CHECK(hipMemsetAsync(problem->offsets.p, 0, sizeof(int), stream), "SpgemmEnactor memset failed");
            GR_CHECK(hipStreamSynchronize(stream), "SpgemmEnactor sync failed");
            return Finish(problem, 0, static_cast<int>(cols), values);
        }
        if ((retval = problem->work.Need(n))) return retval;
        if ((retval = problem->lists.Need(4 * n))) return retval;
        if ((retval = problem->counts.Need(n + 1))) return retval;
        if ((retval = problem->sums.Need(static_cast<size_t>(graphio::ScanScratchWords(rows + 1))))) return retval;
        GR_CHECK(hipMemsetAsync(problem->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "SpgemmEnactor memset failed");
        GR_CHECK(hipMemsetAsync(problem->counts.p, 0, sizeof(unsigned) * (n + 1), stream), "SpgemmEnactor memset failed");

        Ctx c;
        c.a = View(problem->a);
        c.b = View(*right);
        c.babs = nullptr;
        c.words = problem->d_words;
        c.work = problem->work.p;
        c.lists = problem->lists.p;
        c.strategy = options.strategy;
        c.lane_max = options.lane_max;
        c.table_slots = options.table.table_slots;
        c.block_slots = options.table.block_slots;

        // 1. the work
        if (c.b.val && c.b.rows > 0) {
            if ((retval = problem->babs.Need(static_cast<size_t>(c.b.rows)))) return retval;
            c.babs = problem->babs.p;
            if ((retval = host.Run(stream, [&]() {
                     hipLaunchKernelGGL(RowAbsKernel, dim3(CappedGrid((c.b.rows + 255ll) / 256, 2048, max_grid_size)), dim3(256), 0, stream, c.b,
                                        problem->babs.p);
                 })))
                return retval;
        }
        if ((retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL(WorkKernel, dim3(CappedGrid((rows + kThreads - 1) / kThreads, 4096, max_grid_size)), dim3(kThreads), 0, stream, c);
             })))
            return retval;
        unsigned long long words[W_COUNT];
        if ((retval = host.Read(words, problem->d_words, sizeof(words), stream))) return retval;
        products = static_cast<long long>(words[W_SUM]);
        max_products = static_cast<long long>(words[W_MAX]);
        bound = static_cast<double>(static_cast<long long>(words[W_BOUND]));
        for (int r = 0; r < 4; ++r) {
            regime_rows[r] = static_cast<long long>(words[W_LISTS + r]);
            regime_products[r] = static_cast<long long>(words[W_PRODUCTS + r]);
        }
        too_large = !Fits(0, max_products);
        overflow = options.Overflows(static_cast<long long>(words[W_BOUND]));
        if (too_large || overflow) return retval;

        // 2. the distinct columns of every row, their sum, the offsets
        Out o = {problem->counts.p, nullptr, nullptr, nullptr};
        if ((retval = Pass<false, false>(problem, c, o, cols, max_grid_size))) return retval;
        unsigned long long entries = 0;
        if ((retval = host.Read(&entries, problem->d_words + W_NNZ, sizeof(entries), stream))) return retval;
        nnz = static_cast<long long>(entries);
        too_large = !Fits(nnz, max_products);
        if (too_large) return retval;
        if ((retval = host.Run(stream, [&]() {
                 return graphio::DeviceExclusiveScan<int>(problem->counts.p, problem->offsets.p, rows + 1, problem->sums.p, stream);
             })))
            return retval;

        // 3. the entries
        if (nnz > 0) {
            if ((retval = problem->cols.Need(static_cast<size_t>(nnz)))) return retval;
            if (values && (retval = problem->vals.Need(static_cast<size_t>(nnz)))) return retval;
            o = Out{nullptr, problem->offsets.p, problem->cols.p, values ? problem->vals.p : nullptr};
            if (values) retval = Pass<true, true>(problem, c, o, cols, max_grid_size);
            else retval = Pass<true, false>(problem, c, o, cols, max_grid_size);
            if (retval) return retval;
        }
        if ((retval = host.Read(words, problem->d_words, sizeof(words), stream))) return retval;
        probes = static_cast<long long>(words[W_PROBES]);
        return Finish(problem, nnz, static_cast<int>(cols), values);
    }

   private:
    size_t lds_opted[3] = {0, 0, 0};  // per BlockKernel instantiation

    template <typename Problem>
    hipError_t Finish(Problem *problem, long long entries, int cols, bool values)
    {
        problem->nnz = entries;
        problem->result_cols = cols;
        problem->with_values = values;
        return hipSuccess;
    }

    // the kernels of the regimes that have rows, each over its list
    template <bool WRITE, bool VALUES, typename Problem>
    hipError_t Pass(Problem *problem, const Ctx &c, const Out &o, long long cols, int max_grid_size)
    {
        hipError_t retval = hipSuccess;
        hipStream_t stream = problem->stream;
        const long long lane = regime_rows[0], wave = regime_rows[1], block = regime_rows[2], global = regime_rows[3];
        double mark = host.kernel_ms;
        auto timed = [&](int r) {  // what has run since the last call was regime r's
            regime_ms[r] += host.kernel_ms - mark;
            mark = host.kernel_ms;
        };
        if (lane > 0 &&
            (retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL((LaneKernel<WRITE, VALUES>), dim3(CappedGrid((lane + kThreads - 1) / kThreads, 4096, max_grid_size)), dim3(kThreads), 0,
                                    stream, c, o);
             })))
            return retval;
        timed(0);
        if (wave > 0 &&
            (retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL((TableKernel<false, WRITE, VALUES>), dim3(CappedGrid((wave + kWaves - 1) / kWaves, 4096, max_grid_size)),
                                    dim3(kThreads), options.SmallLdsBytes(VALUES), stream, c, o);
             })))
            return retval;
        timed(1);
        if (block > 0) {  // (the LDS: asked for once per kernel, for its largest table)
            if ((retval = AllowLds(reinterpret_cast<const void *>(&TableKernel<true, WRITE, VALUES>), spgemm::BlockLdsBytes(kBlockSlots, VALUES),
                                   &lds_opted[WRITE + VALUES])))
                return retval;
            if ((retval = host.Run(stream, [&]() {
                     hipLaunchKernelGGL((TableKernel<true, WRITE, VALUES>), dim3(CappedGrid(block, 2048, max_grid_size)), dim3(kThreads),
                                        options.BlockLdsBytes(VALUES), stream, c, o);
                 })))
                return retval;
            timed(2);
        }
        if (global > 0) {
            const int blocks = static_cast<int>(options.Slots(CappedGrid(global, 1024, max_grid_size), cols));
            if ((retval = problem->scratch.NeedZeroed(static_cast<size_t>(blocks) * static_cast<size_t>(SlotWords(cols)), stream))) return retval;
            if ((retval = host.Run(stream, [&]() {
                     hipLaunchKernelGGL((GlobalKernel<WRITE, VALUES>), dim3(blocks), dim3(kThreads), 0, stream, c, o, problem->scratch.p);
                 })))
                return retval;
            timed(3);
        }
        return retval;
    }
};

}  // namespace spgemm
}  // namespace app
}  // namespace gunrock
