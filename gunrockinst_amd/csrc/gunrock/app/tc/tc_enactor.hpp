// app/tc/tc_enactor.hpp -- host side of triangle counting.
//
// One Enact: BinKernel sorts the non-empty out-rows into the three regimes of tc_functor.hpp (by length; `strategy` forces one),
// then at most one launch per regime; the row kernels take their list lengths from device memory, so nothing is read back
// until the one copy of the counters at the end.  INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/tc/tc_functor.hpp>
#include <gunrock/app/tc/tc_problem.hpp>

namespace gunrock {
namespace app {
namespace tc {

template <bool INSTRUMENT>
class TCEnactor : public EnactorBase {
   public:
    explicit TCEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    // options (grx_tc_set_option)
    int strategy = TC_AUTO;
    int lane_max_row = kLaneMaxRow;
    int lds_entries = kLdsEntries;

    // of the last Enact (host: its launches and summed kernel time)
    StepHost<INSTRUMENT> host{"TCEnactor"};
    long long entries_probed = 0;
    long long regime_rows[3] = {0, 0, 0};  // rows the lane, LDS and global regimes took

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, M = problem->oriented_edges;
        entries_probed = 0;
        regime_rows[0] = regime_rows[1] = regime_rows[2] = 0;
        if ((retval = host.Begin(0))) return retval;
        if (M <= 0) return retval;
        const Oriented g = problem->DeviceGraph();
        const int longest = static_cast<int>(problem->max_out_row);
        const int budget = lds_entries < longest ? lds_entries : longest;  // entries staged at most (>= 1: M > 0)
        // the regimes that can have a row, from the longest and the shortest possible non-empty row
        const bool any_lane = RegimeOf(1, strategy, lane_max_row, budget) == TC_LANE;
        const bool any_lds = strategy != TC_LANE && strategy != TC_GLOBAL && (strategy == TC_LDS || longest > lane_max_row);
        const bool any_global = RegimeOf(longest, strategy, lane_max_row, budget) == TC_GLOBAL;

        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(int) * 4, stream), "TCEnactor memset failed");
        if ((retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL(BinKernel, dim3(CappedGrid((n + 255) / 256, 2048, max_grid_size)), dim3(256), 0, stream, ds->d_oro,
                                    static_cast<int>(n), strategy, lane_max_row, budget, ds->d_rows[0], ds->d_rows[1], ds->d_words);
             })))
            return retval;

        if (any_lds && (retval = host.Run(stream, [&]() {
                            hipLaunchKernelGGL((RowKernel<true>), dim3(CappedGrid(n, 4096, max_grid_size)), dim3(kTcThreads),
                                               sizeof(int) * 2 * static_cast<size_t>(budget), stream, g, ds->d_rows[0], ds->d_words, budget,
                                               ds->d_triangles, ds->d_counters);
                        })))
            return retval;
        if (any_global && (retval = host.Run(stream, [&]() {
                               hipLaunchKernelGGL((RowKernel<false>), dim3(CappedGrid(n, 4096, max_grid_size)), dim3(kTcThreads), 0, stream, g,
                                                  ds->d_rows[1], ds->d_words + 1, 0, ds->d_triangles, ds->d_counters);
                           })))
            return retval;
        if (any_lane && (retval = host.Run(stream, [&]() {
                             hipLaunchKernelGGL(LaneKernel, dim3(CappedGrid((M + kTcThreads - 1) / kTcThreads, 8192, max_grid_size)), dim3(kTcThreads), 0,
                                                stream, g, M, strategy == TC_LANE ? INT_MAX : lane_max_row, ds->d_triangles, ds->d_counters);
                         })))
            return retval;

        // the one read-back
        int words[4] = {0, 0, 0, 0};
        Count counters[2] = {0, 0};
        if ((retval = host.Copy(words, ds->d_words, sizeof(words), stream))) return retval;
        if ((retval = host.Read(counters, ds->d_counters, sizeof(counters), stream))) return retval;
        regime_rows[0] = words[2];
        regime_rows[1] = words[0];
        regime_rows[2] = words[1];
        entries_probed = static_cast<long long>(counters[1]);
        return retval;
    }
};

}  // namespace tc
}  // namespace app
}  // namespace gunrock
