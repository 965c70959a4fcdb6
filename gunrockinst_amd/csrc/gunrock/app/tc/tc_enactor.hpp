// app/tc/tc_enactor.hpp -- host side of triangle counting.
//
// One Enact: BinKernel sorts the non-empty out-rows into the three regimes of tc_functor.hpp (by length; `strategy` forces one),
// then at most one launch per regime; the row kernels take their list lengths from device memory, so nothing is read back
// until the one copy of the counters at the end.  INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/tc/tc_functor.hpp>
#include <gunrock/app/tc/tc_problem.hpp>

namespace gunrock {
namespace app {
namespace tc {

template <bool INSTRUMENT>
class TCEnactor : public EnactorBase {
   public:
    explicit TCEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}
    ~TCEnactor() override
    {
        if (ev[0]) hipEventDestroy(ev[0]);
        if (ev[1]) hipEventDestroy(ev[1]);
    }

    // options (grx_tc_set_option)
    int strategy = TC_AUTO;
    int lane_max_row = kLaneMaxRow;
    int lds_entries = kLdsEntries;

    // of the last Enact
    long long entries_probed = 0;
    long long launches = 0;
    long long regime_rows[3] = {0, 0, 0};  // rows the lane, LDS and global regimes took
    double kernel_ms = 0;                  // INSTRUMENT: summed kernel time

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, M = problem->oriented_edges;
        entries_probed = launches = 0;
        regime_rows[0] = regime_rows[1] = regime_rows[2] = 0;
        kernel_ms = 0;
        if (M <= 0) return retval;
        if (INSTRUMENT && !ev[0]) {
            GR_CHECK(hipEventCreate(&ev[0]), "TCEnactor hipEventCreate failed");
            GR_CHECK(hipEventCreate(&ev[1]), "TCEnactor hipEventCreate failed");
        }
        auto grid = [&](long long blocks, int cap) {
            if (blocks > cap) blocks = cap;
            if (blocks < 1) blocks = 1;
            return static_cast<int>(max_grid_size > 0 && max_grid_size < blocks ? max_grid_size : blocks);
        };
        auto begin = [&]() -> hipError_t {
            return INSTRUMENT ? util::GRError(hipEventRecord(ev[0], stream), "TCEnactor hipEventRecord failed", __FILE__, __LINE__) : hipSuccess;
        };
        auto end = [&]() -> hipError_t {
            ++launches;
            if (INSTRUMENT) {
                float ms = 0;
                GR_CHECK(hipEventRecord(ev[1], stream), "TCEnactor hipEventRecord failed");
                GR_CHECK(hipEventSynchronize(ev[1]), "TCEnactor hipEventSynchronize failed");
                GR_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]), "TCEnactor hipEventElapsedTime failed");
                kernel_ms += ms;
            }
            return hipSuccess;
        };

        const Oriented g = problem->DeviceGraph();
        const int longest = static_cast<int>(problem->max_out_row);
        const int budget = lds_entries < longest ? lds_entries : longest;  // entries staged at most (>= 1: M > 0)
        // the regimes that can have a row, from the longest and the shortest possible non-empty row
        const bool any_lane = RegimeOf(1, strategy, lane_max_row, budget) == TC_LANE;
        const bool any_lds = strategy != TC_LANE && strategy != TC_GLOBAL && (strategy == TC_LDS || longest > lane_max_row);
        const bool any_global = RegimeOf(longest, strategy, lane_max_row, budget) == TC_GLOBAL;

        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(int) * 4, stream), "TCEnactor memset failed");
        if ((retval = begin())) return retval;
        hipLaunchKernelGGL(BinKernel, dim3(grid((n + 255) / 256, 2048)), dim3(256), 0, stream, ds->d_oro, static_cast<int>(n), strategy, lane_max_row,
                           budget, ds->d_rows[0], ds->d_rows[1], ds->d_words);
        GR_CHECK(hipGetLastError(), "BinKernel launch failed");
        if ((retval = end())) return retval;

        if (any_lds) {
            if ((retval = begin())) return retval;
            hipLaunchKernelGGL((RowKernel<true>), dim3(grid(n, 4096)), dim3(kTcThreads), sizeof(int) * 2 * static_cast<size_t>(budget), stream, g,
                               ds->d_rows[0], ds->d_words, budget, ds->d_triangles, ds->d_counters);
            GR_CHECK(hipGetLastError(), "RowKernel<staged> launch failed");
            if ((retval = end())) return retval;
        }
        if (any_global) {
            if ((retval = begin())) return retval;
            hipLaunchKernelGGL((RowKernel<false>), dim3(grid(n, 4096)), dim3(kTcThreads), 0, stream, g, ds->d_rows[1], ds->d_words + 1, 0,
                               ds->d_triangles, ds->d_counters);
            GR_CHECK(hipGetLastError(), "RowKernel<global> launch failed");
            if ((retval = end())) return retval;
        }
        if (any_lane) {
            if ((retval = begin())) return retval;
            hipLaunchKernelGGL(LaneKernel, dim3(grid((M + kTcThreads - 1) / kTcThreads, 8192)), dim3(kTcThreads), 0, stream, g, M,
                               strategy == TC_LANE ? INT_MAX : lane_max_row, ds->d_triangles, ds->d_counters);
            GR_CHECK(hipGetLastError(), "LaneKernel launch failed");
            if ((retval = end())) return retval;
        }

        // the one read-back
        int words[4] = {0, 0, 0, 0};
        Count counters[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(words, ds->d_words, sizeof(words), hipMemcpyDeviceToHost, stream), "TCEnactor read-back failed");
        GR_CHECK(hipMemcpyAsync(counters, ds->d_counters, sizeof(counters), hipMemcpyDeviceToHost, stream), "TCEnactor read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "TCEnactor read-back sync failed");
        regime_rows[0] = words[2];
        regime_rows[1] = words[0];
        regime_rows[2] = words[1];
        entries_probed = static_cast<long long>(counters[1]);
        return retval;
    }

   private:
    hipEvent_t ev[2] = {nullptr, nullptr};
};

}  // namespace tc
}  // namespace app
}  // namespace gunrock
