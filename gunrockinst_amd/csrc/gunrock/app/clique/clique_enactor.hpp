// app/clique/clique_enactor.hpp -- host side of k-clique counting.
//
// One Enact: the bound of this k (the build left it on the host) is held against `count_limit` before any kernel; BinKernel sorts
// the out-rows of at least k - 1 entries into the two regimes of clique_functor.hpp (by length; `strategy` forces one), then at most one launch per
// regime; both take their list lengths from device memory, so nothing is read back until the one copy of the counters at the end.
// INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/clique/clique_functor.hpp>
#include <gunrock/app/clique/clique_problem.hpp>

namespace gunrock {
namespace app {
namespace clique {

constexpr int kCliqueOverflow = -7;  // GRX_CLIQUE_OVERFLOW
constexpr double kCountLimit = 4611686018427387904.0;  // 2^62

template <bool INSTRUMENT>
class CliqueEnactor : public EnactorBase {
   public:
    explicit CliqueEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    // options (grx_clique_set_option)
    int strategy = CLIQUE_AUTO;
    int bitmap_rows = kBitmapRows;
    double count_limit = kCountLimit;

    // of the last Enact (host: its launches and summed kernel time)
    StepHost<INSTRUMENT> host{"CliqueEnactor"};
    bool refused = false;  // the bound reached count_limit: nothing ran
    double bound = 0;
    long long bit_ands = 0, list_lookups = 0;
    long long regime_rows[2] = {0, 0}, regime_edges[2] = {0, 0};  // the bitmap and the list regime

    // k in 3 .. 6 (the caller has checked)
    template <typename Problem>
    hipError_t Enact(Problem *problem, int k, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, M = problem->oriented_edges;
        bit_ands = list_lookups = 0;
        regime_rows[0] = regime_rows[1] = regime_edges[0] = regime_edges[1] = 0;
        if ((retval = host.Begin(0))) return retval;
        bound = problem->bound[k - kMinK];
        refused = bound >= count_limit;
        if (refused) return retval;
        if (problem->dirty && (retval = problem->Reset())) return retval;
        if (M <= 0) return retval;
        problem->dirty = true;

        const Oriented g = problem->DeviceGraph();
        const int longest = static_cast<int>(problem->max_out_row);  // >= 1: M > 0
        const int limit = strategy == CLIQUE_BITMAP ? kBitmapRowsMax : bitmap_rows;
        const int cap = limit < longest ? limit : longest;  // the longest row the bitmap kernel can meet
        const bool any_row = longest >= k - 1;              // BinKernel lists no shorter row: it holds no clique's other members
        const bool any_bitmap = any_row && strategy != CLIQUE_LIST;
        const bool any_list = any_row && RegimeOf(longest, strategy, bitmap_rows) == CLIQUE_LIST;

        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(int) * 4, stream), "CliqueEnactor memset failed");
        if ((retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL(BinKernel, dim3(CappedGrid((n + 255) / 256, 2048, max_grid_size)), dim3(256), 0, stream, ds->d_oro, static_cast<int>(n), k - 1, strategy,
                                    bitmap_rows, ds->d_bitmap_rows, ds->d_list_edges, ds->d_words);
             })))
            return retval;

        if (any_bitmap) {
            const size_t lds = BitmapLdsBytes(cap);
            const int blocks = CappedGrid(n, 4096, max_grid_size);
            if ((retval = host.Run(stream, [&]() {  // (an error of the LDS opt-in ends the Run)
                     switch (k) {
                         case 3: return LaunchBitmap<3>(blocks, lds, stream, g, ds, cap);
                         case 4: return LaunchBitmap<4>(blocks, lds, stream, g, ds, cap);
                         case 5: return LaunchBitmap<5>(blocks, lds, stream, g, ds, cap);
                         default: return LaunchBitmap<6>(blocks, lds, stream, g, ds, cap);
                     }
                 })))
                return retval;
        }
        if (any_list) {
            const int blocks = CappedGrid(M, 4096, max_grid_size);
            const size_t need = static_cast<size_t>(blocks) * static_cast<size_t>(k - 2) * static_cast<size_t>(longest);
            if ((retval = ds->slabs.Need(need))) return retval;
            if ((retval = host.Run(stream, [&]() {
                     switch (k) {
                         case 3: LaunchList<3>(blocks, stream, g, ds, longest); break;
                         case 4: LaunchList<4>(blocks, stream, g, ds, longest); break;
                         case 5: LaunchList<5>(blocks, stream, g, ds, longest); break;
                         default: LaunchList<6>(blocks, stream, g, ds, longest); break;
                     }
                 })))
                return retval;
        }

        // the one read-back
        int words[4] = {0, 0, 0, 0};
        Count counters[3] = {0, 0, 0};
        if ((retval = host.Copy(words, ds->d_words, sizeof(words), stream))) return retval;
        if ((retval = host.Read(counters, ds->d_counters, sizeof(counters), stream))) return retval;
        regime_rows[0] = words[0];
        regime_rows[1] = words[2];
        regime_edges[0] = words[3];
        regime_edges[1] = words[1];
        bit_ands = static_cast<long long>(counters[1]);
        list_lookups = static_cast<long long>(counters[2]);
        return retval;
    }

   private:
    size_t lds_opted[kMaxK + 1] = {0, 0, 0, 0, 0, 0, 0};  // the dynamic LDS BitmapKernel<K> has been allowed

    template <int K, typename DataSlice>
    hipError_t LaunchBitmap(int blocks, size_t lds, hipStream_t stream, const Oriented &g, DataSlice *ds, int cap)
    {
        hipError_t retval = hipSuccess;
        if (lds > 64 * 1024 && (retval = AllowLds(reinterpret_cast<const void *>(&BitmapKernel<K>), lds, &lds_opted[K]))) return retval;
        hipLaunchKernelGGL((BitmapKernel<K>), dim3(blocks), dim3(kBitmapThreads), lds, stream, g, ds->d_bitmap_rows, ds->d_words, cap, ds->d_cliques,
                           ds->d_counters);
        GR_CHECK(hipGetLastError(), "BitmapKernel launch failed");
        return retval;
    }

    template <int K, typename DataSlice>
    void LaunchList(int blocks, hipStream_t stream, const Oriented &g, DataSlice *ds, int longest)
    {
        hipLaunchKernelGGL((ListKernel<K>), dim3(blocks), dim3(kListThreads), 0, stream, g, ds->d_list_edges, ds->d_words + 1, ds->slabs.p, longest,
                           ds->d_cliques, ds->d_counters);
    }
};

}  // namespace clique
}  // namespace app
}  // namespace gunrock
