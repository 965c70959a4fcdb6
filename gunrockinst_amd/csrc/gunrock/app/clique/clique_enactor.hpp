// app/clique/clique_enactor.hpp -- host side of k-clique counting.
//
// One Enact: the bound of this k (the build left it on the host) is held against `count_limit` before any kernel; BinKernel sorts
// the out-rows of at least k - 1 entries into the two regimes of clique_functor.hpp (by length; `strategy` forces one), then at most one launch per
// regime; both take their list lengths from device memory, so nothing is read back until the one copy of the counters at the end.
// INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/app/enactor_base.hpp>
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
    ~CliqueEnactor() override
    {
        if (ev[0]) hipEventDestroy(ev[0]);
        if (ev[1]) hipEventDestroy(ev[1]);
    }

    // options (grx_clique_set_option)
    int strategy = CLIQUE_AUTO;
    int bitmap_rows = kBitmapRows;
    double count_limit = kCountLimit;

    // of the last Enact
    bool refused = false;  // the bound reached count_limit: nothing ran
    double bound = 0;
    long long bit_ands = 0, list_lookups = 0, launches = 0;
    long long regime_rows[2] = {0, 0}, regime_edges[2] = {0, 0};  // the bitmap and the list regime
    double kernel_ms = 0;                                         // INSTRUMENT: summed kernel time

    // k in 3 .. 6 (the caller has checked)
    template <typename Problem>
    hipError_t Enact(Problem *problem, int k, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, M = problem->oriented_edges;
        bit_ands = list_lookups = launches = 0;
        regime_rows[0] = regime_rows[1] = regime_edges[0] = regime_edges[1] = 0;
        kernel_ms = 0;
        bound = problem->bound[k - kMinK];
        refused = bound >= count_limit;
        if (refused) return retval;
        if (problem->dirty && (retval = problem->Reset())) return retval;
        if (M <= 0) return retval;
        problem->dirty = true;
        if (INSTRUMENT && !ev[0]) {
            GR_CHECK(hipEventCreate(&ev[0]), "CliqueEnactor hipEventCreate failed");
            GR_CHECK(hipEventCreate(&ev[1]), "CliqueEnactor hipEventCreate failed");
        }
        auto grid = [&](long long blocks, int cap) {
            if (blocks > cap) blocks = cap;
            if (blocks < 1) blocks = 1;
            return static_cast<int>(max_grid_size > 0 && max_grid_size < blocks ? max_grid_size : blocks);
        };
        auto begin = [&]() -> hipError_t {
            return INSTRUMENT ? util::GRError(hipEventRecord(ev[0], stream), "CliqueEnactor hipEventRecord failed", __FILE__, __LINE__) : hipSuccess;
        };
        auto end = [&]() -> hipError_t {
            ++launches;
            if (INSTRUMENT) {
                float ms = 0;
                GR_CHECK(hipEventRecord(ev[1], stream), "CliqueEnactor hipEventRecord failed");
                GR_CHECK(hipEventSynchronize(ev[1]), "CliqueEnactor hipEventSynchronize failed");
                GR_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]), "CliqueEnactor hipEventElapsedTime failed");
                kernel_ms += ms;
            }
            return hipSuccess;
        };

        const Oriented g = problem->DeviceGraph();
        const int longest = static_cast<int>(problem->max_out_row);  // >= 1: M > 0
        const int limit = strategy == CLIQUE_BITMAP ? kBitmapRowsMax : bitmap_rows;
        const int cap = limit < longest ? limit : longest;  // the longest row the bitmap kernel can meet
        const bool any_row = longest >= k - 1;              // BinKernel lists no shorter row: it holds no clique's other members
        const bool any_bitmap = any_row && strategy != CLIQUE_LIST;
        const bool any_list = any_row && RegimeOf(longest, strategy, bitmap_rows) == CLIQUE_LIST;

        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(int) * 4, stream), "CliqueEnactor memset failed");
        if ((retval = begin())) return retval;
        hipLaunchKernelGGL(BinKernel, dim3(grid((n + 255) / 256, 2048)), dim3(256), 0, stream, ds->d_oro, static_cast<int>(n), k - 1, strategy, bitmap_rows,
                           ds->d_bitmap_rows, ds->d_list_edges, ds->d_words);
        GR_CHECK(hipGetLastError(), "BinKernel launch failed");
        if ((retval = end())) return retval;

        if (any_bitmap) {
            const size_t lds = BitmapLdsBytes(cap);
            const int blocks = grid(n, 4096);
            if ((retval = begin())) return retval;
            switch (k) {
                case 3: retval = LaunchBitmap<3>(blocks, lds, stream, g, ds, cap); break;
                case 4: retval = LaunchBitmap<4>(blocks, lds, stream, g, ds, cap); break;
                case 5: retval = LaunchBitmap<5>(blocks, lds, stream, g, ds, cap); break;
                default: retval = LaunchBitmap<6>(blocks, lds, stream, g, ds, cap); break;
            }
            if (retval) return retval;
            if ((retval = end())) return retval;
        }
        if (any_list) {
            const int blocks = grid(M, 4096);
            const size_t need = static_cast<size_t>(blocks) * static_cast<size_t>(k - 2) * static_cast<size_t>(longest);
            if (need > ds->slab_ints) {
                if (ds->d_slabs) GR_CHECK(hipFree(ds->d_slabs), "CliqueEnactor hipFree failed");
                ds->d_slabs = nullptr;
                ds->slab_ints = 0;
                GR_CHECK(hipMalloc(&ds->d_slabs, sizeof(int) * need), "CliqueEnactor hipMalloc d_slabs failed");
                ds->slab_ints = need;
            }
            if ((retval = begin())) return retval;
            switch (k) {
                case 3: LaunchList<3>(blocks, stream, g, ds, longest); break;
                case 4: LaunchList<4>(blocks, stream, g, ds, longest); break;
                case 5: LaunchList<5>(blocks, stream, g, ds, longest); break;
                default: LaunchList<6>(blocks, stream, g, ds, longest); break;
            }
            GR_CHECK(hipGetLastError(), "ListKernel launch failed");
            if ((retval = end())) return retval;
        }

        // the one read-back
        int words[4] = {0, 0, 0, 0};
        Count counters[3] = {0, 0, 0};
        GR_CHECK(hipMemcpyAsync(words, ds->d_words, sizeof(words), hipMemcpyDeviceToHost, stream), "CliqueEnactor read-back failed");
        GR_CHECK(hipMemcpyAsync(counters, ds->d_counters, sizeof(counters), hipMemcpyDeviceToHost, stream), "CliqueEnactor read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "CliqueEnactor read-back sync failed");
        regime_rows[0] = words[0];
        regime_rows[1] = words[2];
        regime_edges[0] = words[3];
        regime_edges[1] = words[1];
        bit_ands = static_cast<long long>(counters[1]);
        list_lookups = static_cast<long long>(counters[2]);
        return retval;
    }

   private:
    hipEvent_t ev[2] = {nullptr, nullptr};
    size_t lds_opted[kMaxK + 1] = {0, 0, 0, 0, 0, 0, 0};  // the dynamic LDS BitmapKernel<K> has been allowed

    template <int K, typename DataSlice>
    hipError_t LaunchBitmap(int blocks, size_t lds, hipStream_t stream, const Oriented &g, DataSlice *ds, int cap)
    {
        hipError_t retval = hipSuccess;
        if (lds > 64 * 1024 && lds > lds_opted[K]) {  // beyond the 64 KiB a launch gets unasked
            GR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&BitmapKernel<K>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         static_cast<int>(lds)),
                     "CliqueEnactor hipFuncSetAttribute failed");
            lds_opted[K] = lds;
        }
        hipLaunchKernelGGL((BitmapKernel<K>), dim3(blocks), dim3(kBitmapThreads), lds, stream, g, ds->d_bitmap_rows, ds->d_words, cap, ds->d_cliques,
                           ds->d_counters);
        GR_CHECK(hipGetLastError(), "BitmapKernel launch failed");
        return retval;
    }

    template <int K, typename DataSlice>
    void LaunchList(int blocks, hipStream_t stream, const Oriented &g, DataSlice *ds, int longest)
    {
        hipLaunchKernelGGL((ListKernel<K>), dim3(blocks), dim3(kListThreads), 0, stream, g, ds->d_list_edges, ds->d_words + 1, ds->d_slabs, longest,
                           ds->d_cliques, ds->d_counters);
    }
};

}  // namespace clique
}  // namespace app
}  // namespace gunrock
