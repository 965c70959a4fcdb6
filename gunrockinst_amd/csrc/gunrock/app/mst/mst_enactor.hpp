// app/mst/mst_enactor.hpp -- host loop of the Borůvka minimum spanning forest.
//
// Stands for the reference's MSTEnactor (gunrock/app/mst/mst_enactor.cuh:48-1260):
//   template <bool INSTRUMENT> class MSTEnactor : EnactorBase;  Enact<MSTProblem>(problem, max_grid_size)   (:1198)
//   GetStatistics(total_queued, search_depth, avg_duty)                                                      (:166)
// Schedule (mst_functor.hpp has the kernels):
//   round 1, mirrored input with equal mirror weights: RowMin -> Canonical -> Hook -> flatten, then the first list is filtered out of the
//            CSR (only the f < t copy of every edge);  any other input: the first list is every non-loop entry
//   round r: best = none -> ListMin -> Hook -> flatten -> filter the list (relabel, drop entries inside one component,
//            compact) -- until the list is empty, i.e. no component has an outgoing edge.
// One read-back per pointer-jumping sweep and one per filter (the new list length); nothing else leaves the GPU.
// The reference instead sorts and renumbers the whole contracted graph every round (mst_enactor.cuh:564-640) and needs a
// connected input.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/mst/mst_functor.hpp>
#include <gunrock/app/mst/mst_problem.hpp>
#include <gunrock/graphio/device_csr.hpp>

namespace gunrock {
namespace app {
namespace mst {

template <bool INSTRUMENT>
class MSTEnactor : public EnactorBase {
   public:
    explicit MSTEnactor(bool DEBUG = false) : EnactorBase(EDGE_FRONTIERS, DEBUG) {}
    ~MSTEnactor() override
    {
        if (ev_round[0]) hipEventDestroy(ev_round[0]);
        if (ev_round[1]) hipEventDestroy(ev_round[1]);
    }

    struct Round {
        long long entries;  // entries the round's minimum step read (CSR entries in the row round)
        double ms;          // INSTRUMENT: HIP-event time of the whole round, filter included
    };
    long long rounds = 0;
    long long edges_scanned = 0;  // sum of Round::entries
    long long launches = 0;
    double kernel_ms = 0;         // INSTRUMENT: sum of Round::ms plus the first list's filter
    std::vector<Round> trace;

    void GetStatistics(long long &total_queued, long long &search_depth, double &avg_duty)
    {
        total_queued = edges_scanned;
        search_depth = rounds;
        avg_duty = 0.0;
    }

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        GraphSlice<int, int, int> *gs = problem->graph_slices[0];
        hipStream_t stream = gs->stream;
        const long long n = problem->nodes, m = problem->edges;
        rounds = edges_scanned = launches = 0;
        kernel_ms = 0;
        trace.clear();
        if (n <= 0 || m <= 0) return retval;
        if (INSTRUMENT && !ev_round[0]) {
            GR_CHECK(hipEventCreate(&ev_round[0]), "MSTEnactor hipEventCreate failed");
            GR_CHECK(hipEventCreate(&ev_round[1]), "MSTEnactor hipEventCreate failed");
        }
        auto grid = [&](long long work) {
            const int g = graphio::PairGrid(work);
            return max_grid_size > 0 && max_grid_size < g ? max_grid_size : g;
        };
        auto launched = [&](const char *what) -> hipError_t {
            ++launches;
            return util::GRError(hipGetLastError(), what, __FILE__, __LINE__);
        };
        auto begin = [&]() -> hipError_t { return INSTRUMENT ? util::GRError(hipEventRecord(ev_round[0], stream), "MSTEnactor hipEventRecord failed", __FILE__, __LINE__) : hipSuccess; };
        auto end = [&](long long entries) -> hipError_t {
            float ms = 0;
            if (INSTRUMENT) {
                GR_CHECK(hipEventRecord(ev_round[1], stream), "MSTEnactor hipEventRecord failed");
                GR_CHECK(hipEventSynchronize(ev_round[1]), "MSTEnactor hipEventSynchronize failed");
                GR_CHECK(hipEventElapsedTime(&ms, ev_round[0], ev_round[1]), "MSTEnactor hipEventElapsedTime failed");
                kernel_ms += ms;
            }
            if (entries >= 0) {
                trace.push_back({entries, ms});
                edges_scanned += entries;
                ++rounds;
            }
            return hipSuccess;
        };
        // hook, then pointer jumping until no pointer moves
        auto hook_and_flatten = [&]() -> hipError_t {
            hipLaunchKernelGGL(HookKernel, dim3(grid(n)), dim3(256), 0, stream, ds->d_parent[ds->cur], ds->d_parent[ds->cur ^ 1], ds->d_best,
                               ds->d_froms, gs->d_column_indices, n, ds->d_selected, ds->d_totals);
            if ((retval = launched("HookKernel launch failed"))) return retval;
            ds->cur ^= 1;
            for (;;) {
                GR_CHECK(hipMemsetAsync(ds->d_flag, 0, sizeof(int), stream), "MSTEnactor memset failed");
                hipLaunchKernelGGL(JumpKernel, dim3(grid(n)), dim3(256), 0, stream, ds->d_parent[ds->cur], n, ds->d_flag);
                if ((retval = launched("JumpKernel launch failed"))) return retval;
                int changed = 0;
                if ((retval = problem->ReadWord(ds->d_flag, changed, stream))) return retval;
                if (!changed) break;
            }
            return hipSuccess;
        };
        // new length of the list after a filter (flags[len] = 0, so the scan's last element is the total)
        auto scan = [&](long long len, long long &kept) -> hipError_t {
            GR_CHECK(graphio::DeviceExclusiveScan<unsigned>(ds->d_flags, ds->d_pos, len + 1, ds->d_scan_sums, stream), "MSTEnactor scan failed");
            launches += 3;
            int total = 0;
            if ((retval = problem->ReadWord(reinterpret_cast<const int *>(ds->d_pos + len), total, stream))) return retval;
            kept = static_cast<unsigned>(total);
            return hipSuccess;
        };

        // ---- round 1 by rows (mirrored input with equal mirror weights) ----
        if (problem->mirrored) {
            if ((retval = begin())) return retval;
            util::Memset(ds->d_best.p, kNoEdge, n, stream);
            if ((retval = launched("MemsetKernel launch failed"))) return retval;
            hipLaunchKernelGGL(RowMinKernel, dim3(grid(m)), dim3(256), 0, stream, ds->d_froms, gs->d_column_indices, gs->d_edge_values, m,
                               ds->d_best);
            if ((retval = launched("RowMinKernel launch failed"))) return retval;
            hipLaunchKernelGGL(CanonicalKernel, dim3(grid(n)), dim3(256), 0, stream, gs->d_row_offsets, gs->d_column_indices, n, ds->d_best);
            if ((retval = launched("CanonicalKernel launch failed"))) return retval;
            if ((retval = hook_and_flatten())) return retval;
            if ((retval = end(m))) return retval;
        }

        // ---- the first list, straight from the CSR ----
        if ((retval = begin())) return retval;
        long long len = 0;
        int b = 0;
        hipLaunchKernelGGL(FlagCsrKernel, dim3(grid(m + 1)), dim3(256), 0, stream, ds->d_froms, gs->d_column_indices, ds->d_parent[ds->cur],
                           m, problem->mirrored, ds->d_flags);
        if ((retval = launched("FlagCsrKernel launch failed"))) return retval;
        if ((retval = scan(m, len))) return retval;
        if (len > problem->list_capacity) return util::GRError(hipErrorInvalidValue, "MSTEnactor list overflow", __FILE__, __LINE__);
        hipLaunchKernelGGL(ScatterCsrKernel, dim3(grid(m)), dim3(256), 0, stream, ds->d_froms, gs->d_column_indices, gs->d_edge_values,
                           ds->d_parent[ds->cur], ds->d_flags, ds->d_pos, m, ds->d_cu[b], ds->d_cv[b], ds->d_key[b]);
        if ((retval = launched("ScatterCsrKernel launch failed"))) return retval;
        if ((retval = end(-1))) return retval;

        // ---- Borůvka rounds over the shrinking list ----
        while (len > 0) {
            if ((retval = begin())) return retval;
            util::Memset(ds->d_best.p, kNoEdge, n, stream);
            if ((retval = launched("MemsetKernel launch failed"))) return retval;
            hipLaunchKernelGGL(ListMinKernel, dim3(grid(len)), dim3(256), 0, stream, ds->d_cu[b], ds->d_cv[b], ds->d_key[b], len, ds->d_best);
            if ((retval = launched("ListMinKernel launch failed"))) return retval;
            if ((retval = hook_and_flatten())) return retval;
            const long long entries = len;
            hipLaunchKernelGGL(FlagListKernel, dim3(grid(len + 1)), dim3(256), 0, stream, ds->d_cu[b], ds->d_cv[b], ds->d_parent[ds->cur], len,
                               ds->d_flags);
            if ((retval = launched("FlagListKernel launch failed"))) return retval;
            long long kept = 0;
            if ((retval = scan(len, kept))) return retval;
            if (kept > 0) {
                hipLaunchKernelGGL(ScatterListKernel, dim3(grid(len)), dim3(256), 0, stream, ds->d_cu[b], ds->d_cv[b], ds->d_key[b], ds->d_flags,
                                   ds->d_pos, len, ds->d_cu[b ^ 1], ds->d_cv[b ^ 1], ds->d_key[b ^ 1]);
                if ((retval = launched("ScatterListKernel launch failed"))) return retval;
                b ^= 1;
            }
            if (kept >= len) return util::GRError(hipErrorUnknown, "MSTEnactor: a round removed no entry", __FILE__, __LINE__);
            len = kept;
            if ((retval = end(entries))) return retval;
        }
        return retval;
    }

   private:
    hipEvent_t ev_round[2] = {nullptr, nullptr};
};

}  // namespace mst
}  // namespace app
}  // namespace gunrock
