// app/mis/mis_enactor.hpp -- host loop of the maximal independent set / greedy colourings.
//
// Stands for the reference's MISEnactor (gunrock/app/mis/mis_enactor.cuh:40-440):
//   template <bool INSTRUMENT> class MISEnactor : EnactorBase;  EnactMIS / Enact<MISProblem>(problem, max_grid_size)   (:170-440)
//   GetStatistics(total_queued, avg_duty)                                                                               (:140-160)
// The reference runs a MAX-reducing advance and a filter per iteration and stops after max_iter = 20 of them with the rest
// at -1 (:234-363, tests/mis/test_mis.cu:296).  Here (mis_functor.hpp has the kernels):
//   round r: one SweepKernel over the worklist of undecided vertices (round 1: every vertex); survivors form the next list,
//            its length is the one word read back;
//   tail:    when the list is short (<= kTailVertices), or a sweep decided less than a sixteenth of it (a long
//            dependency chain), the list is sorted by descending key (graphio::DeviceKeySort; not needed for one window) and cut
//            into windows of kTailVertices.  All of H(v) then lies in v's window or an earlier one, so TailKernel can finish a
//            window on its own: up to kTailSweeps sweeps in one launch, one vertex per thread, a blocked vertex polling only its
//            blocking neighbour.  A pass launches a few windows from the first unfinished one back to back and reads the
//            counts back once; a window behind an unfinished one only counts.  A pass always decides at least the undecided vertex of the
//            largest key, so the loop ends.
// use_tail = false (grx_mis_set_tail) keeps one launch per round to the end (measurements).
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/mis/mis_functor.hpp>
#include <gunrock/app/mis/mis_problem.hpp>

namespace gunrock {
namespace app {
namespace mis {

constexpr long long kTailVertices = 32768;  // a worklist this short goes to the device-side loop; the window of that loop
constexpr int kTailSweeps = 1024;           // bound of that loop per launch

template <bool INSTRUMENT>
class MISEnactor : public EnactorBase {
   public:
    explicit MISEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}
    ~MISEnactor() override
    {
        if (ev_round[0]) hipEventDestroy(ev_round[0]);
        if (ev_round[1]) hipEventDestroy(ev_round[1]);
    }

    struct Round {
        long long entries;  // vertices on the round's worklist
        double ms;          // INSTRUMENT: HIP-event time of the round
    };
    long long rounds = 0;        // host-visible sweeps: SweepKernel launches + tail passes (each ends in one read-back)
    long long tail_sweeps = 0;   // sweeps made on the device inside the tail launches
    long long entries_read = 0;  // row entries walked by all sweeps (a colouring's cursor passes every entry once per window)
    long long polls = 0;         // a blocked vertex asking its blocking entry again: one entry and one state each
    long long launches = 0;
    bool use_tail = true;        // false: one launch and one read-back per round to the end (grx_mis_set_tail; measurements)
    double kernel_ms = 0;        // INSTRUMENT: sum of Round::ms plus sort_ms
    double sort_ms = 0;          // INSTRUMENT: ordering the tail's list
    std::vector<Round> trace;

    void GetStatistics(long long &total_queued, long long &search_depth, double &avg_duty)
    {
        total_queued = entries_read;
        search_depth = rounds;
        avg_duty = 0.0;
    }

    template <typename Problem>
    hipError_t Enact(Problem *problem, int mode, int max_grid_size = 0)
    {
        if (mode < MIS_SET || mode > MIS_COLOR_FIRST_FIT) return util::GRError(hipErrorInvalidValue, "MISEnactor: unknown mode", __FILE__, __LINE__);
        const bool hashed = problem->data_slices[0]->d_priorities == nullptr;
        problem->mode = mode;
        switch (mode * 2 + (hashed ? 1 : 0)) {
            case 0: return Run<MIS_SET, false>(problem, max_grid_size);
            case 1: return Run<MIS_SET, true>(problem, max_grid_size);
            case 2: return Run<MIS_COLOR_ROUNDS, false>(problem, max_grid_size);
            case 3: return Run<MIS_COLOR_ROUNDS, true>(problem, max_grid_size);
            case 4: return Run<MIS_COLOR_FIRST_FIT, false>(problem, max_grid_size);
            default: return Run<MIS_COLOR_FIRST_FIT, true>(problem, max_grid_size);
        }
    }

   private:
    template <int MODE, bool HASHED, typename Problem>
    hipError_t Run(Problem *problem, int max_grid_size)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes;
        rounds = tail_sweeps = entries_read = polls = launches = 0;
        kernel_ms = sort_ms = 0;
        trace.clear();
        if (n <= 0) return retval;
        if (INSTRUMENT && !ev_round[0]) {
            GR_CHECK(hipEventCreate(&ev_round[0]), "MISEnactor hipEventCreate failed");
            GR_CHECK(hipEventCreate(&ev_round[1]), "MISEnactor hipEventCreate failed");
        }
        const Graph g = problem->DeviceGraph();
        const Keys k = problem->DeviceKeys();
        const State st = problem->DeviceState();
        auto grid = [&](long long work, int cap) {
            int blocks = graphio::PairGrid(work);
            if (blocks > cap) blocks = cap;
            return max_grid_size > 0 && max_grid_size < blocks ? max_grid_size : blocks;
        };
        auto begin = [&]() -> hipError_t {
            return INSTRUMENT ? util::GRError(hipEventRecord(ev_round[0], stream), "MISEnactor hipEventRecord failed", __FILE__, __LINE__) : hipSuccess;
        };
        auto end = [&](long long entries) -> hipError_t {
            float ms = 0;
            if (INSTRUMENT) {
                GR_CHECK(hipEventRecord(ev_round[1], stream), "MISEnactor hipEventRecord failed");
                GR_CHECK(hipEventSynchronize(ev_round[1]), "MISEnactor hipEventSynchronize failed");
                GR_CHECK(hipEventElapsedTime(&ms, ev_round[0], ev_round[1]), "MISEnactor hipEventElapsedTime failed");
                kernel_ms += ms;
            }
            trace.push_back({entries, ms});
            ++rounds;
            return hipSuccess;
        };

        long long count = n;          // undecided vertices
        const int *d_list = nullptr;  // round 1: every vertex
        int out = 0;
        bool tail = false;
        while (count > 0 && !tail) {
            if ((retval = begin())) return retval;
            GR_CHECK(hipMemsetAsync(ds->d_words + out, 0, sizeof(int), stream), "MISEnactor memset failed");
            hipLaunchKernelGGL((SweepKernel<MODE, HASHED>), dim3(grid(count, 2048)), dim3(kSweepThreads), 0, stream, g, k, st, d_list, count,
                               ds->d_list[out], ds->d_words + out, ds->d_reads);
            GR_CHECK(hipGetLastError(), "SweepKernel launch failed");
            ++launches;
            if ((retval = problem->ReadWords(ds->d_words + out, 1, stream))) return retval;
            const long long left = problem->h_words[0];
            if (left > count) return util::GRError(hipErrorUnknown, "MISEnactor: a sweep returned more vertices than it took", __FILE__, __LINE__);
            tail = use_tail && (left <= kTailVertices || left * 16 > count * 15);
            d_list = ds->d_list[out];
            out ^= 1;
            if ((retval = end(count))) return retval;
            count = left;
        }

        // ---- the tail: windows of the list in descending key order, each swept on the device until it is done ----
        if (count > 0) {
            const long long list_len = count;
            long long window = kTailVertices;
            if (max_grid_size > 0 && static_cast<long long>(max_grid_size) * kSweepThreads < window) window = static_cast<long long>(max_grid_size) * kSweepThreads;
            const long long windows = (list_len + window - 1) / window;
            if ((retval = problem->ReserveTail(windows))) return retval;
            if (windows > 1) {  // (one window holds all of H(v) for each of its vertices in any order)
                if ((retval = begin())) return retval;
                GR_CHECK(problem->order_sort.Reserve(list_len), "MISEnactor sort scratch failed");
                hipLaunchKernelGGL((OrderKeysKernel<HASHED>), dim3(grid(list_len, 2048)), dim3(256), 0, stream, k, d_list, list_len,
                                   problem->order_sort.Keys());
                GR_CHECK(hipGetLastError(), "OrderKeysKernel launch failed");
                unsigned long long *d_sorted = nullptr;
                GR_CHECK(problem->order_sort.Sort(list_len, 64, stream, &d_sorted), "MISEnactor sort failed");
                hipLaunchKernelGGL(OrderedListKernel, dim3(grid(list_len, 2048)), dim3(256), 0, stream, d_sorted, list_len, ds->d_list[out]);
                GR_CHECK(hipGetLastError(), "OrderedListKernel launch failed");
                launches += 2;  // (the radix sort's own kernels are not counted)
                d_list = ds->d_list[out];
                if (INSTRUMENT) {
                    float ms = 0;
                    GR_CHECK(hipEventRecord(ev_round[1], stream), "MISEnactor hipEventRecord failed");
                    GR_CHECK(hipEventSynchronize(ev_round[1]), "MISEnactor hipEventSynchronize failed");
                    GR_CHECK(hipEventElapsedTime(&ms, ev_round[0], ev_round[1]), "MISEnactor hipEventElapsedTime failed");
                    kernel_ms += ms;
                    sort_ms = ms;
                }
            }
            // A pass launches `ahead` windows from the first unfinished one: windows finish in order, and one behind an unfinished
            // window could only count its vertices, so the rest of the list is counted here instead of launched.  `ahead`
            // follows what the last pass finished (a chain much longer than a window finishes less than one per pass).
            long long first = 0;  // windows before this one are done
            long long ahead = 4;
            while (count > 0) {
                if ((retval = begin())) return retval;
                const long long last = first + ahead < windows ? first + ahead : windows;  // [first, last) are launched
                GR_CHECK(hipMemsetAsync(ds->d_tail_words, 0, sizeof(int) * static_cast<size_t>(2 * windows + 1), stream), "MISEnactor memset failed");
                for (long long w = first; w < last; ++w) {
                    const long long at = w * window;
                    const int len = static_cast<int>(list_len - at < window ? list_len - at : window);
                    hipLaunchKernelGGL((TailKernel<MODE, HASHED>), dim3((len + kSweepThreads - 1) / kSweepThreads), dim3(kSweepThreads), 0, stream, g, k, st,
                                       d_list + at, len, kTailSweeps, ds->d_tail_words, ds->d_tail_words + 1 + 2 * w, ds->d_reads);
                    GR_CHECK(hipGetLastError(), "TailKernel launch failed");
                    ++launches;
                }
                GR_CHECK(hipMemcpyAsync(problem->h_tail_words, ds->d_tail_words, sizeof(int) * static_cast<size_t>(2 * windows + 1), hipMemcpyDeviceToHost, stream),
                         "MISEnactor read-back failed");
                GR_CHECK(hipStreamSynchronize(stream), "MISEnactor read-back sync failed");
                const long long beyond = last < windows ? list_len - last * window : 0;  // never launched: all undecided
                const long long left = problem->h_tail_words[0] + beyond;
                for (long long w = first; w < last; ++w) tail_sweeps += problem->h_tail_words[2 + 2 * w];
                const long long was_first = first;
                while (first < last && problem->h_tail_words[1 + 2 * first] == 0) ++first;
                const long long finished = first - was_first;
                ahead = finished == last - was_first ? ahead * 2 : (2 * finished > 2 ? 2 * finished : 2);
                if (left >= count) return util::GRError(hipErrorUnknown, "MISEnactor: a tail pass decided no vertex", __FILE__, __LINE__);
                if ((retval = end(count))) return retval;
                count = left;
            }
        }
        unsigned long long reads[4] = {0, 0, 0, 0};
        GR_CHECK(hipMemcpyAsync(reads, ds->d_reads, sizeof(reads), hipMemcpyDeviceToHost, stream), "MISEnactor read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "MISEnactor read-back sync failed");
        entries_read = static_cast<long long>(reads[0]);
        polls = static_cast<long long>(reads[3]);
        return retval;
    }

    hipEvent_t ev_round[2] = {nullptr, nullptr};
};

}  // namespace mis
}  // namespace app
}  // namespace gunrock
