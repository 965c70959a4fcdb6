// app/truss/truss_enactor.hpp -- host side of the k-truss decomposition: the schedule of truss_functor.hpp's steps.
//
// The peel is a sequence of steps: the scan that opens level s = k - 2 (the live edges at the level go to the queue, the rest give
// the next level) and the sub-rounds [head, tail) of the level.  Two schedules:
//   ROUNDS  every step is a wide launch and the host reads the words after it (one read-back per step): the plain form
//   AUTO    a step is wide when it is wide: a scan of more than loop_max_list edges, a sub-round whose shorter rows hold more than
//           loop_max_entries entries; everything else runs in LoopKernel, which goes on until it meets a step that is too wide
//           for it, so the many thin sub-rounds of a level's tail are one launch
// `rounds` counts the sub-rounds (the same under both schedules: they are those of the synchronous peel), not the read-backs;
// the scans of levels nobody is at are counted nowhere.  INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/truss/truss_functor.hpp>
#include <gunrock/app/truss/truss_problem.hpp>

namespace gunrock {
namespace app {
namespace truss {

constexpr int kPeelWavesPerBlock = kTrussThreads / util::kWaveSize;
constexpr int kPeelWaves = kStepBlocks * kPeelWavesPerBlock;  // 256 CUs x 8 workgroups x 4 waves
static_assert(TRUSS_AUTO == SCHEDULE_AUTO && TRUSS_ROUNDS == SCHEDULE_ROUNDS, "LoopOptions' schedules");

template <bool INSTRUMENT>
class TrussEnactor : public EnactorBase {
   public:
    explicit TrussEnactor(bool DEBUG = false) : EnactorBase(EDGE_FRONTIERS, DEBUG) { loop.wave_min_row = kWaveMinRow; }

    LoopOptions loop;  // options (grx_truss_set_option); wave_min_row starts at truss's own default

    // of the last Enact (step: its launches, read-backs of the words and summed kernel time)
    StepHost<INSTRUMENT> step{"TrussEnactor"};
    long long levels = 0;            // non-empty levels
    long long rounds = 0;            // sub-rounds
    long long edges_peeled = 0;
    long long entries_read = 0;
    std::vector<int> trace_k;        // the non-empty levels: k,
    std::vector<long long> trace_edges;  // the edges peeled at it,
    std::vector<double> trace_ms;    // and the time from its scan to the next one's (the device's constant-rate counter)

    template <typename Problem>
    hipError_t Enact(Problem *problem, int k_limit = -1, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        // the peel starts from the supports and an empty queue: an Enact that does not follow a Reset makes its own
        if (!problem->fresh && (retval = problem->Reset())) return retval;
        problem->fresh = false;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long M = problem->simple_edges;
        const int s_limit = k_limit < 0 ? INT_MAX : k_limit - 2;
        levels = rounds = edges_peeled = entries_read = 0;
        trace_k.clear();
        trace_edges.clear();
        trace_ms.clear();
        if ((retval = step.Begin(sizeof(unsigned) * W_COUNT))) return retval;
        auto run = [&](auto launch) { return step.Run(stream, launch); };
        auto grid_for = [&](long long work) { return GridFor(work, max_grid_size); };

        const Graph g = problem->DeviceGraph();
        const Trace tr = {ds->d_trace_k, ds->d_trace_tail, ds->d_trace_clock};
        unsigned *words = reinterpret_cast<unsigned *>(step.pinned);
        for (int i = 0; i < W_COUNT; ++i) words[i] = 0;
        auto read_words = [&]() { return step.Read(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream); };

        // the state of the peel (LoopKernel carries the same in registers)
        long long head = 0, tail = 0;
        int s = static_cast<int>(problem->min_support), sprev = -1, cur = 1;
        unsigned entries_seen = 0;
        bool open = false;       // the scan of level s has run
        bool wide_once = false;  // LoopKernel gave the next step back as too wide

        while (M > 0) {
            if (open && head >= tail) {  // level s has run dry: the next one is the smallest live value
                sprev = s;
                open = false;
                if (words[W_LOW] == kNoLevel || M - tail <= 0) break;
                s = static_cast<int>(words[W_LOW]);
            }
            if (!open) {
                if (M - tail <= 0) break;
                if (s >= s_limit) break;
            }
            const bool in_loop = !wide_once && loop.schedule == TRUSS_AUTO &&
                                 (open ? static_cast<long long>(words[W_ENTRIES] - entries_seen) <= loop.loop_max_entries : M <= loop.loop_max_list);
            wide_once = false;
            if (in_loop) {
                LoopArgs a;
                a.edges = M;
                a.head = head;
                a.entries_seen = entries_seen;
                a.s = s;
                a.sprev = sprev;
                a.s_limit = s_limit;
                a.round = cur;
                a.level_open = open ? 1 : 0;
                a.wave_min_row = loop.wave_min_row;
                a.max_list = loop.loop_max_list;
                a.max_entries = loop.loop_max_entries;
                a.max_steps = kLoopMaxSteps;
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(LoopKernel, dim3(1), dim3(kLoopThreads), 0, stream, g, ds->d_val, ds->d_stamp, ds->d_queue, ds->d_words,
                                            ds->d_counters, tr, a);
                     })))
                    return retval;
                if ((retval = read_words())) return retval;
                head = static_cast<int>(words[W_HEAD]);
                tail = words[W_TAIL];
                s = static_cast<int>(words[W_S]);
                sprev = static_cast<int>(words[W_SPREV]);
                cur = static_cast<int>(words[W_ROUND]);
                entries_seen = words[W_ENTRIES_SEEN];
                open = (words[W_STATUS] & 0x100u) != 0;
                const int status = static_cast<int>(words[W_STATUS] & 0xFFu);
                if (status == LOOP_DONE || status == LOOP_LIMIT) break;
                wide_once = status == LOOP_WIDE_PEEL || status == LOOP_WIDE_SCAN;
                continue;
            }
            if (open) {  // one sub-round, wide
                const int tile = TileFor(tail - head, kPeelWaves, static_cast<long long>(words[W_ENTRIES] - entries_seen));
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(PeelKernel, StepGrid(tail - head, tile, kPeelWavesPerBlock, max_grid_size), dim3(kTrussThreads), 0, stream, g,
                                            ds->d_val, ds->d_stamp, ds->d_queue, head, tail, s, cur, loop.wave_min_row, tile, ds->d_words, ds->d_counters);
                     })))
                    return retval;
                head = tail;
                entries_seen = words[W_ENTRIES];
                ++cur;
                ++rounds;
                if ((retval = read_words())) return retval;
                tail = words[W_TAIL];
                continue;
            }
            // the start of level s, wide: the scan of every edge
            GR_CHECK(hipMemsetAsync(ds->d_words + W_LOW, 0xFF, sizeof(unsigned), stream), "TrussEnactor memset failed");
            if ((retval = run([&]() {
                     hipLaunchKernelGGL(ScanKernel, grid_for(M), dim3(kTrussThreads), 0, stream, g, ds->d_val, ds->d_stamp, M, sprev, s, cur, ds->d_queue,
                                        ds->d_words, tr, static_cast<unsigned>(tail));
                 })))
                return retval;
            if ((retval = read_words())) return retval;
            tail = words[W_TAIL];
            open = true;
        }

        // truss = min(val, the level a limited run stopped at) + 2
        if ((retval = run([&]() { hipLaunchKernelGGL(FinishKernel, grid_for(M), dim3(256), 0, stream, ds->d_val, M, s_limit, ds->d_truss); }))) return retval;
        problem->enacted = true;
        edges_peeled = tail;

        // the trace and the counters: one more read, not counted as a read-back of the peel
        if ((retval = step.Stamp(ds->d_counters + 3, stream))) return retval;
        unsigned long long counters[4] = {0, 0, 0, 0};
        if ((retval = step.Copy(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream))) return retval;
        if ((retval = step.Copy(counters, ds->d_counters, sizeof(counters), stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "TrussEnactor read-back sync failed");
        entries_read = static_cast<long long>(counters[0]);
        rounds += words[W_SUBROUNDS];
        const size_t scans = words[W_TRACE];
        if (scans > 0) {
            std::vector<int> ks(scans), tails(scans);
            std::vector<unsigned long long> clocks(scans);
            GR_CHECK(hipMemcpyAsync(ks.data(), ds->d_trace_k, sizeof(int) * scans, hipMemcpyDeviceToHost, stream), "TrussEnactor read trace failed");
            GR_CHECK(hipMemcpyAsync(tails.data(), ds->d_trace_tail, sizeof(int) * scans, hipMemcpyDeviceToHost, stream), "TrussEnactor read trace failed");
            GR_CHECK(hipMemcpyAsync(clocks.data(), ds->d_trace_clock, sizeof(unsigned long long) * scans, hipMemcpyDeviceToHost, stream),
                     "TrussEnactor read trace failed");
            GR_CHECK(hipStreamSynchronize(stream), "TrussEnactor read trace sync failed");
            int khz = 0;
            int device = 0;
            GR_CHECK(hipGetDevice(&device), "TrussEnactor hipGetDevice failed");
            GR_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device), "TrussEnactor clock rate failed");
            for (size_t i = 0; i < scans; ++i) {
                const long long next_tail = i + 1 < scans ? tails[i + 1] : tail;
                const unsigned long long next_clock = i + 1 < scans ? clocks[i + 1] : counters[3];
                if (next_tail == tails[i]) continue;  // a level nobody was at
                trace_k.push_back(ks[i]);
                trace_edges.push_back(next_tail - tails[i]);
                trace_ms.push_back(khz > 0 ? static_cast<double>(next_clock - clocks[i]) / static_cast<double>(khz) : 0.0);
            }
        }
        levels = static_cast<long long>(trace_k.size());
        return retval;
    }
};

}  // namespace truss
}  // namespace app
}  // namespace gunrock
