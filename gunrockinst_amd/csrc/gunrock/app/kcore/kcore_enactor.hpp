// app/kcore/kcore_enactor.hpp -- host side of the k-core decomposition: the schedule of kcore_functor.hpp's steps.
//
// The peel is a sequence of steps: the scan that opens level k (the live vertices at the level go to the queue, the rest give the
// next level), the sub-rounds [head, tail) of the level, and now and then a rebuild of the live list.  Three schedules:
//   ROUNDS       every step is a wide launch and the host reads the words after it (one read-back per sub-round): the plain form
//   DEVICE_LOOP  every step runs inside LoopKernel, one workgroup looping on the device
//   AUTO         a step is wide when it is wide: a scan of more than loop_max_list live vertices, a sub-round whose rows hold more
//                than loop_max_entries entries; everything else runs in LoopKernel, which goes on until it meets a step that is
//                too wide for it, so a long thin stretch (a path, the late levels of an R-MAT graph) is one launch
// The live list is rebuilt when the live vertices are at most compact_below of its length (at a level's start).
// INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/kcore/kcore_functor.hpp>
#include <gunrock/app/kcore/kcore_problem.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace kcore {

constexpr int kPeelWavesPerBlock = kKcoreThreads / util::kWaveSize;
constexpr int kPeelWaves = kStepBlocks * kPeelWavesPerBlock;  // 256 CUs x 8 workgroups x 4 waves
static_assert(KCORE_AUTO == SCHEDULE_AUTO && KCORE_ROUNDS == SCHEDULE_ROUNDS && KCORE_DEVICE_LOOP == SCHEDULE_DEVICE_LOOP, "LoopOptions' schedules");

template <bool INSTRUMENT>
class KcoreEnactor : public EnactorBase {
   public:
    explicit KcoreEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    // options (grx_kcore_set_option)
    LoopOptions loop;
    double compact_below = kCompactBelow;

    // of the last Enact (step: its launches and summed kernel time)
    StepHost<INSTRUMENT> step{"KcoreEnactor"};
    long long levels = 0;           // non-empty levels
    long long rounds = 0;           // host-visible read-backs
    long long vertices_peeled = 0;
    long long entries_read = 0;
    long long compactions = 0;
    long long device_subrounds = 0;  // sub-rounds that ran inside LoopKernel
    std::vector<int> trace_k;        // the non-empty levels: the level,
    std::vector<long long> trace_vertices;  // the vertices peeled at it,
    std::vector<double> trace_ms;    // and the time from its scan to the next one's (the device's constant-rate counter)

    template <typename Problem>
    hipError_t Enact(Problem *problem, int k_limit = -1, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        // the peel starts from d(v) and an empty queue: an Enact that does not follow a Reset makes its own
        if (!problem->fresh && (retval = problem->Reset())) return retval;
        problem->fresh = false;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, zeros = problem->zeros;
        levels = rounds = entries_read = compactions = device_subrounds = 0;
        vertices_peeled = zeros;
        trace_k.clear();
        trace_vertices.clear();
        trace_ms.clear();
        if ((retval = step.Begin(sizeof(unsigned) * W_COUNT))) return retval;
        auto run = [&](auto launch) { return step.Run(stream, launch); };
        auto grid_for = [&](long long work) { return GridFor(work, max_grid_size); };

        const Graph g = problem->DeviceGraph();
        const Trace tr = {ds->d_trace_k, ds->d_trace_tail, ds->d_trace_clock};
        unsigned *words = reinterpret_cast<unsigned *>(step.pinned);
        for (int i = 0; i < W_COUNT; ++i) words[i] = 0;
        auto read_words = [&]() { return step.Read(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream); };  // (one per round)

        // the state of the peel (LoopKernel carries the same in registers)
        long long head = 0, tail = 0, list_len = n;
        int list_buf = -1, k = static_cast<int>(problem->min_degree), kprev = 0;
        unsigned entries_seen = 0;
        bool open = false;       // the scan of level k has run
        bool wide_once = false;  // LoopKernel gave the next step back as too wide
        bool limited = false;

        while (problem->simple_edges > 0) {
            if (open && head >= tail) {  // level k has run dry: the next one is the smallest live value
                kprev = k;
                open = false;
                if (words[W_LOW] == kNoLevel || n - zeros - tail <= 0) break;
                k = static_cast<int>(words[W_LOW]);
            }
            if (!open) {
                if (n - zeros - tail <= 0) break;
                if (k_limit >= 0 && k >= k_limit) { limited = true; break; }
            }
            const bool in_loop =
                !wide_once && (loop.schedule == KCORE_DEVICE_LOOP ||
                               (loop.schedule == KCORE_AUTO && (open ? static_cast<long long>(words[W_ENTRIES] - entries_seen) <= loop.loop_max_entries
                                                                     : list_len <= loop.loop_max_list)));
            wide_once = false;
            if (in_loop) {
                const oprtr::Limits lim = loop.LimitsFor();
                LoopArgs a;
                a.d_list[0] = ds->d_list[0];
                a.d_list[1] = ds->d_list[1];
                a.list_buf = list_buf;
                a.list_len = list_len;
                a.nodes = n;
                a.zeros = zeros;
                a.head = head;
                a.entries_seen = entries_seen;
                a.k = k;
                a.kprev = kprev;
                a.k_limit = k_limit;
                a.level_open = open ? 1 : 0;
                a.wave_min_row = loop.wave_min_row;
                a.compact_below = compact_below;
                a.max_list = lim.max_list;
                a.max_entries = lim.max_entries;
                a.max_steps = lim.max_steps;
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(LoopKernel, dim3(1), dim3(kLoopThreads), 0, stream, g, ds->d_core, ds->d_queue, ds->d_words, ds->d_counters, tr, a);
                     })))
                    return retval;
                if ((retval = read_words())) return retval;
                head = static_cast<int>(words[W_HEAD]);
                tail = words[W_TAIL];
                k = static_cast<int>(words[W_K]);
                kprev = static_cast<int>(words[W_KPREV]);
                list_len = static_cast<int>(words[W_LIST_LEN]);
                list_buf = static_cast<int>(words[W_LIST_BUF]);
                entries_seen = words[W_ENTRIES_SEEN];
                open = (words[W_STATUS] & 0x100u) != 0;
                const int status = static_cast<int>(words[W_STATUS] & 0xFFu);
                if (status == LOOP_DONE) break;
                if (status == LOOP_LIMIT) { limited = true; break; }
                wide_once = status == LOOP_WIDE_PEEL || status == LOOP_WIDE_SCAN;
                continue;
            }
            if (open) {  // one sub-round, wide
                const int tile = TileFor(tail - head, kPeelWaves, static_cast<long long>(words[W_ENTRIES] - entries_seen));
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(PeelKernel, StepGrid(tail - head, tile, kPeelWavesPerBlock, max_grid_size), dim3(kKcoreThreads), 0, stream, g,
                                            ds->d_core, ds->d_queue, head, tail, k, loop.wave_min_row, tile, ds->d_words, ds->d_counters);
                     })))
                    return retval;
                head = tail;
                entries_seen = words[W_ENTRIES];
                if ((retval = read_words())) return retval;
                tail = words[W_TAIL];
                continue;
            }
            // the start of level k, wide: the rebuild of the live list when it is due, then the scan
            const long long alive = n - zeros - tail;
            if (compact_below > 0 && static_cast<double>(alive) <= compact_below * static_cast<double>(list_len)) {
                const int to = list_buf == 0 ? 1 : 0;
                GR_CHECK(hipMemsetAsync(ds->d_words + W_SCRATCH, 0, sizeof(unsigned), stream), "KcoreEnactor memset failed");
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(CompactKernel, grid_for(list_len), dim3(kKcoreThreads), 0, stream, ds->d_core,
                                            list_buf < 0 ? nullptr : ds->d_list[list_buf], list_len, kprev, ds->d_list[to], ds->d_words + W_SCRATCH);
                     })))
                    return retval;
                list_buf = to;
                list_len = alive;  // (every live vertex is in the list, and only those are kept: no read-back)
                ++compactions;
            }
            GR_CHECK(hipMemsetAsync(ds->d_words + W_LOW, 0xFF, sizeof(unsigned), stream), "KcoreEnactor memset failed");
            if ((retval = run([&]() {
                     hipLaunchKernelGGL(ScanKernel, grid_for(list_len), dim3(kKcoreThreads), 0, stream, g, ds->d_core,
                                        list_buf < 0 ? nullptr : ds->d_list[list_buf], list_len, kprev, k, ds->d_queue, ds->d_words, ds->d_counters, tr,
                                        static_cast<unsigned>(tail));
                 })))
                return retval;
            if ((retval = read_words())) return retval;
            tail = words[W_TAIL];
            open = true;
        }

        if (limited) {  // what is live at level k_limit has a core number of at least k_limit
            if ((retval = run([&]() { hipLaunchKernelGGL(ClampKernel, grid_for(n), dim3(256), 0, stream, ds->d_core, n, k_limit); }))) return retval;
        }
        vertices_peeled = zeros + tail;
        rounds = step.readbacks;

        // the trace and the counters: one more read, not counted as a round of the peel
        if ((retval = step.Stamp(ds->d_counters + 3, stream))) return retval;
        unsigned long long counters[4] = {0, 0, 0, 0};
        if ((retval = step.Copy(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream))) return retval;
        if ((retval = step.Copy(counters, ds->d_counters, sizeof(counters), stream))) return retval;
        GR_CHECK(hipStreamSynchronize(stream), "KcoreEnactor read-back sync failed");
        entries_read = static_cast<long long>(counters[0]);
        compactions += words[W_COMPACTIONS];
        device_subrounds = words[W_SUBROUNDS];
        const size_t scans = words[W_TRACE];
        if (scans > 0) {
            std::vector<int> ks(scans), tails(scans);
            std::vector<unsigned long long> clocks(scans);
            GR_CHECK(hipMemcpyAsync(ks.data(), ds->d_trace_k, sizeof(int) * scans, hipMemcpyDeviceToHost, stream), "KcoreEnactor read trace failed");
            GR_CHECK(hipMemcpyAsync(tails.data(), ds->d_trace_tail, sizeof(int) * scans, hipMemcpyDeviceToHost, stream), "KcoreEnactor read trace failed");
            GR_CHECK(hipMemcpyAsync(clocks.data(), ds->d_trace_clock, sizeof(unsigned long long) * scans, hipMemcpyDeviceToHost, stream),
                     "KcoreEnactor read trace failed");
            GR_CHECK(hipStreamSynchronize(stream), "KcoreEnactor read trace sync failed");
            int khz = 0;
            int device = 0;
            GR_CHECK(hipGetDevice(&device), "KcoreEnactor hipGetDevice failed");
            GR_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device), "KcoreEnactor clock rate failed");
            for (size_t i = 0; i < scans; ++i) {
                const long long next_tail = i + 1 < scans ? tails[i + 1] : tail;
                const unsigned long long next_clock = i + 1 < scans ? clocks[i + 1] : counters[3];
                if (next_tail == tails[i]) continue;  // a level nobody was at
                trace_k.push_back(ks[i]);
                trace_vertices.push_back(next_tail - tails[i]);
                trace_ms.push_back(khz > 0 ? static_cast<double>(next_clock - clocks[i]) / static_cast<double>(khz) : 0.0);
            }
        }
        levels = static_cast<long long>(trace_k.size());
        return retval;
    }
};

}  // namespace kcore
}  // namespace app
}  // namespace gunrock
