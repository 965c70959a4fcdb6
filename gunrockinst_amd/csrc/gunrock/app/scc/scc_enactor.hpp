// app/scc/scc_enactor.hpp -- host side of the strongly connected components: the schedule of scc_functor.hpp's steps.
//
// The run is a chain of steps (a pass over the live list, a trim sub-round, a search level, a propagation sweep); which one
// follows is scc_functor.hpp's Advance().  Three schedules:
//   ROUNDS       every step is a wide launch (StepKernel) and the host reads the words after it and advances: the plain form
//   DEVICE_LOOP  every step runs inside LoopKernel, one workgroup looping on the device, which advances by itself
//   AUTO         LoopKernel takes a stretch of steps for as long as each is narrow (Narrow(): loop_max_list vertices,
//                loop_max_entries row entries) and hands back the first wide one, which is then a launch
// INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/scc/scc_functor.hpp>
#include <gunrock/app/scc/scc_problem.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace scc {

constexpr int kStepWavesPerBlock = kSccThreads / util::kWaveSize;
constexpr int kStepWaves = kStepBlocks * kStepWavesPerBlock;
static_assert(SCC_AUTO == SCHEDULE_AUTO && SCC_ROUNDS == SCHEDULE_ROUNDS && SCC_DEVICE_LOOP == SCHEDULE_DEVICE_LOOP, "LoopOptions' schedules");

template <bool INSTRUMENT>
class SccEnactor : public EnactorBase {
   public:
    explicit SccEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    // options (grx_scc_set_option)
    LoopOptions loop;
    int pivot_phase = 1;
    int trim = 1;
    int pair_trim = 1;

    // of the last Enact (step: its launches and summed kernel time)
    StepHost<INSTRUMENT> step{"SccEnactor"};
    long long trimmed = 0, trim_rounds = 0, pivot_component = 0, colour_rounds = 0, sweeps = 0, bfs_levels = 0, entries_read = 0;
    std::vector<int> trace_kind;      // one row per phase: PHASE_*,
    std::vector<long long> trace_vertices;  // the vertices finished in it,
    std::vector<double> trace_ms;     // and the time to the next phase's start (the device's constant-rate counter)

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        // the run starts from one live region and words at 0: an Enact that does not follow a Reset makes its own
        if (!problem->fresh && (retval = problem->Reset())) return retval;
        problem->fresh = false;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes;
        trimmed = trim_rounds = pivot_component = colour_rounds = sweeps = bfs_levels = entries_read = 0;
        trace_kind.clear();
        trace_vertices.clear();
        trace_ms.clear();
        // pinned: the words, and behind them LoopKernel's state
        if ((retval = step.Begin(sizeof(unsigned) * W_COUNT + sizeof(State)))) return retval;
        auto run = [&](auto launch) { return step.Run(stream, launch); };

        const Ctx c = problem->DeviceCtx(loop.wave_min_row);
        unsigned *words = reinterpret_cast<unsigned *>(step.pinned);
        State *h_state = reinterpret_cast<State *>(words + W_COUNT);
        for (int i = 0; i < W_COUNT; ++i) words[i] = 0;
        State s = StartState(static_cast<unsigned>(n), 2ull * static_cast<unsigned long long>(problem->edges), trim != 0, pair_trim != 0, pivot_phase != 0, words);
        const Limits lim = loop.LimitsFor();

        while (s.kind < K_DONE) {
            if (loop.schedule == SCC_DEVICE_LOOP || (loop.schedule == SCC_AUTO && Narrow(s, lim))) {
                if ((retval = run([&]() { hipLaunchKernelGGL(LoopKernel, dim3(1), dim3(kLoopThreads), 0, stream, c, s, lim, ds->d_state); }))) return retval;
                if ((retval = step.Read(h_state, ds->d_state, sizeof(State), stream))) return retval;
                s = *h_state;
                continue;
            }
            const bool by_list = ByList(s.kind);
            const long long count = by_list ? s.list_len : static_cast<long long>(s.tail - s.head);
            const int tile = by_list || s.seed >= 0 ? util::kWaveSize : TileFor(count, kStepWaves, s.step_entries);
            const dim3 grid = StepGrid(count, tile, kStepWavesPerBlock, max_grid_size), block(kSccThreads);
            retval = run([&]() {
                switch (s.kind) {
                    case K_COUNT: hipLaunchKernelGGL(StepKernel<K_COUNT>, grid, block, 0, stream, c, s, tile); break;
                    case K_SCAN: hipLaunchKernelGGL(StepKernel<K_SCAN>, grid, block, 0, stream, c, s, tile); break;
                    case K_TRIM: hipLaunchKernelGGL(StepKernel<K_TRIM>, grid, block, 0, stream, c, s, tile); break;
                    case K_PICK: hipLaunchKernelGGL(StepKernel<K_PICK>, grid, block, 0, stream, c, s, tile); break;
                    case K_FWD: hipLaunchKernelGGL(StepKernel<K_FWD>, grid, block, 0, stream, c, s, tile); break;
                    case K_BWD: hipLaunchKernelGGL(StepKernel<K_BWD>, grid, block, 0, stream, c, s, tile); break;
                    case K_SPLIT: hipLaunchKernelGGL(StepKernel<K_SPLIT>, grid, block, 0, stream, c, s, tile); break;
                    case K_INIT: hipLaunchKernelGGL(StepKernel<K_INIT>, grid, block, 0, stream, c, s, tile); break;
                    case K_SWEEP: hipLaunchKernelGGL(StepKernel<K_SWEEP>, grid, block, 0, stream, c, s, tile); break;
                    case K_ROOTS: hipLaunchKernelGGL(StepKernel<K_ROOTS>, grid, block, 0, stream, c, s, tile); break;
                    case K_BACK: hipLaunchKernelGGL(StepKernel<K_BACK>, grid, block, 0, stream, c, s, tile); break;
                    case K_PAIR: hipLaunchKernelGGL(StepKernel<K_PAIR>, grid, block, 0, stream, c, s, tile); break;
                    default: hipLaunchKernelGGL(StepKernel<K_FINISH>, grid, block, 0, stream, c, s, tile); break;
                }
            });
            if (retval) return retval;
            if ((retval = step.Read(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream))) return retval;
            Advance(s, words, static_cast<unsigned>(n));
        }

        if (s.kind == K_STUCK) return util::GRError(hipErrorUnknown, "SccEnactor: a colouring round made no progress", __FILE__, __LINE__);
        hipError_t canonical = hipSuccess;
        if ((retval = run([&]() { canonical = problem->Canonical(); }))) return retval;
        if (canonical) return canonical;
        step.launches += 2;  // (Canonical is three kernels)
        trimmed = s.trimmed;
        trim_rounds = s.trim_rounds;
        pivot_component = s.pivot_component;
        colour_rounds = s.colour_rounds;
        sweeps = s.sweeps;
        bfs_levels = s.bfs_levels;

        // the trace and the counters
        if ((retval = step.Stamp(ds->d_counters + 1, stream))) return retval;
        unsigned long long counters[2] = {0, 0};
        GR_CHECK(hipMemcpyAsync(counters, ds->d_counters, sizeof(counters), hipMemcpyDeviceToHost, stream), "SccEnactor read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "SccEnactor read-back sync failed");
        entries_read = static_cast<long long>(counters[0]);
        const size_t rows = s.trace_at < kTraceRows ? s.trace_at : kTraceRows;
        if (rows > 0) {
            std::vector<int> kinds(rows);
            std::vector<unsigned> finished(rows);
            std::vector<unsigned long long> clocks(rows);
            GR_CHECK(hipMemcpyAsync(kinds.data(), ds->d_trace_kind, sizeof(int) * rows, hipMemcpyDeviceToHost, stream), "SccEnactor read trace failed");
            GR_CHECK(hipMemcpyAsync(finished.data(), ds->d_trace_finished, sizeof(unsigned) * rows, hipMemcpyDeviceToHost, stream),
                     "SccEnactor read trace failed");
            GR_CHECK(hipMemcpyAsync(clocks.data(), ds->d_trace_clock, sizeof(unsigned long long) * rows, hipMemcpyDeviceToHost, stream),
                     "SccEnactor read trace failed");
            GR_CHECK(hipStreamSynchronize(stream), "SccEnactor read trace sync failed");
            int khz = 0;
            int device = 0;
            GR_CHECK(hipGetDevice(&device), "SccEnactor hipGetDevice failed");
            GR_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device), "SccEnactor clock rate failed");
            for (size_t i = 0; i < rows; ++i) {
                const long long next_finished = i + 1 < rows ? finished[i + 1] : s.finished;
                const unsigned long long next_clock = i + 1 < rows ? clocks[i + 1] : counters[1];
                trace_kind.push_back(kinds[i]);
                trace_vertices.push_back(next_finished - static_cast<long long>(finished[i]));
                trace_ms.push_back(khz > 0 ? static_cast<double>(next_clock - clocks[i]) / static_cast<double>(khz) : 0.0);
            }
        }
        return retval;
    }
};

}  // namespace scc
}  // namespace app
}  // namespace gunrock
