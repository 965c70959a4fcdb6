// app/maxflow/maxflow_enactor.hpp -- host side of the maximum flow: the schedule of maxflow_functor.hpp's steps.
//
// Enact runs push-relabel in two phases and then the cut:
//   preflow  global relabel (a backward search from sink: exact heights, n for the vertices that cannot reach it), the arcs of src
//            saturated, then rounds of the discharge kernel over the active list until it is empty.  After relabel_interval * n
//            relabels the global relabel runs again (it also does the gap heuristic's work) and the list is rebuilt from scratch.
//   return   the vertices that still hold excess cannot reach sink: heights become n + the residual distance to src (the same search
//            from src) and the same rounds run with the bound 2n until no excess is left outside src and sink.
//   cut      a forward search from src (side 0) and a backward one from sink (side 2), one pass over the vertices and one over the
//            pairs.  The pass over the vertices looks at the certificate on the device: no excess outside src and sink, and sink not
//            reached from src.  A flow with those two properties is maximum whatever the rounds before it read, so when one fails
//            the enactor goes back to the preflow phase with a fresh global relabel instead of reporting.
// A step is a round or a search level.  Three schedules:
//   ROUNDS       every step is a wide launch and a read-back
//   DEVICE_LOOP  steps run in the one-workgroup loop on the device (at most kLoopMaxSteps per launch)
//   AUTO         a stretch of narrow steps (Narrow(): loop_max_list vertices, loop_max_entries row entries) is one loop launch, a
//                wide step is a launch of its own
// Nothing spins: every device loop has a step bound, no kernel waits on another workgroup, and Enact counts its rounds and stops
// with kGaveUp when they pass max_rounds.  INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/maxflow/maxflow_functor.hpp>
#include <gunrock/app/maxflow/maxflow_problem.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace maxflow {

constexpr int kStepWavesPerBlock = kMaxflowThreads / util::kWaveSize;
constexpr int kStepWaves = kStepBlocks * kStepWavesPerBlock;
static_assert(MAXFLOW_AUTO == SCHEDULE_AUTO && MAXFLOW_ROUNDS == SCHEDULE_ROUNDS && MAXFLOW_DEVICE_LOOP == SCHEDULE_DEVICE_LOOP,
              "LoopOptions' schedules");
constexpr long long kDefaultMaxRounds = 4000000;  // the largest count measured and the margin over it
constexpr long long kMaxMaxRounds = 1ll << 30;    // (a round's stamp is an int)
constexpr int kMaxRestarts = 64;                  // trips back from a failed certificate before Enact gives up
constexpr int kGaveUp = -4;                       // GRX_MAXFLOW_GAVE_UP

template <bool INSTRUMENT>
class MaxflowEnactor : public EnactorBase {
   public:
    explicit MaxflowEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    // options (grx_maxflow_set_option)
    LoopOptions loop;
    int discharge_steps = kDischargeSteps;
    double relabel_interval = 0.1;  // relabels between two global relabels, as a multiple of n (the sweep)
    long long max_rounds = kDefaultMaxRounds;

    // of the last Enact (step: its launches, read-backs and summed kernel time)
    StepHost<INSTRUMENT> step{"MaxflowEnactor"};
    long long rounds = 0, global_relabels = 0, pushes = 0, relabels = 0, entries_read = 0, restarts = 0;
    bool gave_up = false;
    std::vector<long long> trace_rounds;  // one row per phase: the rounds it ran (the cut: its search levels),
    std::vector<double> trace_ms;         // and its time, summed over the restarts (the device's constant-rate counter)

    // hipSuccess, a hipError_t, or hipErrorUnknown with gave_up set
    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        if (problem->src < 0) return hipErrorNotReady;  // no Reset yet: no pair
        if (!problem->fresh && (retval = problem->Reset(problem->src, problem->sink))) return retval;
        problem->fresh = false;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, M = problem->pairs;
        rounds = global_relabels = pushes = relabels = entries_read = restarts = 0;
        gave_up = false;
        trace_rounds.assign(PHASE_COUNT, 0);
        trace_ms.assign(PHASE_COUNT, 0.0);
        if ((retval = step.Begin(512))) return retval;
        auto run = [&](auto launch) { return step.Run(stream, launch); };
        auto stamp_clock = [&](int slot) { return step.Stamp(ds->d_clock + slot, stream); };
        auto grid_for = [&](long long work) { return GridFor(work, max_grid_size); };
        auto step_grid = [&](long long count, int tile) { return StepGrid(count, tile, kStepWavesPerBlock, max_grid_size); };

        const Ctx c = problem->DeviceCtx(loop.wave_min_row, discharge_steps);
        const Limits lim = loop.LimitsFor();
        auto in_loop = [&](long long count, long long entries) { return loop.InLoop(count, entries); };
        unsigned relabel_limit = kNever;
        {
            const double want = relabel_interval * static_cast<double>(n);
            if (want < 4.0e9) relabel_limit = want < 1.0 ? 1u : static_cast<unsigned>(want);
        }
        unsigned char *h_pinned = step.pinned;  // the read-backs land here without a staging copy
        unsigned *words = reinterpret_cast<unsigned *>(h_pinned);                            // W_COUNT
        Front *h_front = reinterpret_cast<Front *>(h_pinned + 64);
        Active *h_active = reinterpret_cast<Active *>(h_pinned + 128);
        unsigned long long *h_counters = reinterpret_cast<unsigned long long *>(h_pinned + 192);  // C_COUNT
        unsigned long long *h_clock = reinterpret_cast<unsigned long long *>(h_pinned + 320);     // 2 stamps
        long long *h_value = reinterpret_cast<long long *>(h_pinned + 352);
        auto read_words = [&]() { return step.Read(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream); };
        int khz = 0, device = 0;
        GR_CHECK(hipGetDevice(&device), "MaxflowEnactor hipGetDevice failed");
        GR_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device), "MaxflowEnactor clock rate failed");
        // a phase's time: the two stamps around it (read with the phase's last read-back)
        auto phase_time = [&](int phase) -> hipError_t {
            hipError_t retval = hipSuccess;
            GR_CHECK(hipMemcpyAsync(h_clock, ds->d_clock + phase, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, stream),
                     "MaxflowEnactor read-back failed");
            GR_CHECK(hipStreamSynchronize(stream), "MaxflowEnactor read-back sync failed");
            if (khz > 0 && h_clock[1] >= h_clock[0]) trace_ms[phase] += static_cast<double>(h_clock[1] - h_clock[0]) / static_cast<double>(khz);
            return retval;
        };

        // one search from `root` at level `base`; *levels receives the levels it ran
        auto search = [&](const Search &s, int root, int base, long long *levels) -> hipError_t {
            hipError_t retval = hipSuccess;
            if ((retval = run([&]() { hipLaunchKernelGGL(oprtr::FillKernel<int>, grid_for(n), dim3(256), 0, stream, s.out, n, s.unseen); }))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(SeedKernel, dim3(1), dim3(1), 0, stream, c, s, root, base); }))) return retval;
            if ((retval = read_words())) return retval;
            Front f = {base, 0u, words[W_TAIL], words[W_ENTRIES], words[W_ENTRIES]};
            while (f.head < f.tail) {
                const long long count = f.tail - f.head;
                if (in_loop(count, f.step_entries)) {
                    if ((retval = run([&]() { hipLaunchKernelGGL(SearchLoopKernel, dim3(1), dim3(kLoopThreads), 0, stream, c, s, f, lim, ds->d_front); })))
                        return retval;
                    if ((retval = step.Read(h_front, ds->d_front, sizeof(Front), stream))) return retval;
                    f = *h_front;
                    continue;
                }
                const int tile = TileFor(count, kStepWaves, f.step_entries);
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(SearchKernel, step_grid(count, tile), dim3(kMaxflowThreads), 0, stream, c, s, f.level, f.head, f.tail, tile);
                     })))
                    return retval;
                if ((retval = read_words())) return retval;
                ++f.level;
                f.head = f.tail;
                f.tail = words[W_TAIL];
                f.step_entries = words[W_ENTRIES] - f.entries_seen;
                f.entries_seen = words[W_ENTRIES];
            }
            if (levels) *levels += f.level - base;
            return retval;
        };

        int stamp = 0;  // of the last round
        // W_NEXT and W_NEXT_ENTRIES at 0 in front of everything that appends to a list
        auto clear_next = [&]() -> hipError_t {
            return util::GRError(hipMemsetAsync(ds->d_words + W_NEXT, 0, sizeof(unsigned) * 2, stream), "MaxflowEnactor memset failed", __FILE__, __LINE__);
        };
        // one phase: relabel from `root`, then rounds until the list is empty; heights from `bound` on are out of it
        auto phase = [&](int which, int root, int skip, int base, int bound, bool saturate) -> hipError_t {
            hipError_t retval = hipSuccess;
            const Search s = {ds->d_height, bound, skip, 1};
            for (;;) {
                if ((retval = search(s, root, base, nullptr))) return retval;
                ++global_relabels;
                if (saturate) {
                    if ((retval = run([&]() { hipLaunchKernelGGL(SaturateKernel, dim3(1), dim3(256), 0, stream, c); }))) return retval;
                    saturate = false;
                }
                GR_CHECK(hipMemsetAsync(ds->d_words + W_RELABELS, 0, sizeof(unsigned), stream), "MaxflowEnactor memset failed");
                if ((retval = clear_next())) return retval;
                if ((retval = run([&]() { hipLaunchKernelGGL(BuildActiveKernel, grid_for(n), dim3(256), 0, stream, c, ds->d_list[0], bound); })))
                    return retval;
                if ((retval = read_words())) return retval;
                Active a = {words[W_NEXT], words[W_NEXT_ENTRIES], 0, stamp, 0u, 0};
                while (a.count > 0 && (relabel_limit == kNever || a.relabels < relabel_limit)) {
                    if (rounds >= max_rounds) {
                        gave_up = true;
                        return hipErrorUnknown;
                    }
                    if ((retval = clear_next())) return retval;
                    if (in_loop(a.count, a.entries)) {
                        Limits now = lim;  // (the loop stops at max_rounds too)
                        if (max_rounds - rounds < now.max_steps) now.max_steps = static_cast<int>(max_rounds - rounds);
                        if ((retval = run([&]() {
                                 hipLaunchKernelGGL(DischargeLoopKernel, dim3(1), dim3(kLoopThreads), 0, stream, c, ds->d_list[0], ds->d_list[1], a, now, bound,
                                                    relabel_limit, ds->d_active);
                             })))
                            return retval;
                        if ((retval = step.Read(h_active, ds->d_active, sizeof(Active), stream))) return retval;
                        a = *h_active;
                        rounds += a.steps;
                        trace_rounds[which] += a.steps;
                        continue;
                    }
                    const int tile = TileFor(a.count, kStepWaves, a.entries);
                    const int *cur = ds->d_list[a.cur];
                    int *next = ds->d_list[a.cur ^ 1];
                    if ((retval = run([&]() {
                             hipLaunchKernelGGL(DischargeKernel, step_grid(a.count, tile), dim3(kMaxflowThreads), 0, stream, c, cur, next, a.count, bound,
                                                a.stamp + 1, tile);
                         })))
                        return retval;
                    if ((retval = read_words())) return retval;
                    a.count = words[W_NEXT] < static_cast<unsigned>(n) ? words[W_NEXT] : static_cast<unsigned>(n);
                    a.entries = words[W_NEXT_ENTRIES];
                    a.relabels = words[W_RELABELS];
                    a.cur ^= 1;
                    ++a.stamp;
                    ++rounds;
                    ++trace_rounds[which];
                }
                stamp = a.stamp;
                if (a.count == 0) return retval;
            }
        };

        for (;;) {
            // ---- preflow ----
            if ((retval = stamp_clock(PHASE_PREFLOW))) return retval;
            if ((retval = phase(PHASE_PREFLOW, problem->sink, problem->src, 0, static_cast<int>(n), true))) return retval;
            // ---- return ----
            if ((retval = stamp_clock(PHASE_RETURN))) return retval;
            if ((retval = phase_time(PHASE_PREFLOW))) return retval;
            if ((retval = phase(PHASE_RETURN, problem->src, problem->sink, static_cast<int>(n), static_cast<int>(2 * n), false))) return retval;
            // ---- cut ----
            if ((retval = stamp_clock(PHASE_CUT))) return retval;
            if ((retval = phase_time(PHASE_RETURN))) return retval;
            GR_CHECK(hipMemsetAsync(ds->d_counters + C_SIDE0, 0, sizeof(unsigned long long) * (C_COUNT - C_SIDE0), stream), "MaxflowEnactor memset failed");
            const Search fwd = {ds->d_fwd, kFar, -1, 0}, bwd = {ds->d_bwd, kFar, -1, 1};
            if ((retval = search(fwd, problem->src, 0, &trace_rounds[PHASE_CUT]))) return retval;
            if ((retval = search(bwd, problem->sink, 0, &trace_rounds[PHASE_CUT]))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(SidesKernel, grid_for(n), dim3(256), 0, stream, c, ds->d_fwd, ds->d_bwd, ds->d_side); })))
                return retval;
            if (M > 0 && (retval = run([&]() {
                              hipLaunchKernelGGL(PairsKernel, grid_for(M), dim3(256), 0, stream, c, ds->d_a, ds->d_b, ds->d_pent, ds->d_cap, ds->d_side, M,
                                                 ds->d_flow, ds->d_cut);
                          })))
                return retval;
            if ((retval = stamp_clock(PHASE_COUNT))) return retval;
            GR_CHECK(hipMemcpyAsync(h_counters, ds->d_counters, sizeof(unsigned long long) * C_COUNT, hipMemcpyDeviceToHost, stream),
                     "MaxflowEnactor read-back failed");
            GR_CHECK(hipMemcpyAsync(h_value, ds->d_excess + problem->sink, sizeof(long long), hipMemcpyDeviceToHost, stream), "MaxflowEnactor read-back failed");
            if ((retval = read_words())) return retval;
            if ((retval = phase_time(PHASE_CUT))) return retval;
            const bool certified = words[W_FLAG] == 0 && static_cast<long long>(h_counters[C_CAP0]) == *h_value &&
                                   static_cast<long long>(h_counters[C_CAP1]) == *h_value;
            if (certified) break;
            // the certificate failed (rounds that read stale heights can end a phase early): once more, from a fresh global relabel
            if (++restarts > kMaxRestarts) {
                gave_up = true;
                return hipErrorUnknown;
            }
            GR_CHECK(hipMemsetAsync(ds->d_words + W_FLAG, 0, sizeof(unsigned), stream), "MaxflowEnactor memset failed");
        }

        entries_read = static_cast<long long>(h_counters[C_READS]);
        pushes = static_cast<long long>(h_counters[C_PUSHES]);
        relabels = static_cast<long long>(h_counters[C_RELABELS]);
        Summary &out = problem->summary;
        out = Summary();
        out.value = *h_value;
        out.side0 = static_cast<long long>(h_counters[C_SIDE0]);
        out.side1 = static_cast<long long>(h_counters[C_SIDE1]);
        out.side2 = static_cast<long long>(h_counters[C_SIDE2]);
        out.cut0 = static_cast<long long>(h_counters[C_CUT0]);
        out.cut1 = static_cast<long long>(h_counters[C_CUT1]);
        out.cap0 = static_cast<long long>(h_counters[C_CAP0]);
        out.cap1 = static_cast<long long>(h_counters[C_CAP1]);
        problem->enacted = true;
        return retval;
    }
};

}  // namespace maxflow
}  // namespace app
}  // namespace gunrock
