// app/matching/matching_enactor.hpp -- host side of the heavy-edge matching: the schedule of matching_functor.hpp's rounds.
//
// A round is the point step and the match step over the live list.  Three schedules:
//   ROUNDS       every round is a launch pair (PointKernel, MatchKernel) and one read-back
//   DEVICE_LOOP  rounds run in the one-workgroup loop on the device (at most kLoopMaxSteps per launch)
//   AUTO         a stretch of narrow rounds (Narrow(): loop_max_list vertices, loop_max_entries row entries) is one loop launch, a
//                wide round is a launch pair of its own
// The largest-keyed pair with two unmatched ends is matched by the round that sees it, and a round that matches nothing leaves an
// empty list, so an Enact runs at most matched + 1 <= n / 2 + 1 rounds: that bound is the default of max_rounds.  `rounds` counts
// the rounds that matched a pair, which is the count of the mutual-best rounds of the definition; the closing round in which the
// last vertices find no unmatched neighbour is in `sweeps` only.  Nothing spins: every device loop has a step bound, no kernel waits
// on another workgroup, and Enact stops with kGaveUp when its rounds pass max_rounds.  INSTRUMENT times every kernel with HIP events
// (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/matching/matching_functor.hpp>
#include <gunrock/app/matching/matching_problem.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace matching {

constexpr int kStepWavesPerBlock = kMatchingThreads / util::kWaveSize;
constexpr int kStepWaves = kStepBlocks * kStepWavesPerBlock;
static_assert(MATCHING_AUTO == SCHEDULE_AUTO && MATCHING_ROUNDS == SCHEDULE_ROUNDS && MATCHING_DEVICE_LOOP == SCHEDULE_DEVICE_LOOP,
              "LoopOptions' schedules");
constexpr long long kMaxMaxRounds = 1ll << 31;
constexpr int kGaveUp = -4;  // GRX_MATCHING_GAVE_UP

template <bool INSTRUMENT>
class MatchingEnactor : public EnactorBase {
   public:
    explicit MatchingEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) { loop.loop_max_entries = kLoopMaxEntries; }

    // options (grx_matching_set_option)
    LoopOptions loop;          // (loop_max_entries starts at matching's own default)
    long long max_rounds = 0;  // 0: n / 2 + 1

    // of the last Enact (step: its launches, read-backs and summed kernel time)
    StepHost<INSTRUMENT> step{"MatchingEnactor"};
    long long rounds = 0, sweeps = 0, loop_rounds = 0, entries_read = 0, polls = 0;
    bool gave_up = false;
    // one row per host step: a wide round or a loop launch, the rounds it ran, the list it started from and the pairs it matched
    std::vector<int> trace_kind;
    std::vector<long long> trace_rounds, trace_list, trace_matched;

    // hipSuccess, a hipError_t, or hipErrorUnknown with gave_up set
    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        if (!problem->fresh && (retval = problem->Reset())) return retval;
        problem->fresh = false;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, M = problem->pairs;
        rounds = sweeps = loop_rounds = entries_read = polls = 0;
        gave_up = false;
        trace_kind.clear();
        trace_rounds.clear();
        trace_list.clear();
        trace_matched.clear();
        if ((retval = step.Begin(256))) return retval;
        auto run = [&](auto launch) { return step.Run(stream, launch); };
        auto step_grid = [&](long long count, int tile) { return StepGrid(count, tile, kStepWavesPerBlock, max_grid_size); };

        const Ctx c = problem->DeviceCtx(loop.wave_min_row);
        const Limits lim = loop.LimitsFor();
        auto in_loop = [&](long long count, long long entries) { return loop.InLoop(count, entries); };
        const long long bound = max_rounds > 0 ? max_rounds : n / 2 + 1;
        unsigned char *h_pinned = step.pinned;  // the read-backs land here without a staging copy
        unsigned *words = reinterpret_cast<unsigned *>(h_pinned);  // W_COUNT
        Active *h_active = reinterpret_cast<Active *>(h_pinned + 64);
        unsigned long long *h_counters = reinterpret_cast<unsigned long long *>(h_pinned + 128);  // C_COUNT
        auto read_words = [&]() { return step.Read(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream); };
        // W_NEXT and W_NEXT_ENTRIES at 0 in front of everything that appends to a list
        auto clear_next = [&]() -> hipError_t {
            return util::GRError(hipMemsetAsync(ds->d_words + W_NEXT, 0, sizeof(unsigned) * 2, stream), "MatchingEnactor memset failed", __FILE__, __LINE__);
        };
        auto trace = [&](int kind, long long ran, long long list, long long matched) {
            trace_kind.push_back(kind);
            trace_rounds.push_back(ran);
            trace_list.push_back(list);
            trace_matched.push_back(matched);
        };

        // (Reset left the first list in list 0 and its size and entries in the words)
        if ((retval = read_words())) return retval;
        Active a = {words[W_NEXT], words[W_NEXT_ENTRIES], 0, 0u, 0, 0};
        while (a.count > 0) {
            if (sweeps >= bound) {
                gave_up = true;
                return hipErrorUnknown;
            }
            if ((retval = clear_next())) return retval;
            const long long list = a.count;
            const unsigned before = a.matched;
            if (in_loop(a.count, a.entries)) {
                Limits now = lim;  // (the loop stops at the bound too)
                if (bound - sweeps < now.max_steps) now.max_steps = static_cast<int>(bound - sweeps);
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(LoopKernel, dim3(1), dim3(kLoopThreads), 0, stream, c, ds->d_list[0], ds->d_list[1], a, now, ds->d_active);
                     })))
                    return retval;
                if ((retval = step.Read(h_active, ds->d_active, sizeof(Active), stream))) return retval;
                a = *h_active;
                sweeps += a.steps;
                loop_rounds += a.steps;
                rounds += a.match_steps;
                trace(STEP_LOOP, a.steps, list, static_cast<long long>(a.matched - before));
                continue;
            }
            const int tile = TileFor(a.count, kStepWaves, a.entries);
            const int *cur = ds->d_list[a.cur];
            int *next = ds->d_list[a.cur ^ 1];
            if ((retval = run([&]() { hipLaunchKernelGGL(PointKernel, step_grid(a.count, tile), dim3(kMatchingThreads), 0, stream, c, cur, a.count, tile); })))
                return retval;
            if ((retval = run([&]() {
                     hipLaunchKernelGGL(MatchKernel, step_grid(a.count, util::kWaveSize), dim3(kMatchingThreads), 0, stream, c, cur, next, a.count);
                 })))
                return retval;
            if ((retval = read_words())) return retval;
            a.count = words[W_NEXT] < static_cast<unsigned>(n) ? words[W_NEXT] : static_cast<unsigned>(n);
            a.entries = words[W_NEXT_ENTRIES];
            a.cur ^= 1;
            ++sweeps;
            if (words[W_MATCHED] != a.matched) ++rounds;
            a.matched = words[W_MATCHED];
            trace(STEP_WIDE, 1, list, static_cast<long long>(a.matched - before));
        }

        if ((retval = step.Read(h_counters, ds->d_counters, sizeof(unsigned long long) * C_COUNT, stream))) return retval;
        entries_read = static_cast<long long>(h_counters[C_READS]);
        polls = static_cast<long long>(h_counters[C_POLLS]);
        Summary &out = problem->summary;
        out = Summary();
        out.pairs = M;
        out.matched = a.matched;
        out.weight = static_cast<long long>(h_counters[C_WEIGHT]);
        out.unmatched = n - 2 * out.matched;
        out.unmatched_with_neighbours = problem->with_neighbours - 2 * out.matched;
        problem->enacted = true;
        return retval;
    }
};

}  // namespace matching
}  // namespace app
}  // namespace gunrock
