// app/lp/lp_enactor.hpp -- host side of label propagation: the schedule of lp_functor.hpp's rounds.
//
//   SYNC     a round is VoteKernel over the active list (HubKernel behind it when a row can reach the BLOCK regime), ApplyKernel,
//            which moves the votes into L[] and compacts the next list, and one read-back
//   CLASSES  a round is one VoteKernel per non-empty class, in class order, over that class's list (HubKernel behind it when a row of
//            the class can reach the BLOCK regime), and one read-back behind the last class
// An Enact ends LP_CONVERGED behind a round that changed nothing, LP_PERIOD2 (SYNC) behind a round r >= 2 whose changed vertices are
// those of round r - 1 and all went back to their label of two rounds ago, or LP_CAPPED behind round max_rounds.  `rounds` counts
// the rounds that changed a label.  Nothing spins: no kernel waits on another workgroup and the host loop stops at max_rounds.
// INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/lp/lp_functor.hpp>
#include <gunrock/app/lp/lp_problem.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace lp {

constexpr int kVoteBlocks = 2048;  // 256 CUs x 8 workgroups
constexpr int kHubBlocks = 1024;
constexpr long long kMaxMaxRounds = 1ll << 30;

template <bool INSTRUMENT>
class LpEnactor : public EnactorBase {
   public:
    explicit LpEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    // options (grx_lp_set_option)
    int mode = LP_CLASSES;
    int strategy = LP_AUTO;
    int lane_max_row = kLaneMaxRow;
    int wave_max_row = kWaveMaxRow;
    int table_slots = kTableSlots;
    long long max_rounds = 0;  // 0: 2 n + 64 (a policy value)

    // of the last Enact (step: its launches, read-backs and summed kernel time)
    StepHost<INSTRUMENT> step{"LpEnactor"};
    long long rounds = 0, visits = 0, entries_read = 0, regime_rows[3] = {0, 0, 0}, fallback_rows = 0;
    int state = LP_CONVERGED;
    std::vector<long long> trace_list, trace_changed;  // per round: the vertices visited and the labels changed

    // hipSuccess or a hipError_t (hipErrorNotReady: CLASSES without classes)
    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        if (mode == LP_CLASSES && problem->classes < 1) return hipErrorNotReady;
        if (!problem->fresh && (retval = problem->Reset())) return retval;
        problem->fresh = false;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes;
        rounds = visits = entries_read = fallback_rows = 0;
        regime_rows[0] = regime_rows[1] = regime_rows[2] = 0;
        state = LP_CONVERGED;
        trace_list.clear();
        trace_changed.clear();
        if ((retval = step.Begin(sizeof(unsigned long long) * W_COUNT))) return retval;
        auto run = [&](auto launch) { return step.Run(stream, launch); };
        auto grid = [&](long long count, int per_block, int most) {
            long long blocks = (count + per_block - 1) / per_block;
            if (blocks > most) blocks = most;
            if (max_grid_size > 0 && blocks > max_grid_size) blocks = max_grid_size;
            if (blocks < 1) blocks = 1;
            return dim3(static_cast<unsigned>(blocks));
        };

        const Ctx c = problem->DeviceCtx(strategy, lane_max_row, wave_max_row, table_slots);
        const size_t lds = static_cast<size_t>(kLpWaves) * table_slots * (sizeof(unsigned long long) + sizeof(int));
        // can a row of `longest` entries reach HubKernel?
        auto hubs_from = [&](int longest) { return longest > 0 && Regime(longest, strategy, lane_max_row, wave_max_row) == LP_BLOCK; };
        // the votes of one list: VoteKernel, and HubKernel behind it for what it left in hubs[]
        auto vote = [&](bool sync, const int *list, long long count, int longest) -> hipError_t {
            hipError_t retval = hipSuccess;
            if ((retval = run([&]() {
                     if (sync) hipLaunchKernelGGL(VoteKernel<true>, grid(count, kLpThreads, kVoteBlocks), dim3(kLpThreads), lds, stream, c, list, count);
                     else hipLaunchKernelGGL(VoteKernel<false>, grid(count, kLpThreads, kVoteBlocks), dim3(kLpThreads), lds, stream, c, list, count);
                 })))
                return retval;
            if (!hubs_from(longest)) return retval;
            if ((retval = run([&]() {
                     if (sync) hipLaunchKernelGGL(HubKernel<true>, grid(count, 1, kHubBlocks), dim3(kLpThreads), lds, stream, c, count);
                     else hipLaunchKernelGGL(HubKernel<false>, grid(count, 1, kHubBlocks), dim3(kLpThreads), lds, stream, c, count);
                 })))
                return retval;
            GR_CHECK(hipMemsetAsync(ds->d_words + W_HUBS, 0, sizeof(unsigned long long), stream), "LpEnactor memset failed");
            return retval;
        };

        const long long bound = max_rounds > 0 ? max_rounds : 2 * n + 64;
        unsigned long long *h_words = reinterpret_cast<unsigned long long *>(step.pinned);
        auto read_words = [&]() { return step.Read(h_words, ds->d_words, sizeof(unsigned long long) * W_COUNT, stream); };

        long long count = n, changed_before = 0, visits_before = 0;
        int cur = 0;
        for (long long r = 1;; ++r) {
            GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * kRoundWords, stream), "LpEnactor memset failed");
            if (mode == LP_SYNC) {
                if ((retval = vote(true, ds->d_list[cur], count, problem->longest_row))) return retval;
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(ApplyKernel, grid(count, kLpThreads, kVoteBlocks), dim3(kLpThreads), 0, stream, c, ds->d_list[cur], count,
                                            ds->d_list[cur ^ 1], static_cast<int>(r));
                     })))
                    return retval;
            } else {
                for (int k = 0; k < problem->classes; ++k) {
                    const int from = problem->class_off[k], size = problem->class_off[k + 1] - from;
                    if (size > 0 && (retval = vote(false, ds->d_class_list + from, size, problem->class_longest[k]))) return retval;
                }
            }
            if ((retval = read_words())) return retval;
            const long long changed = static_cast<long long>(h_words[W_CHANGED]);
            trace_list.push_back(static_cast<long long>(h_words[W_VISITS]) - visits_before);
            trace_changed.push_back(changed);
            visits_before = static_cast<long long>(h_words[W_VISITS]);
            if (changed == 0) {
                state = LP_CONVERGED;
                break;
            }
            ++rounds;
            if (mode == LP_SYNC && r >= 2 && changed == changed_before && static_cast<long long>(h_words[W_RETURNED]) == changed) {
                state = LP_PERIOD2;
                break;
            }
            if (r >= bound) {
                state = LP_CAPPED;
                break;
            }
            changed_before = changed;
            count = static_cast<long long>(h_words[W_NEXT]) < n ? static_cast<long long>(h_words[W_NEXT]) : n;
            cur ^= 1;
        }

        if ((retval = problem->Finish())) return retval;
        if ((retval = read_words())) return retval;
        visits = static_cast<long long>(h_words[W_VISITS]);
        entries_read = static_cast<long long>(h_words[W_ENTRIES]);
        for (int i = 0; i < 3; ++i) regime_rows[i] = static_cast<long long>(h_words[W_REGIME + i]);
        fallback_rows = static_cast<long long>(h_words[W_FALLBACK]);
        problem->communities = static_cast<long long>(h_words[W_COMMUNITIES]);
        problem->enacted = true;
        return retval;
    }
};

}  // namespace lp
}  // namespace app
}  // namespace gunrock
