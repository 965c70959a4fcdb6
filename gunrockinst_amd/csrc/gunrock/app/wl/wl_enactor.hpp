// app/wl/wl_enactor.hpp -- host side of colour refinement: the loop over wl_functor.hpp's rounds.
//
// The start grouping by the labels is round 0.  A round is SigKernel (SigWaveKernel and SigHubKernel behind it when a row can reach
// the WAVE or the BLOCK regime), GroupKernel, AssignKernel, the certificate kernels and one read-back of the words.  `attempt`
// counts the signature passes and is mixed into every signature, so no two passes hash alike.
//   max_rounds < 0   rounds are committed as they come until one splits nothing (the class count stays); that round is certified
//                    (the kernels are gated on the count, so the host need not read it first).  Passed: WL_STABLE.  Failed: a
//                    repair, and the refinement goes on.  Hashing only ever merges, so the working partition stays coarser than or
//                    equal to the coarsest equitable one, and an equitable partition that is coarser than or equal to it is it.
//   max_rounds >= 0  the result is the colouring after exactly that many rounds (or the stable one, if that comes first), so every
//                    round is certified before it is committed and attempted again when it fails: the next attempt groups by
//                    (the refused attempt's group, a fresh signature), so what one attempt told apart stays apart and a class that
//                    has to fall into more parts than sig_bits can name still gets there.  WL_CAPPED behind round max_rounds.
//                    With "history" (max_rounds in 1 .. 64) every committed round is kept.
// More than max_repairs repairs end the Enact with kNotCertified and no result.  WlOptions is plain C++ a host-only program can
// call.  INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/table_ladder.hpp>
#include <gunrock/app/wl/wl_functor.hpp>
#include <gunrock/app/wl/wl_problem.hpp>

namespace gunrock {
namespace app {
namespace wl {

constexpr int kTooLarge = -4;      // GRX_WL_TOO_LARGE
constexpr int kNotCertified = -5;  // GRX_WL_NOT_CERTIFIED
constexpr int kSigBlocks = 2048;   // 256 CUs x 8 workgroups
constexpr int kHubBlocks = 1024;
constexpr long long kMaxMaxRounds = 1ll << 30;
constexpr long long kMaxMaxRepairs = 1ll << 30;
constexpr int kMaxHistoryRounds = 64;
constexpr int kMaxRepairs = 64;  // default "max_repairs"

// options (grx_wl_set_option) and what the host derives from them
struct WlOptions {
    int strategy = WL_AUTO;
    int lane_max_row = kLaneMaxRow;
    int wave_max_row = kWaveMaxRow;
    long long max_rounds = -1;
    long long max_repairs = kMaxRepairs;
    int history = 0;
    int sig_bits = 128;
    uint64_t seed = 0;
    ladder::TableOptions table;  // "table_slots", "block_slots", "scratch_mib"

    // 0: set, 1: unknown name, -1: a value out of range
    int Set(const char *name, double value)
    {
        if (!(value == value)) return Known(name) ? -1 : 1;  // (NaN)
        const long long v = Whole(value);
        if (!std::strcmp(name, "strategy")) {
            if (v < WL_AUTO || v > WL_BLOCK) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "lane_max_row")) {
            if (v < 0) return -1;
            lane_max_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else if (!std::strcmp(name, "wave_max_row")) {
            if (v < 0) return -1;
            wave_max_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else if (!std::strcmp(name, "max_rounds")) {
            if (v < -1 || v > kMaxMaxRounds) return -1;
            max_rounds = v;
        } else if (!std::strcmp(name, "max_repairs")) {
            if (v < 0 || v > kMaxMaxRepairs) return -1;
            max_repairs = v;
        } else if (!std::strcmp(name, "history")) {
            if (v < 0 || v > 1) return -1;
            history = static_cast<int>(v);
        } else if (!std::strcmp(name, "sig_bits")) {
            if (v < 1 || v > 128) return -1;
            sig_bits = static_cast<int>(v);
        } else if (!std::strcmp(name, "seed")) {
            if (value < 0 || value >= 18446744073709551616.0) return -1;
            seed = static_cast<uint64_t>(value);
        } else {
            return table.Set(name, value);
        }
        return 0;
    }
    static bool Known(const char *name)
    {
        static const char *names[] = {"strategy", "lane_max_row", "wave_max_row", "max_rounds", "max_repairs", "history", "sig_bits", "seed",
                                      "table_slots", "block_slots", "scratch_mib"};
        for (const char *n : names)
            if (!std::strcmp(name, n)) return true;
        return false;
    }

    // history asks for max_rounds in 1 .. 64
    bool HistoryValid() const { return !history || (max_rounds >= 1 && max_rounds <= kMaxHistoryRounds); }
    // (max_rounds + 1) n colours within int32 offsets
    bool HistoryFits(long long nodes) const { return !history || (max_rounds + 1) * nodes <= 0x7FFFFFFFll; }
    bool CertifyAll() const { return max_rounds >= 0; }
    // (a forced strategy sends every row one way; else a row longer than lane_max_row can be a wave's)
    bool AnyWave(int longest) const
    {
        return longest > 0 && (strategy == WL_WAVE || (strategy == WL_AUTO && longest > lane_max_row && wave_max_row > lane_max_row));
    }
    bool AnyHub(int longest) const { return longest > 0 && Regime(longest, strategy, lane_max_row, wave_max_row) == WL_BLOCK; }
    // Rung() never falls as a row grows: the rung of the longest row tells which kernels a graph can need
    bool AnyBlock(int longest) const { return longest > 0 && Rung(longest, table.table_slots, table.block_slots) >= WL_RUNG_BLOCK; }
    bool AnyGlobal(int longest) const { return longest > 0 && Rung(longest, table.table_slots, table.block_slots) == WL_RUNG_GLOBAL; }
};

template <bool INSTRUMENT>
class WlEnactor : public EnactorBase {
   public:
    explicit WlEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    WlOptions options;

    // of the last Enact (step: its launches, read-backs and summed kernel time)
    StepHost<INSTRUMENT> step{"WlEnactor"};
    long long rounds = 0, repairs = 0, certificate_runs = 0, classes = 0, attempts = 0;
    long long regime_rows[3] = {0, 0, 0}, rung_rows[3] = {0, 0, 0};
    int state = WL_STABLE;
    int code = 0;  // 0, -1 (history without max_rounds in 1 .. 64), kTooLarge or kNotCertified: then there is no result
    std::vector<long long> trace_classes;  // the classes behind the start grouping and behind each committed round

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes;
        rounds = repairs = certificate_runs = classes = attempts = 0;
        for (int i = 0; i < 3; ++i) regime_rows[i] = rung_rows[i] = 0;
        state = WL_STABLE;
        code = 0;
        trace_classes.clear();
        problem->enacted = false;
        problem->history_rounds = -1;
        if (!options.HistoryValid()) {
            code = -1;
            return retval;
        }
        if (!options.HistoryFits(n)) {
            code = kTooLarge;
            return retval;
        }
        if ((retval = step.Begin(sizeof(unsigned long long) * W_COUNT))) return retval;
        auto run = [&](auto launch) { return step.Run(stream, launch); };
        auto grid = [&](long long blocks, int most) { return dim3(static_cast<unsigned>(CappedGrid(blocks, most, max_grid_size))); };
        const dim3 threads(kWlThreads);
        const dim3 wide = grid((n + kWlThreads - 1) / kWlThreads, kSigBlocks);
        unsigned long long *h_words = reinterpret_cast<unsigned long long *>(step.pinned);
        auto read_words = [&]() { return step.Read(h_words, ds->d_words, sizeof(unsigned long long) * W_COUNT, stream); };
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "WlEnactor memset failed");

        Ctx c;
        c.ro = problem->graph_slices[0]->d_row_offsets;
        c.ci = problem->graph_slices[0]->d_column_indices;
        c.sig = ds->d_sig;
        c.slot = ds->d_slot;
        c.owner = ds->d_owner;
        c.smallest = ds->d_smallest;
        c.waves = ds->d_waves;
        c.hubs = ds->d_hubs;
        c.block_list = ds->d_block_list;
        c.global_list = ds->d_global_list;
        c.words = ds->d_words;
        c.table_mask = problem->table_slots - 1;
        c.seed = options.seed;
        c.attempt = 0;
        c.nodes = static_cast<int>(n);
        c.strategy = options.strategy;
        c.lane_max_row = options.lane_max_row;
        c.wave_max_row = options.wave_max_row;
        c.sig_bits = options.sig_bits;
        c.table_slots = options.table.table_slots;
        c.block_slots = options.table.block_slots;
        c.vector_loads = (reinterpret_cast<uintptr_t>(c.ci) & 15) == 0;

        const bool keep = options.history != 0;
        if (keep && (retval = ds->history.Need(static_cast<size_t>(options.max_rounds + 1) * static_cast<size_t>(n)))) return retval;
        auto remember = [&](long long h, const int *colour) -> hipError_t {
            hipError_t retval = hipSuccess;
            if (!keep) return retval;
            GR_CHECK(hipMemcpyAsync(ds->history.p + static_cast<size_t>(h) * static_cast<size_t>(n), colour, sizeof(int) * static_cast<size_t>(n),
                                    hipMemcpyDeviceToDevice, stream),
                     "WlEnactor history copy failed");
            return retval;
        };

        // round 0: the classes of the labels
        int cur = 0, part = -1;  // d_colour[cur] is c; d_colour[part] what the refused attempts at this round have made of it
        c.colour = nullptr;
        c.key = problem->labelled ? ds->d_start : nullptr;
        c.fresh = ds->d_colour[cur];
        if ((retval = problem->ClearTable(stream))) return retval;
        if ((retval = run([&]() { hipLaunchKernelGGL(GroupKernel<true>, wide, threads, 0, stream, c); }))) return retval;
        if ((retval = run([&]() { hipLaunchKernelGGL(AssignKernel, wide, threads, 0, stream, c); }))) return retval;
        if ((retval = read_words())) return retval;
        classes = static_cast<long long>(h_words[W_CLASSES]);
        trace_classes.push_back(classes);
        if ((retval = remember(0, ds->d_colour[cur]))) return retval;

        const bool all = options.CertifyAll();
        const bool any_wave = options.AnyWave(problem->longest_row), any_hub = options.AnyHub(problem->longest_row);
        const bool any_block = options.AnyBlock(problem->longest_row), any_global = options.AnyGlobal(problem->longest_row);
        const size_t small_lds = options.table.SmallLdsBytes(kWlWaves);
        int global_blocks = 1;
        if (any_global) {
            global_blocks = static_cast<int>(options.table.Slots(CappedGrid(n, kHubBlocks, max_grid_size), n));
            if ((retval = ds->rows.NeedZeroed(static_cast<size_t>(global_blocks) * static_cast<size_t>(n), stream))) return retval;
        }
        if (any_block && (retval = AllowLds(reinterpret_cast<const void *>(&CertBlockKernel), ladder::TableOptions::kMaxBlockLdsBytes, &lds_opted)))
            return retval;

        state = options.max_rounds == 0 ? WL_CAPPED : WL_STABLE;
        while (options.max_rounds != 0) {
            c.attempt = static_cast<uint64_t>(++attempts);
            const int out = part < 0 ? (cur + 1) % 3 : 3 - cur - part;
            c.colour = ds->d_colour[cur];
            c.key = ds->d_colour[part < 0 ? cur : part];
            c.fresh = ds->d_colour[out];
            const long long gate = all ? -1 : classes;
            GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * kRoundWords, stream), "WlEnactor memset failed");
            if ((retval = problem->ClearTable(stream))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(SigKernel, wide, threads, 0, stream, c); }))) return retval;
            if (any_wave && (retval = run([&]() { hipLaunchKernelGGL(SigWaveKernel, grid((n + kWlWaves - 1) / kWlWaves, kSigBlocks), threads, 0, stream, c); })))
                return retval;
            if (any_hub && (retval = run([&]() { hipLaunchKernelGGL(SigHubKernel, grid(n, kHubBlocks), threads, 0, stream, c); }))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(GroupKernel<false>, wide, threads, 0, stream, c); }))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(AssignKernel, wide, threads, 0, stream, c); }))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(CertKernel, wide, threads, small_lds, stream, c, gate); }))) return retval;
            if (any_block && (retval = run([&]() {
                                  hipLaunchKernelGGL(CertBlockKernel, grid(n, kHubBlocks), threads, options.table.BlockLdsBytes(), stream, c, gate);
                              })))
                return retval;
            if (any_global &&
                (retval = run([&]() { hipLaunchKernelGGL(CertGlobalKernel, dim3(global_blocks), threads, 0, stream, c, gate, ds->rows.p); })))
                return retval;
            if ((retval = read_words())) return retval;
            const long long fresh_classes = static_cast<long long>(h_words[W_CLASSES]);
            const bool split = fresh_classes != classes;
            const bool certified = all || !split;
            if (certified) {
                ++certificate_runs;
                if (h_words[W_FAILS]) {  // the hash merged two multisets: again, under the next attempt
                    if (++repairs > options.max_repairs) {
                        code = kNotCertified;
                        return retval;
                    }
                    if (split) part = out;  // (what this attempt told apart stays apart)
                    continue;
                }
                if (!split) {
                    state = WL_STABLE;
                    break;
                }
            }
            cur = out;
            part = -1;
            classes = fresh_classes;
            ++rounds;
            trace_classes.push_back(classes);
            if ((retval = remember(rounds, ds->d_colour[cur]))) return retval;
            if (options.max_rounds > 0 && rounds >= options.max_rounds) {
                state = WL_CAPPED;
                break;
            }
        }
        for (int i = 0; i < 3; ++i) {
            regime_rows[i] = static_cast<long long>(h_words[W_REGIME + i]);
            rung_rows[i] = static_cast<long long>(h_words[W_RUNG + i]);
        }
        problem->current = cur;
        if ((retval = problem->Finish())) return retval;
        if (keep) problem->history_rounds = static_cast<int>(rounds);
        problem->enacted = true;
        return retval;
    }

   private:
    size_t lds_opted = 0;
};

}  // namespace wl
}  // namespace app
}  // namespace gunrock
