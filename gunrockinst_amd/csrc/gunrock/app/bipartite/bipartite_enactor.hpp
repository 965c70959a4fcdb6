// app/bipartite/bipartite_enactor.hpp -- host side of the maximum bipartite matching: the schedule of bipartite_functor.hpp's searches.
//
// An Enact: the greedy start (option "greedy"), then phases -- RootsKernel, the levels of the forest from the unmatched columns until
// the first level that found an end, AugmentKernel -- until a phase finds none ("max_phases" > 0 caps them: BIPARTITE_CAPPED).  Behind
// the last phase its forest is marked as the horizontal part, one more search from the unmatched rows gives the vertical part, and
// CertKernel's counts are read back once: a result is only kept when they hold (else kNotCertified and no result).
// A level is a wide launch with one read-back, or one of a stretch inside LoopKernel (LoopOptions: "schedule", "loop_max_list",
// "loop_max_entries").  INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <vector>

#include <gunrock/app/bipartite/bipartite_functor.hpp>
#include <gunrock/app/bipartite/bipartite_problem.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace bipartite {

constexpr int kNotCertified = -4;  // GRX_BIPARTITE_NOT_CERTIFIED
constexpr int kNotMaximum = -6;    // GRX_BIPARTITE_NOT_MAXIMUM: the parts, the cover and the blocks of a capped run
constexpr long long kMaxMaxPhases = 1ll << 40;
constexpr int kStepWaves = kStepBlocks * kWaves;

enum { MS_ROOTS = 0, MS_LEVEL, MS_LOOP, MS_AUGMENT, MS_REST, MS_COUNT };  // the kernels an instrumented Enact times apart

// options (grx_bipartite_set_option) and what the host derives from them
struct BipartiteOptions {
    LoopOptions loop;  // "schedule", "wave_min_row", "loop_max_list", "loop_max_entries"
    int strategy = BIPARTITE_AUTO;
    int block_min_row = kBlockMinRow;
    int greedy = 1;
    long long max_phases = 0;

    // 0: set, 1: unknown name, -1: a value out of range
    int Set(const char *name, double value)
    {
        const long long v = Whole(value);
        if (!std::strcmp(name, "strategy")) {
            if (v < BIPARTITE_AUTO || v > BIPARTITE_BLOCK) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "block_min_row")) {
            if (v < 1) return -1;
            block_min_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else if (!std::strcmp(name, "greedy")) {
            if (v < 0 || v > 1) return -1;
            greedy = static_cast<int>(v);
        } else if (!std::strcmp(name, "max_phases")) {
            if (v < 0 || v > kMaxMaxPhases) return -1;
            max_phases = v;
        } else {
            return loop.Set(name, value);
        }
        return 0;
    }
    int RegimeOf(int len) const { return Regime(len, strategy, loop.wave_min_row, block_min_row); }
    // whether a level of `count` frontier vertices with `entries` entries runs in the device loop
    bool LevelInLoop(long long count, long long entries) const { return loop.InLoop(count, entries); }
    bool Capped(long long phases) const { return max_phases > 0 && phases >= max_phases; }
};

template <bool INSTRUMENT>
class BipartiteEnactor {
   public:
    BipartiteOptions options;

    // of the last Enact (step: its launches, read-backs and summed kernel time)
    StepHost<INSTRUMENT> step{"BipartiteEnactor"};
    long long size = 0, phases = 0, levels = 0, vertical_levels = 0, augmentations = 0, greedy_pairs = 0, loop_levels = 0;
    long long certificate[3] = {0, 0, 0}, regime[3] = {0, 0, 0};
    int state = BIPARTITE_MAXIMUM;
    int code = 0;  // 0 or kNotCertified: then there is no result
    double kind_ms[MS_COUNT] = {0, 0, 0, 0, 0};
    std::vector<int> trace_levels;       // one row per phase, then one for the vertical search
    std::vector<long long> trace_aug;
    std::vector<double> trace_ms;

    hipError_t Enact(BipartiteProblem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        // the run starts from the matching of the last Reset: an Enact that does not follow one starts from the empty matching
        if (!problem->fresh && (retval = problem->Reset(nullptr))) return retval;
        problem->fresh = false;
        problem->state = -1;
        problem->square_k = -1;
        hipStream_t stream = problem->stream;
        const int rows = problem->rows, cols = problem->cols, larger = problem->larger;
        size = phases = levels = vertical_levels = augmentations = greedy_pairs = loop_levels = 0;
        for (int i = 0; i < 3; ++i) certificate[i] = regime[i] = 0;
        for (double &ms : kind_ms) ms = 0;
        state = BIPARTITE_MAXIMUM;
        code = 0;
        trace_levels.clear();
        trace_aug.clear();
        trace_ms.clear();
        if ((retval = step.Begin(kPinnedBytes))) return retval;
        auto run = [&](int kind, auto launch) {
            const double before = step.kernel_ms;
            const hipError_t result = step.Run(stream, launch);
            kind_ms[kind] += step.kernel_ms - before;
            return result;
        };
        unsigned *words = reinterpret_cast<unsigned *>(step.pinned + kPinnedWords);
        Front *h_front = reinterpret_cast<Front *>(step.pinned + kPinnedFront);
        unsigned long long *h_counts = reinterpret_cast<unsigned long long *>(step.pinned + kPinnedCounts);
        auto read_words = [&]() { return step.Read(words, problem->d_words, sizeof(unsigned) * W_COUNT, stream); };
        const dim3 block(kThreads);
        const Limits lim = options.loop.LimitsFor();

        Ctx from_cols;
        from_cols.ro = problem->t.ro, from_cols.ci = problem->t.ci;
        from_cols.mate_u = problem->d_mate_col, from_cols.mate_w = problem->d_mate_row;
        from_cols.pred = problem->d_pred, from_cols.root = problem->d_root, from_cols.winner = problem->d_winner, from_cols.queue = problem->d_queue;
        from_cols.words = problem->d_words, from_cols.counts = problem->d_counts;
        from_cols.n_u = cols, from_cols.n_w = rows, from_cols.cap = larger;
        from_cols.strategy = options.strategy, from_cols.wave_min_row = options.loop.wave_min_row, from_cols.block_min_row = options.block_min_row;
        Ctx from_rows = from_cols;
        from_rows.ro = problem->a.ro, from_rows.ci = problem->a.ci;
        from_rows.mate_u = problem->d_mate_row, from_rows.mate_w = problem->d_mate_col;
        from_rows.n_u = rows, from_rows.n_w = cols;

        GR_CHECK(hipMemsetAsync(problem->d_counts, 0, sizeof(unsigned long long) * C_COUNT, stream), "BipartiteEnactor memset failed");
        if ((retval = run(MS_REST, [&]() {
                 hipLaunchKernelGGL(oprtr::FillKernel<int>, GridFor(rows, max_grid_size), block, 0, stream, problem->d_row_part.p,
                                    static_cast<long long>(rows), static_cast<int>(BIPARTITE_SQUARE));
             })))
            return retval;
        if ((retval = run(MS_REST, [&]() {
                 hipLaunchKernelGGL(oprtr::FillKernel<int>, GridFor(cols, max_grid_size), block, 0, stream, problem->d_col_part.p,
                                    static_cast<long long>(cols), static_cast<int>(BIPARTITE_SQUARE));
             })))
            return retval;
        if (options.greedy &&
            (retval = run(MS_REST, [&]() { hipLaunchKernelGGL(GreedyKernel, GridFor(rows, max_grid_size), block, 0, stream, problem->DeviceSides(), problem->d_words.p); })))
            return retval;

        // one search: the forest from every unmatched vertex of c's side, until its frontier is empty or (stop_on_end) a level found an end
        unsigned roots = 0;
        auto search = [&](const Ctx &c, bool stop_on_end, Front &s) -> hipError_t {
            hipError_t retval = hipSuccess;
            GR_CHECK(hipMemsetAsync(problem->d_words, 0, sizeof(unsigned) * (W_FOUND + 1), stream), "BipartiteEnactor memset failed");
            const long long most = c.n_u > c.n_w ? c.n_u : c.n_w;
            if ((retval = run(MS_ROOTS, [&]() { hipLaunchKernelGGL(RootsKernel, GridFor(most, max_grid_size), block, 0, stream, c); }))) return retval;
            if ((retval = read_words())) return retval;
            roots = words[W_TAIL];
            s = Front{0, 0u, words[W_TAIL], words[W_ENTRIES], words[W_ENTRIES], 0u};
            while (s.head < s.tail && !(stop_on_end && s.found)) {
                const long long count = s.tail - s.head;
                if (options.LevelInLoop(count, s.step_entries)) {
                    const int before = s.level;
                    if ((retval = run(MS_LOOP, [&]() {
                             hipLaunchKernelGGL(LoopKernel, dim3(1), dim3(kLoopThreads), 0, stream, c, s, lim, stop_on_end ? 1 : 0, problem->d_front.p);
                         })))
                        return retval;
                    if ((retval = step.Read(h_front, problem->d_front, sizeof(Front), stream))) return retval;
                    s = *h_front;
                    loop_levels += s.level - before;
                    continue;
                }
                const int tile = TileFor(count, kStepWaves, s.step_entries);
                if ((retval = run(MS_LEVEL, [&]() {
                         hipLaunchKernelGGL(StepKernel, StepGrid(count, tile, kWaves, max_grid_size), block, 0, stream, c, s.head, s.tail, tile);
                     })))
                    return retval;
                if ((retval = read_words())) return retval;
                ++s.level;
                s.head = s.tail;
                s.tail = words[W_TAIL];
                s.step_entries = words[W_ENTRIES] - s.entries_seen;
                s.entries_seen = words[W_ENTRIES];
                s.found = words[W_FOUND];
            }
            return retval;
        };
        auto now = []() { return std::chrono::steady_clock::now(); };
        auto since = [](std::chrono::steady_clock::time_point t0) {
            return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        };

        // ---- the phases ----
        Front s{};
        long long flipped_seen = 0;
        bool pending = false;  // the last phase's augmentations have not been read back
        for (;;) {
            const auto t0 = now();
            if ((retval = search(from_cols, true, s))) return retval;
            if (pending) {  // (this search's first read-back brought them)
                trace_aug.back() = static_cast<long long>(words[W_AUG]) - flipped_seen;
                flipped_seen = words[W_AUG];
                pending = false;
            }
            if (phases == 0) greedy_pairs = words[W_GREEDY];
            ++phases;
            levels += s.level;
            trace_levels.push_back(s.level);
            trace_aug.push_back(0);
            if (s.found) {
                if ((retval = run(MS_AUGMENT, [&]() { hipLaunchKernelGGL(AugmentKernel, GridFor(roots, max_grid_size), block, 0, stream, from_cols, roots); })))
                    return retval;
                pending = true;
            }
            trace_ms.push_back(since(t0));
            if (!s.found) break;
            if (options.Capped(phases)) {
                state = BIPARTITE_CAPPED;
                break;
            }
        }
        if (pending) {
            if ((retval = read_words())) return retval;
            trace_aug.back() = static_cast<long long>(words[W_AUG]) - flipped_seen;
            flipped_seen = words[W_AUG];
        }
        augmentations = flipped_seen;

        // ---- the parts and the certificate ----
        long long stray_ends = 0;
        if (state == BIPARTITE_MAXIMUM) {
            const auto t0 = now();
            if ((retval = run(MS_REST, [&]() {
                     hipLaunchKernelGGL(MarkKernel, GridFor(larger, max_grid_size), block, 0, stream, from_cols, s.tail, static_cast<int>(BIPARTITE_HORIZONTAL),
                                        problem->d_col_part.p, problem->d_row_part.p);
                 })))
                return retval;
            Front v{};
            if ((retval = search(from_rows, false, v))) return retval;
            vertical_levels = v.level;
            stray_ends = v.found;
            if ((retval = run(MS_REST, [&]() {
                     hipLaunchKernelGGL(MarkKernel, GridFor(larger, max_grid_size), block, 0, stream, from_rows, v.tail, static_cast<int>(BIPARTITE_VERTICAL),
                                        problem->d_row_part.p, problem->d_col_part.p);
                 })))
                return retval;
            trace_levels.push_back(v.level);
            trace_aug.push_back(0);
            trace_ms.push_back(since(t0));
        }
        if ((retval = run(MS_REST, [&]() {
                 hipLaunchKernelGGL(CertKernel, GridFor(larger, max_grid_size), block, 0, stream, problem->DeviceSides(), problem->d_row_part.p,
                                    problem->d_col_part.p, problem->d_row_cover.p, problem->d_col_cover.p, state == BIPARTITE_MAXIMUM ? 1 : 0,
                                    problem->d_counts.p);
             })))
            return retval;
        if ((retval = step.Read(h_counts, problem->d_counts, sizeof(unsigned long long) * C_COUNT, stream))) return retval;
        size = static_cast<long long>(h_counts[C_SIZE]);
        certificate[0] = static_cast<long long>(h_counts[C_BAD_PAIRS]);
        certificate[1] = static_cast<long long>(h_counts[C_UNCOVERED]) + stray_ends;
        certificate[2] = static_cast<long long>(h_counts[C_COVER]);
        for (int i = 0; i < 3; ++i) regime[i] = static_cast<long long>(h_counts[C_REGIME + i]);
        const bool maximum = state == BIPARTITE_MAXIMUM;
        if (certificate[0] || (maximum && (certificate[1] || certificate[2] != size))) {
            code = kNotCertified;
            return retval;
        }
        problem->state = state;
        problem->size = size;
        for (int i = 0; i < 6; ++i) problem->part_size[i] = maximum ? static_cast<long long>(h_counts[C_PART + i]) : 0;
        return retval;
    }
};

}  // namespace bipartite
}  // namespace app
}  // namespace gunrock
