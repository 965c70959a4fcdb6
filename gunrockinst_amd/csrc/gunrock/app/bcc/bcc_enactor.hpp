// app/bcc/bcc_enactor.hpp -- host side of the biconnected components: the schedule of bcc_functor.hpp's steps.
//
// Four chains of steps, each as long as the forest is deep: the search (its levels are found as it runs: a read-back of two words per
// launch), then sizes (bottom-up), numbering (top-down) and low/high (bottom-up) over levels whose ranges are known, so they are
// launched without a read-back.  Three schedules:
//   ROUNDS       every level is a wide launch (StepKernel)
//   DEVICE_LOOP  every level runs in the one-workgroup loop on the device (at most kLoopMaxSteps per launch)
//   AUTO         a stretch of narrow levels (Narrow(): loop_max_list vertices, loop_max_entries row entries) is one loop launch,
//                a wide level is a launch of its own
// The link and label passes behind the chains are one wide launch each.  INSTRUMENT times every kernel with HIP events (and waits
// for each).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <type_traits>
#include <vector>

#include <gunrock/app/bcc/bcc_functor.hpp>
#include <gunrock/app/bcc/bcc_problem.hpp>
#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace bcc {

constexpr int kStepWavesPerBlock = kBccThreads / util::kWaveSize;
constexpr int kStepWaves = kStepBlocks * kStepWavesPerBlock;
static_assert(BCC_AUTO == SCHEDULE_AUTO && BCC_ROUNDS == SCHEDULE_ROUNDS && BCC_DEVICE_LOOP == SCHEDULE_DEVICE_LOOP, "LoopOptions' schedules");

template <bool INSTRUMENT>
class BccEnactor : public EnactorBase {
   public:
    explicit BccEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    LoopOptions loop;  // options (grx_bcc_set_option)

    // of the last Enact (step: its launches, read-backs and summed kernel time)
    StepHost<INSTRUMENT> step{"BccEnactor"};
    long long trees = 0, levels = 0, entries_read = 0;
    std::vector<long long> trace_items;  // one row per phase: the vertices or edges it touched,
    std::vector<double> trace_ms;        // and the time to the next phase's start (the device's constant-rate counter)

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        if (!problem->fresh && (retval = problem->Reset())) return retval;
        problem->fresh = false;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, M = problem->simple_edges;
        trees = levels = entries_read = 0;
        trace_items.assign(PHASE_COUNT, 0);
        trace_ms.assign(PHASE_COUNT, 0.0);
        // pinned: the words, LoopKernel's front, the counters and the clocks
        if ((retval = step.Begin(256))) return retval;
        auto run = [&](auto launch) { return step.Run(stream, launch); };
        auto stamp = [&](int phase) { return step.Stamp(ds->d_clock + phase, stream); };
        auto grid_for = [&](long long work) { return GridFor(work, max_grid_size); };
        auto step_grid = [&](long long count, int tile) { return StepGrid(count, tile, kStepWavesPerBlock, max_grid_size); };

        const Ctx c = problem->DeviceCtx(loop.wave_min_row);
        const Tree tr = problem->DeviceTree();
        const Limits lim = loop.LimitsFor();
        unsigned *words = reinterpret_cast<unsigned *>(step.pinned);
        Front *h_front = reinterpret_cast<Front *>(step.pinned + 32);
        unsigned long long *h_counters = reinterpret_cast<unsigned long long *>(step.pinned + 64);  // 8, then PHASE_COUNT + 1 clocks
        unsigned long long *h_clock = h_counters + 8;

        // ---- forest ----
        if ((retval = stamp(PHASE_FOREST))) return retval;
        if (M > 0) {
            if ((retval = run([&]() { hipLaunchKernelGGL(scc::IotaKernel, grid_for(n), dim3(256), 0, stream, ds->d_uf, n); }))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(UniteEdgesKernel, grid_for(M), dim3(256), 0, stream, ds->d_src, ds->d_dst, M, ds->d_uf); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(CompressKernel, grid_for(n), dim3(256), 0, stream, ds->d_uf, n, ds->d_comp); }))) return retval;
        } else {
            if ((retval = run([&]() { hipLaunchKernelGGL(scc::IotaKernel, grid_for(n), dim3(256), 0, stream, ds->d_comp, n); }))) return retval;
        }
        if ((retval = run([&]() { hipLaunchKernelGGL(RootsKernel, grid_for(n), dim3(256), 0, stream, c, ds->d_comp); }))) return retval;
        if ((retval = step.Read(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream))) return retval;
        trees = words[W_TAIL];
        Front s = {0, 0u, words[W_TAIL], words[W_ENTRIES], words[W_ENTRIES]};
        while (s.head < s.tail) {
            const long long count = s.tail - s.head;
            if (loop.InLoop(count, s.step_entries)) {
                if ((retval = run([&]() { hipLaunchKernelGGL(ForestLoopKernel, dim3(1), dim3(kLoopThreads), 0, stream, c, s, lim, ds->d_front); })))
                    return retval;
                if ((retval = step.Read(h_front, ds->d_front, sizeof(Front), stream))) return retval;
                s = *h_front;
                continue;
            }
            const int tile = TileFor(count, kStepWaves, s.step_entries);
            if ((retval = run([&]() {
                     hipLaunchKernelGGL(StepKernel<K_FOREST>, step_grid(count, tile), dim3(kBccThreads), 0, stream, c, s.level, s.head, s.tail,
                                        s.entries_seen, tile);
                 })))
                return retval;
            if ((retval = step.Read(words, ds->d_words, sizeof(unsigned) * W_COUNT, stream))) return retval;
            ++s.level;
            s.head = s.tail;
            s.tail = words[W_TAIL];
            s.step_entries = words[W_ENTRIES] - s.entries_seen;
            s.entries_seen = words[W_ENTRIES];
        }
        levels = s.level;  // (the level that came out empty is none)
        const long long reached = s.tail;
        trace_items[PHASE_FOREST] = reached;

        // the level table, for the three chains behind the search
        std::vector<int> bounds(static_cast<size_t>(levels) + 1, 0);
        std::vector<unsigned> ents(static_cast<size_t>(levels) + 1, 0u);
        if (levels > 0) {
            if ((retval = step.Copy(bounds.data(), ds->d_bounds, sizeof(int) * bounds.size(), stream))) return retval;
            if ((retval = step.Read(ents.data(), ds->d_ents, sizeof(unsigned) * ents.size(), stream))) return retval;
        }
        auto width = [&](long long L) { return static_cast<long long>(bounds[L + 1]) - bounds[L]; };
        auto weight = [&](long long L) { return static_cast<long long>(ents[L + 1] - ents[L]); };
        auto in_loop = [&](long long L) { return loop.InLoop(width(L), weight(L)); };

        // one chain: the levels from `first` on in direction dir
        auto chain = [&](auto kind, int dir) -> hipError_t {
            constexpr int KIND = decltype(kind)::value;
            hipError_t retval = hipSuccess;
            long long L = dir > 0 ? 0 : levels - 1;
            auto inside = [&](long long l) { return l >= 0 && l < levels; };
            while (inside(L)) {
                if (in_loop(L)) {
                    int count = 0;
                    while (inside(L + static_cast<long long>(count) * dir) && count < kLoopMaxSteps && in_loop(L + static_cast<long long>(count) * dir)) ++count;
                    const int first = static_cast<int>(L);
                    if ((retval = run([&]() { hipLaunchKernelGGL(ChainLoopKernel<KIND>, dim3(1), dim3(kLoopThreads), 0, stream, c, first, count, dir); })))
                        return retval;
                    L += static_cast<long long>(count) * dir;
                    continue;
                }
                const int tile = TileFor(width(L), kStepWaves, weight(L));
                const int level = static_cast<int>(L);
                if ((retval = run([&]() {
                         hipLaunchKernelGGL(StepKernel<KIND>, step_grid(width(level), tile), dim3(kBccThreads), 0, stream, c, level,
                                            static_cast<unsigned>(bounds[level]), static_cast<unsigned>(bounds[level + 1]), 0u, tile);
                     })))
                    return retval;
                L += dir;
            }
            return retval;
        };
        if ((retval = stamp(PHASE_SIZES))) return retval;
        if ((retval = chain(std::integral_constant<int, K_SIZES>(), -1))) return retval;
        trace_items[PHASE_SIZES] = reached;
        if ((retval = stamp(PHASE_NUMBER))) return retval;
        if ((retval = chain(std::integral_constant<int, K_NUMBER>(), 1))) return retval;
        trace_items[PHASE_NUMBER] = reached;
        if ((retval = stamp(PHASE_LOWHIGH))) return retval;
        if ((retval = chain(std::integral_constant<int, K_LOWHIGH>(), -1))) return retval;
        trace_items[PHASE_LOWHIGH] = reached;

        // ---- link: the bridges and the union-find over the tree edges ----
        if ((retval = stamp(PHASE_LINK))) return retval;
        if (M > 0) {
            if ((retval = run([&]() { hipLaunchKernelGGL(BridgeKernel, grid_for(n), dim3(256), 0, stream, tr, n, ds->d_bridge); }))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(scc::IotaKernel, grid_for(n), dim3(256), 0, stream, ds->d_uf, n); }))) return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(LinkKernel, grid_for(M), dim3(256), 0, stream, tr, ds->d_src, ds->d_dst, M, ds->d_uf); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(CompressKernel, grid_for(n), dim3(256), 0, stream, ds->d_uf, n, ds->d_set); }))) return retval;
        }
        trace_items[PHASE_LINK] = M;

        // ---- label: block ids and sizes, articulation points, 2-edge-connected components, the summary ----
        if ((retval = stamp(PHASE_LABEL))) return retval;
        if (M > 0) {
            if ((retval = run([&]() { hipLaunchKernelGGL(EdgeSetKernel, grid_for(M), dim3(256), 0, stream, tr, ds->d_src, ds->d_dst, M, ds->d_set, ds->d_bcc); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(oprtr::FillKernel<int>, grid_for(n), dim3(256), 0, stream, ds->d_min_of, n, INT_MAX); }))) return retval;
            GR_CHECK(hipMemsetAsync(ds->d_cnt_of, 0, sizeof(int) * static_cast<size_t>(n), stream), "BccEnactor memset failed");
            if ((retval = run([&]() { hipLaunchKernelGGL(scc::MergeKernel<false>, grid_for(M), dim3(256), 0, stream, ds->d_bcc, M, ds->d_min_of); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(scc::MergeKernel<true>, grid_for(M), dim3(256), 0, stream, ds->d_bcc, M, ds->d_cnt_of); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(scc::GatherKernel, grid_for(M), dim3(256), 0, stream, ds->d_bcc, M, ds->d_cnt_of, ds->d_bsize); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(scc::GatherKernel, grid_for(M), dim3(256), 0, stream, ds->d_bcc, M, ds->d_min_of, ds->d_bcc); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(FirstChildKernel, grid_for(n), dim3(256), 0, stream, tr, n, ds->d_set, ds->d_first); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(ArticulationKernel, grid_for(n), dim3(256), 0, stream, tr, n, ds->d_set, ds->d_first, ds->d_art); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(CountBytesKernel, grid_for(n), dim3(256), 0, stream, ds->d_art, n, ds->d_counters + 1); })))
                return retval;
            if ((retval = run([&]() { hipLaunchKernelGGL(scc::SummaryKernel, grid_for(M), dim3(256), 0, stream, ds->d_bcc, ds->d_bsize, M, ds->d_counters + 2); })))
                return retval;
        }
        // (d_min_of holds the cut forest, d_cnt_of each vertex's root in it; then d_min_of the smallest id per root and d_cnt_of the counts)
        if ((retval = run([&]() { hipLaunchKernelGGL(CutForestKernel, grid_for(n), dim3(256), 0, stream, tr, n, ds->d_bridge, ds->d_min_of); }))) return retval;
        if ((retval = run([&]() { hipLaunchKernelGGL(CompressKernel, grid_for(n), dim3(256), 0, stream, ds->d_min_of, n, ds->d_cnt_of); }))) return retval;
        if ((retval = run([&]() { hipLaunchKernelGGL(scc::IotaKernel, grid_for(n), dim3(256), 0, stream, ds->d_min_of, n); }))) return retval;
        if ((retval = run([&]() { hipLaunchKernelGGL(scc::MergeKernel<false>, grid_for(n), dim3(256), 0, stream, ds->d_cnt_of, n, ds->d_min_of); }))) return retval;
        if ((retval = run([&]() { hipLaunchKernelGGL(scc::GatherKernel, grid_for(n), dim3(256), 0, stream, ds->d_cnt_of, n, ds->d_min_of, ds->d_tecc); })))
            return retval;
        GR_CHECK(hipMemsetAsync(ds->d_cnt_of, 0, sizeof(int) * static_cast<size_t>(n), stream), "BccEnactor memset failed");
        if ((retval = run([&]() { hipLaunchKernelGGL(scc::MergeKernel<true>, grid_for(n), dim3(256), 0, stream, ds->d_tecc, n, ds->d_cnt_of); }))) return retval;
        if ((retval = run([&]() { hipLaunchKernelGGL(scc::GatherKernel, grid_for(n), dim3(256), 0, stream, ds->d_tecc, n, ds->d_cnt_of, ds->d_tsize); })))
            return retval;
        if ((retval = run([&]() { hipLaunchKernelGGL(scc::SummaryKernel, grid_for(n), dim3(256), 0, stream, ds->d_tecc, ds->d_tsize, n, ds->d_counters + 5); })))
            return retval;
        trace_items[PHASE_LABEL] = M + n;
        if ((retval = stamp(PHASE_COUNT))) return retval;

        // the counters and the clocks
        if ((retval = step.Copy(h_counters, ds->d_counters, sizeof(unsigned long long) * 8, stream))) return retval;
        if ((retval = step.Read(h_clock, ds->d_clock, sizeof(unsigned long long) * (PHASE_COUNT + 1), stream))) return retval;
        entries_read = static_cast<long long>(h_counters[0]);
        Summary &out = problem->summary;
        out = Summary();
        out.articulation_points = static_cast<long long>(h_counters[1]);
        out.blocks = static_cast<long long>(h_counters[2]);
        out.bridges = static_cast<long long>(h_counters[3]);  // (the blocks of one edge)
        out.largest_block = static_cast<long long>(h_counters[4] >> 32);
        if (out.blocks) out.largest_block_id = static_cast<int>(0xFFFFFFFFu - static_cast<unsigned>(h_counters[4] & 0xFFFFFFFFull));
        out.tecc_components = static_cast<long long>(h_counters[5]);
        out.largest_tecc = static_cast<long long>(h_counters[7] >> 32);
        if (out.tecc_components) out.largest_tecc_root = static_cast<int>(0xFFFFFFFFu - static_cast<unsigned>(h_counters[7] & 0xFFFFFFFFull));
        int khz = 0, device = 0;
        GR_CHECK(hipGetDevice(&device), "BccEnactor hipGetDevice failed");
        GR_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device), "BccEnactor clock rate failed");
        for (int i = 0; i < PHASE_COUNT; ++i)
            trace_ms[i] = khz > 0 && h_clock[i + 1] >= h_clock[i] ? static_cast<double>(h_clock[i + 1] - h_clock[i]) / static_cast<double>(khz) : 0.0;
        problem->enacted = true;
        return retval;
    }
};

}  // namespace bcc
}  // namespace app
}  // namespace gunrock
