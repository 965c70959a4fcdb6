// app/msbfs/msbfs_enactor.hpp -- host side of the multi-source BFS: the batches, and the level loop of each.
//
// Batches of up to 64 sources run one after another on the same state.  A level is a push or a pull (msbfs_functor.hpp); the host
// reads five words back after each -- vertices reached, their out-row entries, the row entries of the vertices that every search
// of the batch has now reached, entries walked -- and chooses the next direction from them:
//   AUTO       push -> pull when frontier edges * alpha > unexplored edges, pull -> push when frontier vertices * beta < nodes
//              (the rule of the BFS's alpha / beta; "unexplored" counts the rows of the vertices some search has not reached,
//              which are the rows a pull walks)
//   PUSH / PULL / ALTERNATE   forced, for tests and measurements (ALTERNATE: odd levels push, even levels pull)
// Without in-neighbour lists every level is a push.  No direction changes a result.  INSTRUMENT times every level with HIP events
// (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/msbfs/msbfs_functor.hpp>
#include <gunrock/app/msbfs/msbfs_problem.hpp>
#include <gunrock/app/step_host.hpp>

namespace gunrock {
namespace app {
namespace msbfs {

constexpr int kPushWavesPerBlock = kThreads / util::kWaveSize;

template <bool INSTRUMENT>
class MsbfsEnactor : public EnactorBase {
   public:
    explicit MsbfsEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    // options (grx_msbfs_set_option)
    int direction = MSBFS_AUTO;
    double alpha = kAlpha, beta = kBeta;
    int wave_min_row = kWaveMinRow;

    // of the last Enact (step: its launches and, summed over the levels, their time)
    StepHost<INSTRUMENT> step{"MsbfsEnactor"};
    long long batches = 0, levels = 0, push_levels = 0, pull_levels = 0, entries_read = 0;
    std::vector<int> trace_batch, trace_level, trace_kind;        // one row per level: its batch, its depth, LEVEL_PUSH / LEVEL_PULL,
    std::vector<long long> trace_frontier, trace_edges;           // the frontier it started from: vertices and out-row entries,
    std::vector<double> trace_ms;                                 // and (INSTRUMENT) its time

    // *refused: Problem::SettleInverse's (an Enact that had to make its own Reset)
    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size, bool *refused)
    {
        hipError_t retval = hipSuccess;
        *refused = false;
        if (!problem->fresh && ((retval = problem->ResetAgain(refused)) || *refused)) return retval;
        problem->fresh = false;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, m = problem->edges;
        batches = levels = push_levels = pull_levels = entries_read = 0;
        trace_batch.clear();
        trace_level.clear();
        trace_kind.clear();
        trace_frontier.clear();
        trace_edges.clear();
        trace_ms.clear();
        if ((retval = step.Begin(sizeof(Word) * W_COUNT))) return retval;
        Word *h_words = reinterpret_cast<Word *>(step.pinned);
        auto cap = [&](long long blocks) {
            if (max_grid_size > 0 && blocks > max_grid_size) blocks = max_grid_size;
            return dim3(static_cast<unsigned>(blocks < 1 ? 1 : blocks));
        };
        auto clear_words = [&]() { return util::GRError(hipMemsetAsync(ds->d_words, 0, sizeof(Word) * W_COUNT, stream), "MsbfsEnactor memset failed", __FILE__, __LINE__); };
        auto read_words = [&]() { return step.Read(h_words, ds->d_words, sizeof(Word) * W_COUNT, stream); };

        const size_t state_bytes = sizeof(Word) * static_cast<size_t>(n);
        const dim3 block(kThreads);
        batches = problem->Batches();
        for (long long batch = 0; batch < batches; ++batch) {
            Ctx c = problem->DeviceCtx(batch, wave_min_row);
            const long long in_batch = static_cast<long long>(problem->sources.size()) - batch * kBatch;
            GR_CHECK(hipMemsetAsync(c.seen, 0, state_bytes, stream), "MsbfsEnactor memset failed");
            GR_CHECK(hipMemsetAsync(c.frontier, 0, state_bytes, stream), "MsbfsEnactor memset failed");
            GR_CHECK(hipMemsetAsync(c.next, 0, state_bytes, stream), "MsbfsEnactor memset failed");
            if ((retval = clear_words())) return retval;
            hipLaunchKernelGGL(InitKernel, dim3(1), dim3(kBatch), 0, stream, c, ds->d_sources + batch * kBatch, static_cast<int>(in_batch < kBatch ? in_batch : kBatch));
            GR_CHECK(hipGetLastError(), "InitKernel launch failed");
            ++step.launches;
            if ((retval = read_words())) return retval;
            long long count = static_cast<long long>(h_words[W_NEW]);
            long long frontier_edges = static_cast<long long>(h_words[W_FRONTIER_EDGES]);
            long long full_edges = static_cast<long long>(h_words[W_FULL_EDGES]);
            bool queued = true;      // queue_in holds the frontier
            bool next_clean = true;  // next[] is all zero
            bool pulling = false;
            for (int level = 1; count > 0; ++level) {
                bool pull = false;
                if (c.iro) {
                    if (direction == MSBFS_PULL) pull = true;
                    else if (direction == MSBFS_ALTERNATE) pull = level % 2 == 0;
                    else if (direction == MSBFS_AUTO)
                        pull = pulling ? !(static_cast<double>(count) * beta < static_cast<double>(n))
                                       : static_cast<double>(frontier_edges) * alpha > static_cast<double>(m - full_edges);
                }
                pulling = pull;
                c.level = level;
                trace_batch.push_back(static_cast<int>(batch));
                trace_level.push_back(level);
                trace_kind.push_back(pull ? LEVEL_PULL : LEVEL_PUSH);
                trace_frontier.push_back(count);
                trace_edges.push_back(frontier_edges);
                if ((retval = step.Start(stream))) return retval;  // (a level is timed as a whole)
                if (pull) {
                    if ((retval = clear_words())) return retval;
                    hipLaunchKernelGGL(PullKernel, cap(graphio::PairGrid(n)), block, 0, stream, c);
                    GR_CHECK(hipGetLastError(), "PullKernel launch failed");
                    ++step.launches;
                    ++pull_levels;
                    Word *was = c.frontier;  // next[] holds the new frontier for every vertex
                    c.frontier = c.next;
                    c.next = was;
                    queued = false;
                    next_clean = false;
                } else {
                    if (!next_clean) {
                        GR_CHECK(hipMemsetAsync(c.next, 0, state_bytes, stream), "MsbfsEnactor memset failed");
                        next_clean = true;
                    }
                    if (!queued) {
                        if ((retval = clear_words())) return retval;
                        hipLaunchKernelGGL(CompactKernel, cap(graphio::PairGrid(n)), block, 0, stream, c);
                        GR_CHECK(hipGetLastError(), "CompactKernel launch failed");
                        ++step.launches;
                        queued = true;
                    }
                    if ((retval = clear_words())) return retval;
                    const int tile = TileFor(count, static_cast<long long>(kStepBlocks) * kPushWavesPerBlock, frontier_edges);
                    hipLaunchKernelGGL(PushKernel, StepGrid(count, tile, kPushWavesPerBlock, max_grid_size), block, 0, stream, c, count, tile);
                    GR_CHECK(hipGetLastError(), "PushKernel launch failed");
                    // a push reaches at most one vertex per entry it walks
                    hipLaunchKernelGGL(UpdateKernel, cap(graphio::PairGrid(frontier_edges < n ? frontier_edges : n)), block, 0, stream, c);
                    GR_CHECK(hipGetLastError(), "UpdateKernel launch failed");
                    step.launches += 2;
                    ++push_levels;
                    int *was = c.queue_in;
                    c.queue_in = c.queue_out;
                    c.queue_out = was;
                }
                float ms = 0;
                if ((retval = step.Stop(stream, &ms))) return retval;
                if ((retval = read_words())) return retval;
                trace_ms.push_back(ms);
                ++levels;
                count = static_cast<long long>(h_words[W_NEW]);
                frontier_edges = static_cast<long long>(h_words[W_FRONTIER_EDGES]);
                full_edges += static_cast<long long>(h_words[W_FULL_EDGES]);
                entries_read += static_cast<long long>(h_words[W_READS]);
            }
        }
        return retval;
    }
};

}  // namespace msbfs
}  // namespace app
}  // namespace gunrock
