// app/sim/sim_enactor.hpp -- host side of vertex similarity.
//
// Two Enacts on one problem.  Both first hold the query against what int32 offsets address (refused: kSimTooLarge), then check its ids on
// the device (ValidateIdsKernel, one word read back) before any kernel writes a result.  EnactPairs is one PairKernel.  EnactTopk is
// SmallKernel, which serves the WAVE sources and lists the others; BlockKernel and GlobalKernel follow when the largest Wd of the graph
// can reach their regime.  Both take their list lengths from device memory, so nothing more is read back until the one copy of the
// counters at the end.  The host-side rules -- option ranges, the regimes, table and LDS sizes, the workgroup slots of the GLOBAL regime,
// the refusals -- are SimOptions, plain C++ that a host-only program can call.  INSTRUMENT times every kernel with HIP events (and waits
// for each).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/table_ladder.hpp>
#include <gunrock/app/sim/sim_functor.hpp>
#include <gunrock/app/sim/sim_problem.hpp>

namespace gunrock {
namespace app {
namespace sim {

constexpr int kSimTooLarge = -4;  // GRX_SIM_TOO_LARGE

// options (grx_sim_set_option) and what the host derives from them
struct SimOptions {
    int metric = SIM_JACCARD;
    int strategy = SIM_AUTO;
    int skip_neighbors = 0;
    int lane_max = kLaneMax;
    ladder::TableOptions table;  // "table_slots", "block_slots", "scratch_mib"

    // 0: set, 1: unknown name, -1: a value out of range
    int Set(const char *name, double value)
    {
        if (!(value == value)) return -1;
        const long long v = Whole(value);
        if (!std::strcmp(name, "metric")) {
            if (v < SIM_COMMON || v > SIM_SORENSEN) return -1;
            metric = static_cast<int>(v);
        } else if (!std::strcmp(name, "strategy")) {
            if (v < SIM_AUTO || v > SIM_GLOBAL) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "skip_neighbors")) {
            if (v < 0 || v > 1) return -1;
            skip_neighbors = static_cast<int>(v);
        } else if (!std::strcmp(name, "lane_max")) {
            if (v < 0 || v > kMaxLaneMax) return -1;
            lane_max = static_cast<int>(v);
        } else {
            return table.Set(name, value);
        }
        return 0;
    }

    int PairRegimeOf(long long rows) const { return PairRegime(rows, strategy, lane_max); }
    int TopkRegimeOf(long long wd) const { return TopkRegime(wd, strategy, table.table_slots, table.block_slots); }
    // TopkRegime() never falls as Wd grows: the regimes of no wedge and of the largest Wd tell which kernels a graph can need
    bool AnyBlock(long long max_wedges) const { return TopkRegimeOf(0) <= SIM_BLOCK && TopkRegimeOf(max_wedges) >= SIM_BLOCK; }
    bool AnyGlobal(long long max_wedges) const { return TopkRegimeOf(max_wedges) == SIM_GLOBAL; }
    long long Slots(long long grid, long long nodes) const { return table.Slots(grid, nodes); }
    size_t SmallLdsBytes() const { return table.SmallLdsBytes(kSimWaves); }
    // the table, or the lists the waves exchange in its place when that takes more
    size_t BlockLdsBytes() const
    {
        const size_t bytes = table.BlockLdsBytes(), exchange = sizeof(int) * static_cast<size_t>(kExchangeInts);
        return bytes > exchange ? bytes : exchange;
    }
    // what int32 offsets address
    static bool ValidK(long long k) { return k >= 1 && k <= kMaxK; }
    static bool PairsFit(long long pairs) { return pairs >= 0 && pairs <= 0x7FFFFFFFll; }
    static bool TopkFits(long long sources, long long k) { return sources >= 0 && sources <= 0x7FFFFFFFll && sources * k <= 0x7FFFFFFFll; }
};

template <bool INSTRUMENT>
class SimEnactor : public EnactorBase {
   public:
    explicit SimEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    SimOptions options;

    // of the last Enact (host: its launches and summed kernel time)
    StepHost<INSTRUMENT> host{"SimEnactor"};
    bool refused = false;  // the query is beyond int32 offsets: nothing ran
    bool bad_id = false;   // an id outside [0, nodes): no result was written
    long long probes = 0, candidates = 0, walked = 0;
    long long regime_pairs[2] = {0, 0};                                 // LANE, WAVE
    long long regime_sources[3] = {0, 0, 0}, regime_wedges[3] = {0, 0, 0};  // WAVE, BLOCK, GLOBAL

    // d_u, d_v: `pairs` ids each, in device memory
    template <typename Problem>
    hipError_t EnactPairs(Problem *problem, long long pairs, const int *d_u, const int *d_v, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        stream = problem->graph_slices[0]->stream;
        grid_limit = max_grid_size;
        if ((retval = Clear())) return retval;
        problem->pairs = -1;
        refused = !SimOptions::PairsFit(pairs);
        if (refused) return retval;
        if (pairs == 0) {
            problem->pairs = 0;
            return retval;
        }
        if ((retval = Prepare(ds))) return retval;
        if ((retval = Validate(problem, d_u, d_v, pairs))) return retval;
        if (bad_id) return retval;
        const size_t count = static_cast<size_t>(pairs);
        if ((retval = ds->pair_common.Need(count))) return retval;
        if ((retval = ds->pair_num.Need(count))) return retval;
        if ((retval = ds->pair_den.Need(count))) return retval;
        const Ctx c = Context(problem);
        const long long groups = (pairs + util::kWaveSize - 1) / util::kWaveSize;
        if ((retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL(PairKernel, dim3(CappedGrid((groups + kSimWaves - 1) / kSimWaves, 8192, grid_limit)), dim3(kSimThreads), 0, stream, c,
                                    d_u, d_v, pairs, ds->pair_common.p, ds->pair_num.p, ds->pair_den.p);
             })))
            return retval;
        if ((retval = ReadWords(ds))) return retval;
        problem->pairs = pairs;
        return retval;
    }

    // d_sources: `sources` ids in device memory; k in 1 .. kMaxK (the caller's to check)
    template <typename Problem>
    hipError_t EnactTopk(Problem *problem, long long sources, const int *d_sources, int k, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        stream = problem->graph_slices[0]->stream;
        grid_limit = max_grid_size;
        const long long n = problem->nodes;
        if ((retval = Clear())) return retval;
        problem->sources = -1;
        problem->k = 0;
        refused = !SimOptions::TopkFits(sources, k);
        if (refused) return retval;
        if (sources == 0) {
            problem->sources = 0;
            problem->k = k;
            return retval;
        }
        if ((retval = Prepare(ds))) return retval;
        if ((retval = Validate(problem, d_sources, nullptr, sources))) return retval;
        if (bad_id) return retval;
        const size_t rows = static_cast<size_t>(sources), count = rows * static_cast<size_t>(k);
        if ((retval = ds->ids.Need(count))) return retval;
        if ((retval = ds->common.Need(count))) return retval;
        if ((retval = ds->num.Need(count))) return retval;
        if ((retval = ds->den.Need(count))) return retval;
        if ((retval = ds->count.Need(rows))) return retval;
        if ((retval = ds->candidates.Need(rows))) return retval;
        if ((retval = ds->lists.Need(2 * rows))) return retval;
        const Ctx c = Context(problem);
        const TopkOut o = {ds->ids.p, ds->common.p, ds->num.p, ds->den.p, ds->count.p, ds->candidates.p};
        const int S = static_cast<int>(sources);
        int *block_list = ds->lists.p, *global_list = ds->lists.p + rows;

        if ((retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL(SmallKernel, dim3(CappedGrid((sources + kSimWaves - 1) / kSimWaves, 4096, grid_limit)), dim3(kSimThreads),
                                    options.SmallLdsBytes(), stream, c, o, d_sources, S, k, block_list, global_list);
             })))
            return retval;

        if (options.AnyBlock(problem->max_wedges)) {  // (the LDS: asked for once, for the largest table)
            if ((retval = AllowLds(reinterpret_cast<const void *>(&BlockKernel), ladder::TableOptions::kMaxBlockLdsBytes, &lds_opted))) return retval;
            if ((retval = host.Run(stream, [&]() {
                     hipLaunchKernelGGL(BlockKernel, dim3(CappedGrid(sources, 2048, grid_limit)), dim3(kSimThreads), options.BlockLdsBytes(), stream, c, o,
                                        d_sources, S, k, block_list);
                 })))
                return retval;
        }
        if (options.AnyGlobal(problem->max_wedges)) {
            const int blocks = static_cast<int>(options.Slots(CappedGrid(sources, 1024, grid_limit), n));
            if ((retval = ds->rows.NeedZeroed(static_cast<size_t>(blocks) * static_cast<size_t>(n), stream))) return retval;
            if ((retval = host.Run(stream, [&]() {
                     hipLaunchKernelGGL(GlobalKernel, dim3(blocks), dim3(kSimThreads), 0, stream, c, o, d_sources, S, k, global_list, ds->rows.p);
                 })))
                return retval;
        }
        if ((retval = ReadWords(ds))) return retval;
        problem->sources = sources;
        problem->k = k;
        return retval;
    }

   private:
    size_t lds_opted = 0;
    hipStream_t stream = nullptr;
    int grid_limit = 0;

    hipError_t Clear()
    {
        refused = bad_id = false;
        probes = candidates = walked = 0;
        regime_pairs[0] = regime_pairs[1] = 0;
        for (int r = 0; r < 3; ++r) regime_sources[r] = regime_wedges[r] = 0;
        return host.Begin(0);
    }

    template <typename DataSlice>
    hipError_t Prepare(DataSlice *ds)
    {
        hipError_t retval = hipSuccess;
        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "SimEnactor memset failed");
        return retval;
    }

    template <typename Problem>
    Ctx Context(Problem *problem) const
    {
        typename Problem::DataSlice *ds = problem->data_slices[0];
        Ctx c;
        c.ro = ds->d_ro;
        c.ci = ds->d_ci;
        c.wd = ds->d_wd;
        c.words = ds->d_words;
        c.nodes = static_cast<int>(problem->nodes);
        c.metric = options.metric;
        c.strategy = options.strategy;
        c.skip_neighbors = options.skip_neighbors;
        c.lane_max = options.lane_max;
        c.table_slots = options.table.table_slots;
        c.block_slots = options.table.block_slots;
        return c;
    }

    // the ids of a query on the device; the one word read back says whether all are vertices
    template <typename Problem>
    hipError_t Validate(Problem *problem, const int *d_a, const int *d_b, long long count)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        unsigned long long bad = 0;
        if ((retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL(ValidateIdsKernel, dim3(CappedGrid((count + 255) / 256, 2048, grid_limit)), dim3(256), 0, stream, d_a, d_b, count,
                                    static_cast<int>(problem->nodes), ds->d_words);
             })))
            return retval;
        if ((retval = host.Read(&bad, ds->d_words + W_BAD, sizeof(bad), stream))) return retval;
        bad_id = bad != 0;
        return retval;
    }

    // the counters of the kernels, once, at the end
    template <typename DataSlice>
    hipError_t ReadWords(DataSlice *ds)
    {
        hipError_t retval = hipSuccess;
        unsigned long long words[W_COUNT];
        if ((retval = host.Read(words, ds->d_words, sizeof(words), stream))) return retval;
        probes = static_cast<long long>(words[W_PROBES]);
        candidates = static_cast<long long>(words[W_CANDIDATES]);
        walked = static_cast<long long>(words[W_WALKED]);
        for (int r = 0; r < 2; ++r) regime_pairs[r] = static_cast<long long>(words[W_PAIRS + r]);
        for (int r = 0; r < 3; ++r) {
            regime_sources[r] = static_cast<long long>(words[W_SOURCES + r]);
            regime_wedges[r] = static_cast<long long>(words[W_WEDGES + r]);
        }
        return retval;
    }
};

}  // namespace sim
}  // namespace app
}  // namespace gunrock
