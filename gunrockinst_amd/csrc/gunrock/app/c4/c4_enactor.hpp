// app/c4/c4_enactor.hpp -- host side of 4-cycle (butterfly) counting.
//
// One Enact: the bound (the build left it on the host) is held against `count_limit` before any kernel.  SmallKernel counts the start
// vertices of the LANE and WAVE regimes and lists the others; BlockKernel and GlobalKernel follow when the largest W of the graph
// can reach their regime.  Both take their list lengths from device memory, so nothing is read back until the one copy of the
// counters at the end.  The host-side rules -- option ranges, the largest regime of a graph, the workgroup slots of the GLOBAL regime
// -- are C4Options, plain C++ that a host-only program can call.  INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/table_ladder.hpp>
#include <gunrock/app/c4/c4_functor.hpp>
#include <gunrock/app/c4/c4_problem.hpp>

namespace gunrock {
namespace app {
namespace c4 {

constexpr int kC4Overflow = -7;  // GRX_C4_OVERFLOW
constexpr double kCountLimit = 4611686018427387904.0;  // 2^62

// options (grx_c4_set_option) and what the host derives from them
struct C4Options {
    int strategy = C4_AUTO;
    int lane_max_wedges = kLaneMaxWedges;
    ladder::TableOptions table;  // "table_slots", "block_slots", "scratch_mib"
    int edges = 1;
    double count_limit = kCountLimit;

    // 0: set, 1: unknown name, -1: a value out of range
    int Set(const char *name, double value)
    {
        if (!(value == value)) return -1;
        const long long v = Whole(value);
        if (!std::strcmp(name, "strategy")) {
            if (v < C4_AUTO || v > C4_GLOBAL) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "lane_max_wedges")) {
            if (v < 0 || v > kLaneArray) return -1;
            lane_max_wedges = static_cast<int>(v);
        } else if (!std::strcmp(name, "edges")) {
            if (v < 0 || v > 1) return -1;
            edges = static_cast<int>(v);
        } else if (!std::strcmp(name, "count_limit")) {
            if (!(value >= 1.0 && value <= kCountLimit)) return -1;
            count_limit = value;
        } else {
            return table.Set(name, value);
        }
        return 0;
    }

    int RegimeOf(long long w) const { return Regime(w, strategy, lane_max_wedges, table.table_slots, table.block_slots); }
    // Regime() never falls as W grows: the regime of the largest W tells which kernels a graph can need
    bool AnyBlock(long long max_wedges) const { return max_wedges >= 2 && RegimeOf(max_wedges) >= C4_BLOCK; }
    bool AnyGlobal(long long max_wedges) const { return max_wedges >= 2 && RegimeOf(max_wedges) == C4_GLOBAL; }
    long long Slots(long long grid, long long nodes) const { return table.Slots(grid, nodes); }
    size_t SmallLdsBytes() const { return table.SmallLdsBytes(kC4Waves); }
    size_t BlockLdsBytes() const { return table.BlockLdsBytes(); }
};

template <bool INSTRUMENT>
class C4Enactor : public EnactorBase {
   public:
    explicit C4Enactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    C4Options options;

    // of the last Enact (host: its launches and summed kernel time)
    StepHost<INSTRUMENT> host{"C4Enactor"};
    bool refused = false;  // the bound reached count_limit: nothing ran
    bool with_edges = false;
    double bound = 0;
    long long probes = 0;
    long long regime_vertices[4] = {0, 0, 0, 0}, regime_wedges[4] = {0, 0, 0, 0};  // LANE, WAVE, BLOCK, GLOBAL

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes;
        probes = 0;
        for (int r = 0; r < 4; ++r) regime_vertices[r] = regime_wedges[r] = 0;
        if ((retval = host.Begin(0))) return retval;
        with_edges = false;
        bound = problem->bound;
        refused = bound >= options.count_limit;
        if (refused) return retval;
        if (problem->dirty && (retval = problem->Reset())) return retval;
        with_edges = options.edges != 0;
        if (with_edges && (retval = problem->NeedEdgeCycles())) return retval;
        if (problem->max_wedges < 2) return retval;  // no start vertex: no 4-cycle
        problem->dirty = true;

        Ctx c;
        c.ro = ds->d_ro;
        c.ci = ds->d_ci;
        c.eid = ds->d_eid;
        c.pre = ds->d_pre;
        c.dlow = ds->d_dlow;
        c.wedges = ds->d_wedges;
        c.inv = ds->d_inv;
        c.cycles = ds->d_cycles;
        c.edge_cycles = with_edges ? ds->d_edge_cycles : nullptr;
        c.words = ds->d_words;
        c.block_list = ds->d_lists;
        c.global_list = ds->d_lists + n;
        c.nodes = static_cast<int>(n);
        c.strategy = options.strategy;
        c.lane_max_wedges = options.lane_max_wedges;
        c.table_slots = options.table.table_slots;
        c.block_slots = options.table.block_slots;

        GR_CHECK(hipMemsetAsync(ds->d_words + W_BLOCK_LIST, 0, sizeof(unsigned long long) * 2, stream), "C4Enactor memset failed");
        const long long groups = (n + util::kWaveSize - 1) / util::kWaveSize;
        if ((retval = host.Run(stream, [&]() {
                 hipLaunchKernelGGL(SmallKernel, dim3(CappedGrid((groups + kC4Waves - 1) / kC4Waves, 4096, max_grid_size)), dim3(kC4Threads),
                                    options.SmallLdsBytes(), stream, c);
             })))
            return retval;

        if (options.AnyBlock(problem->max_wedges)) {  // (the LDS: asked for once, for the largest table)
            if ((retval = AllowLds(reinterpret_cast<const void *>(&BlockKernel), ladder::TableOptions::kMaxBlockLdsBytes, &lds_opted))) return retval;
            if ((retval = host.Run(stream, [&]() {
                     hipLaunchKernelGGL(BlockKernel, dim3(CappedGrid(n, 2048, max_grid_size)), dim3(kC4Threads), options.BlockLdsBytes(), stream, c);
                 })))
                return retval;
        }
        if (options.AnyGlobal(problem->max_wedges)) {
            const int blocks = static_cast<int>(options.Slots(CappedGrid(n, 1024, max_grid_size), n));
            if ((retval = ds->rows.NeedZeroed(static_cast<size_t>(blocks) * static_cast<size_t>(n), stream))) return retval;
            if ((retval = host.Run(stream, [&]() { hipLaunchKernelGGL(GlobalKernel, dim3(blocks), dim3(kC4Threads), 0, stream, c, ds->rows.p); })))
                return retval;
        }

        // the one read-back
        unsigned long long words[W_COUNT];
        if ((retval = host.Read(words, ds->d_words, sizeof(words), stream))) return retval;
        probes = static_cast<long long>(words[W_PROBES]);
        for (int r = 0; r < 4; ++r) {
            regime_vertices[r] = static_cast<long long>(words[W_VERTICES + r]);
            regime_wedges[r] = static_cast<long long>(words[W_WEDGES + r]);
        }
        return retval;
    }

   private:
    size_t lds_opted = 0;
};

}  // namespace c4
}  // namespace app
}  // namespace gunrock
