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
    int table_slots = kTableSlots;
    int block_slots = kBlockSlots;
    int scratch_mib = kScratchMib;
    int edges = 1;
    double count_limit = kCountLimit;

    static bool PowerOfTwo(long long v) { return v > 0 && (v & (v - 1)) == 0; }

    // 0: set, 1: unknown name, -1: a value out of range
    int Set(const char *name, double value)
    {
        if (!(value == value)) return -1;
        const long long v = static_cast<long long>(value < -1e18 ? -1e18 : value > 1e18 ? 1e18 : value);
        if (!std::strcmp(name, "strategy")) {
            if (v < C4_AUTO || v > C4_GLOBAL) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "lane_max_wedges")) {
            if (v < 0 || v > kLaneArray) return -1;
            lane_max_wedges = static_cast<int>(v);
        } else if (!std::strcmp(name, "table_slots")) {
            if (v < kMinTableSlots || v > kTableSlots || !PowerOfTwo(v)) return -1;
            table_slots = static_cast<int>(v);
        } else if (!std::strcmp(name, "block_slots")) {
            if (v < kMinBlockSlots || v > kBlockSlots || !PowerOfTwo(v)) return -1;
            block_slots = static_cast<int>(v);
        } else if (!std::strcmp(name, "scratch_mib")) {
            if (v < 1 || v > kMaxScratchMib) return -1;
            scratch_mib = static_cast<int>(v);
        } else if (!std::strcmp(name, "edges")) {
            if (v < 0 || v > 1) return -1;
            edges = static_cast<int>(v);
        } else if (!std::strcmp(name, "count_limit")) {
            if (!(value >= 1.0 && value <= kCountLimit)) return -1;
            count_limit = value;
        } else {
            return 1;
        }
        return 0;
    }

    int RegimeOf(long long w) const { return Regime(w, strategy, lane_max_wedges, table_slots, block_slots); }
    // Regime() never falls as W grows: the regime of the largest W tells which kernels a graph can need
    bool AnyBlock(long long max_wedges) const { return max_wedges >= 2 && RegimeOf(max_wedges) >= C4_BLOCK; }
    bool AnyGlobal(long long max_wedges) const { return max_wedges >= 2 && RegimeOf(max_wedges) == C4_GLOBAL; }
    long long Slots(long long grid, long long nodes) const { return GlobalSlots(grid, scratch_mib, nodes); }
    size_t SmallLdsBytes() const { return sizeof(int) * 2 * static_cast<size_t>(kC4Waves) * static_cast<size_t>(table_slots); }
    size_t BlockLdsBytes() const { return sizeof(int) * 2 * static_cast<size_t>(block_slots); }
};

template <bool INSTRUMENT>
class C4Enactor : public EnactorBase {
   public:
    explicit C4Enactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}
    ~C4Enactor() override
    {
        if (ev[0]) hipEventDestroy(ev[0]);
        if (ev[1]) hipEventDestroy(ev[1]);
    }

    C4Options options;

    // of the last Enact
    bool refused = false;  // the bound reached count_limit: nothing ran
    bool with_edges = false;
    double bound = 0;
    long long probes = 0, launches = 0;
    long long regime_vertices[4] = {0, 0, 0, 0}, regime_wedges[4] = {0, 0, 0, 0};  // LANE, WAVE, BLOCK, GLOBAL
    double kernel_ms = 0;  // INSTRUMENT: summed kernel time

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes;
        probes = launches = 0;
        for (int r = 0; r < 4; ++r) regime_vertices[r] = regime_wedges[r] = 0;
        kernel_ms = 0;
        with_edges = false;
        bound = problem->bound;
        refused = bound >= options.count_limit;
        if (refused) return retval;
        if (problem->dirty && (retval = problem->Reset())) return retval;
        with_edges = options.edges != 0;
        if (with_edges && (retval = problem->NeedEdgeCycles())) return retval;
        if (problem->max_wedges < 2) return retval;  // no start vertex: no 4-cycle
        problem->dirty = true;
        if (INSTRUMENT && !ev[0]) {
            GR_CHECK(hipEventCreate(&ev[0]), "C4Enactor hipEventCreate failed");
            GR_CHECK(hipEventCreate(&ev[1]), "C4Enactor hipEventCreate failed");
        }
        auto grid = [&](long long blocks, long long cap) {
            if (blocks > cap) blocks = cap;
            if (blocks < 1) blocks = 1;
            return static_cast<int>(max_grid_size > 0 && max_grid_size < blocks ? max_grid_size : blocks);
        };
        auto begin = [&]() -> hipError_t {
            return INSTRUMENT ? util::GRError(hipEventRecord(ev[0], stream), "C4Enactor hipEventRecord failed", __FILE__, __LINE__) : hipSuccess;
        };
        auto end = [&]() -> hipError_t {
            ++launches;
            if (INSTRUMENT) {
                float ms = 0;
                GR_CHECK(hipEventRecord(ev[1], stream), "C4Enactor hipEventRecord failed");
                GR_CHECK(hipEventSynchronize(ev[1]), "C4Enactor hipEventSynchronize failed");
                GR_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]), "C4Enactor hipEventElapsedTime failed");
                kernel_ms += ms;
            }
            return hipSuccess;
        };

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
        c.table_slots = options.table_slots;
        c.block_slots = options.block_slots;

        GR_CHECK(hipMemsetAsync(ds->d_words + W_BLOCK_LIST, 0, sizeof(unsigned long long) * 2, stream), "C4Enactor memset failed");
        const long long groups = (n + util::kWaveSize - 1) / util::kWaveSize;
        if ((retval = begin())) return retval;
        hipLaunchKernelGGL(SmallKernel, dim3(grid((groups + kC4Waves - 1) / kC4Waves, 4096)), dim3(kC4Threads), options.SmallLdsBytes(), stream, c);
        GR_CHECK(hipGetLastError(), "SmallKernel launch failed");
        if ((retval = end())) return retval;

        if (options.AnyBlock(problem->max_wedges)) {
            const size_t lds = options.BlockLdsBytes();
            if (lds > lds_opted) {  // (64 KiB is all a launch gets unasked; asked for once, for the largest table)
                GR_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&BlockKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(sizeof(int) * 2 * kBlockSlots)),
                         "C4Enactor hipFuncSetAttribute failed");
                lds_opted = sizeof(int) * 2 * kBlockSlots;
            }
            if ((retval = begin())) return retval;
            hipLaunchKernelGGL(BlockKernel, dim3(grid(n, 2048)), dim3(kC4Threads), lds, stream, c);
            GR_CHECK(hipGetLastError(), "BlockKernel launch failed");
            if ((retval = end())) return retval;
        }
        if (options.AnyGlobal(problem->max_wedges)) {
            const int blocks = static_cast<int>(options.Slots(grid(n, 1024), n));
            const size_t need = static_cast<size_t>(blocks) * static_cast<size_t>(n);
            if (need > ds->row_ints) {
                if (ds->d_rows) GR_CHECK(hipFree(ds->d_rows), "C4Enactor hipFree failed");
                ds->d_rows = nullptr;
                ds->row_ints = 0;
                GR_CHECK(hipMalloc(&ds->d_rows, sizeof(int) * need), "C4Enactor hipMalloc d_rows failed");
                GR_CHECK(hipMemsetAsync(ds->d_rows, 0, sizeof(int) * need, stream), "C4Enactor memset failed");  // (once: the kernel leaves them 0)
                ds->row_ints = need;
            }
            if ((retval = begin())) return retval;
            hipLaunchKernelGGL(GlobalKernel, dim3(blocks), dim3(kC4Threads), 0, stream, c, ds->d_rows);
            GR_CHECK(hipGetLastError(), "GlobalKernel launch failed");
            if ((retval = end())) return retval;
        }

        // the one read-back
        unsigned long long words[W_COUNT];
        GR_CHECK(hipMemcpyAsync(words, ds->d_words, sizeof(words), hipMemcpyDeviceToHost, stream), "C4Enactor read-back failed");
        GR_CHECK(hipStreamSynchronize(stream), "C4Enactor read-back sync failed");
        probes = static_cast<long long>(words[W_PROBES]);
        for (int r = 0; r < 4; ++r) {
            regime_vertices[r] = static_cast<long long>(words[W_VERTICES + r]);
            regime_wedges[r] = static_cast<long long>(words[W_WEDGES + r]);
        }
        return retval;
    }

   private:
    hipEvent_t ev[2] = {nullptr, nullptr};
    size_t lds_opted = 0;
};

}  // namespace c4
}  // namespace app
}  // namespace gunrock
