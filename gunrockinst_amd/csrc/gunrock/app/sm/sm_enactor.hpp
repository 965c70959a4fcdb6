// app/sm/sm_enactor.hpp -- host side of subgraph matching.
//
// One Enact: the work bound (q - 1) * hom(T, G) of the plan's anchor tree (computed once per plan, before any enumeration) is held
// against `work_limit`: beyond it nothing runs (kTooLarge).  Then BinKernel sorts the entries that pass levels 0 and 1 into the two
// regimes of sm_functor.hpp, at most one enumeration launch per regime -- both take their list lengths from device memory -- the
// division by aut when the plan has no symmetry breaking, and the one copy of the words and the counters at the end.  A remainder
// of that division is kNotCertified.  INSTRUMENT times every kernel with HIP events (and waits for each).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/sm/sm_functor.hpp>
#include <gunrock/app/sm/sm_problem.hpp>

namespace gunrock {
namespace app {
namespace sm {

constexpr int kTooLarge = -4;      // GRX_SM_TOO_LARGE
constexpr int kNotCertified = -5;  // GRX_SM_NOT_CERTIFIED
constexpr double kWorkLimit = 274877906944.0;         // 2^38: the default "work_limit" (by reasoning)
constexpr double kWorkLimitMax = 4611686018427387904.0;  // 2^62: no counter can wrap

enum { MS_BIN = 0, MS_GROUP8 = 1, MS_WAVE = 2, MS_FINISH = 3, MS_COUNT = 4 };

struct SmOptions {
    int symmetry = 1, per_vertex = 1, strategy = SM_AUTO, group_max_row = kGroupMaxRow, order = ORDER_RULE;
    double work_limit = kWorkLimit;

    // 0 taken, -1 a value out of range, 1 an unknown name
    int Set(const char *name, double value)
    {
        const long long v = Whole(value);
        if (!std::strcmp(name, "symmetry")) {
            if (v < 0 || v > 1) return -1;
            symmetry = static_cast<int>(v);
        } else if (!std::strcmp(name, "per_vertex")) {
            if (v < 0 || v > 1) return -1;
            per_vertex = static_cast<int>(v);
        } else if (!std::strcmp(name, "strategy")) {
            if (v < SM_AUTO || v > SM_WAVE) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "group_max_row")) {
            if (v < 1) return -1;
            group_max_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else if (!std::strcmp(name, "order")) {
            if (v < ORDER_RULE || v > ORDER_ID) return -1;
            order = static_cast<int>(v);
        } else if (!std::strcmp(name, "work_limit")) {
            if (!(value >= 1.0)) return -1;
            work_limit = value < kWorkLimitMax ? value : kWorkLimitMax;
        } else {
            return 1;
        }
        return 0;
    }
};

template <bool INSTRUMENT>
class SmEnactor : public EnactorBase {
   public:
    explicit SmEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    // of the last Enact
    StepHost<INSTRUMENT> host{"SmEnactor"};
    int code = 0;  // 0, kTooLarge or kNotCertified
    double bound = 0;        // hom(T, G)
    bool bound_known = false;  // ... of the plan in force (the runner clears it with every new plan)
    long long items[2] = {0, 0};  // per regime: GROUP8, WAVE
    long long streamed = 0, bisections = 0;
    long long occurrences = 0, embeddings = 0;
    double kind_ms[MS_COUNT] = {0, 0, 0, 0};

    template <typename Problem>
    hipError_t Enact(Problem *problem, const Plan &plan, const SmOptions &options, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long n = problem->nodes, entries = 2 * problem->pairs;
        const int q = plan.q;
        code = 0;
        items[0] = items[1] = streamed = bisections = occurrences = embeddings = 0;
        for (double &ms : kind_ms) ms = 0;
        if ((retval = host.Begin(0))) return retval;
        if (!bound_known) {
            if ((retval = problem->Bound(plan.levels, &bound))) return retval;
            bound_known = true;
        }
        if (bound * (q - 1) > options.work_limit) {
            code = kTooLarge;
            return retval;
        }
        if (problem->dirty && (retval = problem->Reset())) return retval;
        if (entries <= 0) return retval;
        problem->dirty = true;

        const Graph g = problem->DeviceGraph();
        const int strategy = options.strategy, per_vertex = options.per_vertex;
        if ((retval = Timed(MS_BIN, stream, [&]() {
                 hipLaunchKernelGGL(BinKernel, dim3(CappedGrid((entries + kThreads - 1) / kThreads, 2048, max_grid_size)), dim3(kThreads), 0, stream, g,
                                    plan.levels, strategy, options.group_max_row, per_vertex, ds->d_items8.p, ds->d_items64.p, ds->d_words.p,
                                    ds->d_count.p, ds->d_counters.p);
             })))
            return retval;
        if (q > 2) {
            const bool any8 = strategy != SM_WAVE;
            const bool any64 = strategy == SM_WAVE || (strategy == SM_AUTO && problem->longest_row > options.group_max_row);
            if (any8) {
                const int blocks = CappedGrid((entries + 8 * kWaves - 1) / (8 * kWaves), 4096, max_grid_size);
                if ((retval = Timed(MS_GROUP8, stream, [&]() { Launch<8>(q, per_vertex, blocks, stream, g, plan.levels, ds->d_items8.p, ds->d_words.p + W_ITEMS8, ds); })))
                    return retval;
            }
            if (any64) {
                const int blocks = CappedGrid((entries + kWaves - 1) / kWaves, 4096, max_grid_size);
                if ((retval = Timed(MS_WAVE, stream, [&]() { Launch<64>(q, per_vertex, blocks, stream, g, plan.levels, ds->d_items64.p, ds->d_words.p + W_ITEMS64, ds); })))
                    return retval;
            }
        }
        const bool divide = !options.symmetry && plan.aut > 1;
        if (divide && (retval = Timed(MS_FINISH, stream, [&]() {
                           hipLaunchKernelGGL(FinishKernel, dim3(CappedGrid((n + kThreads) / kThreads, 2048, max_grid_size)), dim3(kThreads), 0, stream,
                                              ds->d_count.p, n, ds->d_counters.p, static_cast<unsigned>(plan.aut), ds->d_words.p);
                       })))
            return retval;

        // the one read-back
        unsigned words[W_COUNT] = {0, 0, 0, 0};
        Count counters[C_COUNT] = {0, 0, 0, 0};
        if ((retval = host.Copy(words, ds->d_words, sizeof(words), stream))) return retval;
        if ((retval = host.Read(counters, ds->d_counters, sizeof(counters), stream))) return retval;
        items[0] = words[W_ITEMS8];
        items[1] = words[W_ITEMS64];
        streamed = static_cast<long long>(counters[C_STREAMED]);
        bisections = static_cast<long long>(counters[C_BISECTIONS]);
        if (words[W_BAD]) {
            code = kNotCertified;
            return retval;
        }
        occurrences = static_cast<long long>(counters[C_TOTAL]);
        embeddings = occurrences * plan.aut;
        return retval;
    }

   private:
    template <typename LaunchFn>
    hipError_t Timed(int kind, hipStream_t stream, LaunchFn launch)
    {
        const double before = host.kernel_ms;
        const hipError_t retval = host.Run(stream, launch);
        kind_ms[kind] += host.kernel_ms - before;
        return retval;
    }

    template <int G, typename DataSlice>
    void Launch(int q, int per_vertex, int blocks, hipStream_t stream, const Graph &g, const PlanLevels &plan, const int *d_items, const unsigned *d_item_count,
                DataSlice *ds)
    {
        switch (q) {
            case 3: hipLaunchKernelGGL((EnumerateKernel<3, G>), dim3(blocks), dim3(kThreads), 0, stream, g, plan, d_items, d_item_count, per_vertex, ds->d_count.p, ds->d_counters.p); break;
            case 4: hipLaunchKernelGGL((EnumerateKernel<4, G>), dim3(blocks), dim3(kThreads), 0, stream, g, plan, d_items, d_item_count, per_vertex, ds->d_count.p, ds->d_counters.p); break;
            case 5: hipLaunchKernelGGL((EnumerateKernel<5, G>), dim3(blocks), dim3(kThreads), 0, stream, g, plan, d_items, d_item_count, per_vertex, ds->d_count.p, ds->d_counters.p); break;
            default: hipLaunchKernelGGL((EnumerateKernel<6, G>), dim3(blocks), dim3(kThreads), 0, stream, g, plan, d_items, d_item_count, per_vertex, ds->d_count.p, ds->d_counters.p); break;
        }
    }
};

}  // namespace sm
}  // namespace app
}  // namespace gunrock
