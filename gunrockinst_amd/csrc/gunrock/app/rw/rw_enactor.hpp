// app/rw/rw_enactor.hpp -- host side of the random walks.
//
// One Enact is one launch of LaneKernel or TileKernel (every walker from its start to its end), VisitsKernel behind it when the
// option "visits" asks, and one read-back of the four counters.  The host-side rules -- option ranges, the strategy AUTO takes for a
// length, the pitch of a row -- are RwOptions and rw_functor.hpp's Pitch, plain C++ that a host-only program can call.  INSTRUMENT
// times the kernels with HIP events.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include <gunrock/app/enactor_base.hpp>
#include <gunrock/app/step_host.hpp>
#include <gunrock/app/rw/rw_functor.hpp>
#include <gunrock/app/rw/rw_problem.hpp>

namespace gunrock {
namespace app {
namespace rw {

// AUTO takes TILE from this length on: it won every measured cell from length 1 up; length 0 has one column and
// nothing to stage
constexpr int kTileMinLength = 1;

// options (grx_rw_set_option) and what the host derives from them
struct RwOptions {
    int strategy = RW_AUTO;
    int length = 0;
    unsigned long long seed = 0;
    int weighted = 0;
    int bias_return = 1, bias_in = 1, bias_out = 1;
    int tries = kDefaultTries;
    int visits = 0;

    // 0: set, 1: unknown name, -1: a value out of range.  `weights`: Init had weights
    int Set(const char *name, double value, bool weights)
    {
        if (!(value == value)) return -1;
        const long long v = Whole(value);
        const bool whole = static_cast<double>(v) == value;
        if (!std::strcmp(name, "strategy")) {
            if (v < RW_AUTO || v > RW_TILE) return -1;
            strategy = static_cast<int>(v);
        } else if (!std::strcmp(name, "length")) {
            if (v < 0 || v > kMaxLength) return -1;
            length = static_cast<int>(v);
        } else if (!std::strcmp(name, "seed")) {
            if (!whole || v < 0 || v >= (1ll << 53)) return -1;
            seed = static_cast<unsigned long long>(v);
        } else if (!std::strcmp(name, "weighted")) {
            if (v < 0 || v > 1 || (v == 1 && !weights)) return -1;
            weighted = static_cast<int>(v);
        } else if (!std::strcmp(name, "bias_return") || !std::strcmp(name, "bias_in") || !std::strcmp(name, "bias_out")) {
            if (v < 0 || v > kMaxBias) return -1;
            (name[5] == 'r' ? bias_return : name[5] == 'i' ? bias_in : bias_out) = static_cast<int>(v);
        } else if (!std::strcmp(name, "tries")) {
            if (v < 1 || v > kMaxTries) return -1;
            tries = static_cast<int>(v);
        } else if (!std::strcmp(name, "visits")) {
            if (v < 0 || v > 1) return -1;
            visits = static_cast<int>(v);
        } else {
            return 1;
        }
        return 0;
    }

    bool Biased() const { return !(bias_return == bias_in && bias_in == bias_out); }
    int MaxBias() const { return bias_return > bias_in ? (bias_return > bias_out ? bias_return : bias_out) : (bias_in > bias_out ? bias_in : bias_out); }
    // the kernel that writes the rows
    int Strategy() const { return strategy != RW_AUTO ? strategy : length >= kTileMinLength ? RW_TILE : RW_LANE; }
};

template <bool INSTRUMENT>
class RwEnactor : public EnactorBase {
   public:
    explicit RwEnactor(bool DEBUG = false) : EnactorBase(VERTEX_FRONTIERS, DEBUG) {}

    RwOptions options;

    // of the last Enact (host: its launches and summed kernel time)
    StepHost<INSTRUMENT> host{"RwEnactor"};
    int length = 0;
    bool with_visits = false;
    int taken = RW_LANE;  // the strategy that ran
    long long steps = 0, ended = 0, tries = 0, forced = 0;

    template <typename Problem>
    hipError_t Enact(Problem *problem, int max_grid_size = 0)
    {
        hipError_t retval = hipSuccess;
        typename Problem::DataSlice *ds = problem->data_slices[0];
        hipStream_t stream = problem->graph_slices[0]->stream;
        const long long walks = problem->num_walks;
        steps = ended = tries = forced = 0;
        if ((retval = host.Begin(0))) return retval;
        length = options.length;
        with_visits = options.visits != 0;
        taken = options.Strategy();
        if ((retval = problem->NeedWalks(Pitch(length)))) return retval;
        if (with_visits && (retval = problem->NeedVisits())) return retval;
        Ctx c;
        c.ro = ds->d_ro;
        c.ci = ds->d_ci;
        c.prefix = options.weighted ? ds->d_prefix : nullptr;
        c.starts = ds->d_starts;
        c.walks = ds->d_walks;
        c.lengths = ds->d_lengths;
        c.words = ds->d_words;
        c.num_walks = walks;
        c.pitch = problem->pitch;
        c.seed = options.seed;
        c.length = length;
        c.b_return = options.bias_return;
        c.b_in = options.bias_in;
        c.b_out = options.bias_out;
        c.amax = options.MaxBias();
        c.biased = options.Biased() ? 1 : 0;
        c.tries = options.tries;

        GR_CHECK(hipMemsetAsync(ds->d_words, 0, sizeof(unsigned long long) * W_COUNT, stream), "RwEnactor memset failed");
        const int blocks = CappedGrid((walks + kRwThreads - 1) / kRwThreads, 8192, max_grid_size);
        if ((retval = host.Run(stream, [&]() {
                 if (taken == RW_TILE) hipLaunchKernelGGL(TileKernel, dim3(blocks), dim3(kRwThreads), 0, stream, c);
                 else hipLaunchKernelGGL(LaneKernel, dim3(blocks), dim3(kRwThreads), 0, stream, c);
             })))
            return retval;
        if (with_visits) {
            GR_CHECK(hipMemsetAsync(ds->d_visits, 0, sizeof(unsigned long long) * static_cast<size_t>(problem->nodes), stream), "RwEnactor memset failed");
            if ((retval = host.Run(stream, [&]() {
                     hipLaunchKernelGGL(VisitsKernel, dim3(CappedGrid((walks * (length + 1) + 255) / 256, 2048, max_grid_size)), dim3(256), 0, stream,
                                        ds->d_walks, walks, length + 1, problem->pitch, ds->d_visits);
                 })))
                return retval;
        }

        // the one read-back
        unsigned long long words[W_COUNT];
        if ((retval = host.Read(words, ds->d_words, sizeof(words), stream))) return retval;
        steps = static_cast<long long>(words[W_STEPS]);
        ended = static_cast<long long>(words[W_ENDED]);
        tries = static_cast<long long>(words[W_TRIES]);
        forced = static_cast<long long>(words[W_FORCED]);
        return retval;
    }
};

}  // namespace rw
}  // namespace app
}  // namespace gunrock
