// app/step_host.hpp -- what the enactor of a stepped run (oprtr/step.hpp) does around a launch.
//
// LoopOptions are the four options every stepped primitive takes and what they decide: which steps go to the device loop.
// StepHost owns what an Enact needs around its kernels -- the two events of an instrumented launch, the pinned buffer the
// read-backs land in, the counts of launches and read-backs -- so that an enactor keeps only its own schedule.  The one-shot
// enactors (c4, sim, rw, tc, clique: a fixed handful of launches and one read-back, no steps) hold one too, with no pinned buffer:
// Begin(0), Run per kernel, Read at the end; CappedGrid sizes their launches and AllowLds opts a kernel into a large table.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include <gunrock/oprtr/step.hpp>
#include <gunrock/util/device_array.hpp>
#include <gunrock/util/error_utils.hpp>

namespace gunrock {
namespace app {

// the schedules (every primitive's own enum and the C header's constants have these values)
enum { SCHEDULE_AUTO = 0, SCHEDULE_ROUNDS = 1, SCHEDULE_DEVICE_LOOP = 2 };

constexpr int kStepBlocks = 2048;  // the grid of a wide step at the most: 256 CUs x 8 workgroups

// an option's value as a whole number: out of long long's range the nearest end, NaN the low end (below every option's range)
inline long long Whole(double value)
{
    if (!(value == value)) return LLONG_MIN;
    return value >= 9.0e18 ? LLONG_MAX : (value <= -9.0e18 ? LLONG_MIN : static_cast<long long>(value));
}

struct LoopOptions {
    int schedule = SCHEDULE_AUTO;
    int wave_min_row = oprtr::kWaveMinRow;
    long long loop_max_list = oprtr::kLoopMaxList;
    long long loop_max_entries = oprtr::kLoopMaxEntries;

    // a set_option call: 0 taken, -1 a value out of range, 1 not one of these names (the caller looks at its own)
    int Set(const char *name, double value, int max_schedule = SCHEDULE_DEVICE_LOOP)
    {
        const long long v = Whole(value);
        if (!std::strcmp(name, "schedule")) {
            if (v < SCHEDULE_AUTO || v > max_schedule) return -1;
            schedule = static_cast<int>(v);
        } else if (!std::strcmp(name, "wave_min_row")) {
            if (v < 1) return -1;
            wave_min_row = static_cast<int>(v < (1 << 30) ? v : (1 << 30));
        } else if (!std::strcmp(name, "loop_max_list")) {
            if (v < 0) return -1;
            loop_max_list = v;
        } else if (!std::strcmp(name, "loop_max_entries")) {
            if (v < 0) return -1;
            loop_max_entries = v;
        } else {
            return 1;
        }
        return 0;
    }
    // what a device loop is launched with: DEVICE_LOOP takes every step, whatever its width
    oprtr::Limits LimitsFor() const
    {
        const bool all = schedule == SCHEDULE_DEVICE_LOOP;
        return {all ? LLONG_MAX : loop_max_list, all ? LLONG_MAX : loop_max_entries, oprtr::kLoopMaxSteps};
    }
    // whether a step over `count` items whose rows hold `entries` entries runs in the device loop
    bool InLoop(long long count, long long entries) const
    {
        return schedule == SCHEDULE_DEVICE_LOOP || (schedule == SCHEDULE_AUTO && oprtr::Narrow(count, entries, LimitsFor()));
    }
};

// the grid of a 256-thread grid-stride pass over `work` items
inline dim3 GridFor(long long work, int max_grid_size)
{
    long long blocks = (work + 255) / 256;
    if (blocks > kStepBlocks) blocks = kStepBlocks;
    if (max_grid_size > 0 && blocks > max_grid_size) blocks = max_grid_size;
    if (blocks < 1) blocks = 1;
    return dim3(static_cast<unsigned>(blocks));
}

// the grid of a wide step: a wave per `tile` of the `count` items
inline dim3 StepGrid(long long count, int tile, int waves_per_block, int max_grid_size)
{
    long long blocks = ((count + tile - 1) / tile + waves_per_block - 1) / waves_per_block;
    if (blocks > kStepBlocks) blocks = kStepBlocks;
    if (max_grid_size > 0 && blocks > max_grid_size) blocks = max_grid_size;
    if (blocks < 1) blocks = 1;
    return dim3(static_cast<unsigned>(blocks));
}

// the grid of a one-shot enactor's launch: `blocks` capped at `cap`, then at max_grid_size, at least 1
inline int CappedGrid(long long blocks, long long cap, int max_grid_size)
{
    if (blocks > cap) blocks = cap;
    if (max_grid_size > 0 && blocks > max_grid_size) blocks = max_grid_size;
    if (blocks < 1) blocks = 1;
    return static_cast<int>(blocks);
}

// `kernel` may be launched with `bytes` of dynamic LDS (64 KiB is all a launch gets unasked): asked for once, *allowed is what it has
inline hipError_t AllowLds(const void *kernel, size_t bytes, size_t *allowed)
{
    if (bytes <= *allowed) return hipSuccess;
    const hipError_t retval = util::GRError(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)),
                                            "hipFuncSetAttribute failed", __FILE__, __LINE__);
    if (!retval) *allowed = bytes;
    return retval;
}

// INSTRUMENT: every launch is timed with two events (and waited for).  `who` names the enactor in the error messages.
template <bool INSTRUMENT>
struct StepHost {
    const char *who;
    unsigned char *pinned = nullptr;  // the read-backs land here without a staging copy; the enactor lays it out
    util::PinnedArray<unsigned char> pinned_block;  // (its owner)
    // of the last Enact
    long long launches = 0, readbacks = 0;
    double kernel_ms = 0;  // INSTRUMENT: summed kernel time

    explicit StepHost(const char *who) : who(who) {}
    StepHost(const StepHost &) = delete;
    StepHost &operator=(const StepHost &) = delete;
    ~StepHost()
    {
        if (ev[0]) hipEventDestroy(ev[0]);
        if (ev[1]) hipEventDestroy(ev[1]);
    }

    // the start of an Enact: the counts at zero, `pinned_bytes` of pinned memory (zeroed when first made), the events
    hipError_t Begin(size_t pinned_bytes)
    {
        hipError_t retval = hipSuccess;
        launches = readbacks = 0;
        kernel_ms = 0;
        if (pinned_bytes > bytes) {
            pinned = nullptr;
            bytes = 0;
            if ((retval = Check(pinned_block.Alloc(pinned_bytes), "hipHostMalloc failed", __LINE__))) return retval;
            pinned = pinned_block;
            bytes = pinned_bytes;
            std::memset(pinned, 0, bytes);
        }
        if (INSTRUMENT && !ev[0]) {
            if ((retval = Check(hipEventCreate(&ev[0]), "hipEventCreate failed", __LINE__))) return retval;
            if ((retval = Check(hipEventCreate(&ev[1]), "hipEventCreate failed", __LINE__))) return retval;
        }
        return retval;
    }

    // Around what is timed when instrumented (else both do nothing): Stop waits for it, adds its time to kernel_ms and gives it
    // in *ms (0 when not instrumented).
    hipError_t Start(hipStream_t stream) { return INSTRUMENT ? Check(hipEventRecord(ev[0], stream), "hipEventRecord failed", __LINE__) : hipSuccess; }
    hipError_t Stop(hipStream_t stream, float *ms = nullptr)
    {
        hipError_t retval = hipSuccess;
        float t = 0;
        if (INSTRUMENT) {
            if ((retval = Check(hipEventRecord(ev[1], stream), "hipEventRecord failed", __LINE__))) return retval;
            if ((retval = Check(hipEventSynchronize(ev[1]), "hipEventSynchronize failed", __LINE__))) return retval;
            if ((retval = Check(hipEventElapsedTime(&t, ev[0], ev[1]), "hipEventElapsedTime failed", __LINE__))) return retval;
            kernel_ms += t;
        }
        if (ms) *ms = t;
        return retval;
    }
    // one kernel launch, counted, and timed when instrumented.  A launch() that gives a hipError_t ends the Run with it when it
    // fails: the stop event is not recorded.
    template <typename Launch>
    hipError_t Run(hipStream_t stream, Launch launch)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Start(stream))) return retval;
        if constexpr (std::is_void<decltype(launch())>::value) launch();
        else if ((retval = launch())) return retval;
        if ((retval = Check(hipGetLastError(), "kernel launch failed", __LINE__))) return retval;
        ++launches;
        return Stop(stream);
    }

    // a copy to the host, queued: the Read behind it waits for it too
    hipError_t Copy(void *dst, const void *d_src, size_t count, hipStream_t stream)
    {
        return Check(hipMemcpyAsync(dst, d_src, count, hipMemcpyDeviceToHost, stream), "read-back failed", __LINE__);
    }
    // one read-back: the copy, the wait for the stream, counted
    hipError_t Read(void *dst, const void *d_src, size_t count, hipStream_t stream)
    {
        hipError_t retval = hipSuccess;
        if ((retval = Copy(dst, d_src, count, stream))) return retval;
        if ((retval = Check(hipStreamSynchronize(stream), "read-back sync failed", __LINE__))) return retval;
        ++readbacks;
        return retval;
    }

    // the clock stamp, launched but not counted as a launch of the run
    hipError_t Stamp(unsigned long long *d_clock, hipStream_t stream)
    {
        hipLaunchKernelGGL(oprtr::StampKernel<>, dim3(1), dim3(1), 0, stream, d_clock);
        return Check(hipGetLastError(), "StampKernel launch failed", __LINE__);
    }

   private:
    hipEvent_t ev[2] = {nullptr, nullptr};
    size_t bytes = 0;

    hipError_t Check(hipError_t error, const char *what, int line) const
    {
        if (error != hipSuccess) {
            std::fprintf(stderr, "[%s, %d] %s %s (HIP error %d: %s)\n", __FILE__, line, who, what, static_cast<int>(error), hipGetErrorString(error));
            std::fflush(stderr);
        }
        return error;
    }
};

}  // namespace app
}  // namespace gunrock
