// oprtr/step.hpp -- what a step of a stepped run is made of (the run, its limits, the tile rule, the ticket).
//
// A stepped run is a sequence of steps over a range of a queue or over a live list.  A step is either one wide launch that the
// host reads back behind, or one of a stretch of narrow steps inside a one-workgroup loop on the device: kLoopThreads threads,
// a fence and a barrier between steps, and agent-scope accesses (Ld<true> / St<true>) on everything a step leaves for the next,
// because the loop's CU does not see in its L1 what atomics put into L2.  The primitives keep what is their own (their words,
// their Tally, their row walkers); the pieces they had copied from one another are here, once.
//
// Plain inline functions and kernel templates: a translation unit that uses none of them gets no code and no warning.
#pragma once

#include <hip/hip_runtime.h>

#include <gunrock/util/device_intrinsics.hpp>

namespace gunrock {
namespace oprtr {

// ---------------- the defaults of the options every stepped primitive has ----------------

constexpr int kLoopThreads = 1024;            // the device loop's one workgroup
constexpr int kWaveMinRow = 16;               // "wave_min_row": a row of this many entries and more is walked by the whole wave
constexpr long long kLoopMaxList = 32768;     // "loop_max_list": AUTO gives the device loop a step over up to this many items ...
constexpr long long kLoopMaxEntries = 8192;   // "loop_max_entries": ... whose rows hold up to this many entries
constexpr int kLoopMaxSteps = 4096;           // steps per launch of a device loop

// ---------------- accesses ----------------

// FRESH: agent-scope relaxed, for what another step of the same launch wrote; else a plain access
template <bool FRESH>
__device__ __forceinline__ int Ld(const int *p)
{
    return FRESH ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
template <bool FRESH>
__device__ __forceinline__ void St(int *p, int v)
{
    if (FRESH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// ---------------- which steps the device loop takes ----------------

struct Limits {
    long long max_list, max_entries;
    int max_steps;
};

// a step one workgroup takes: up to max_list items whose rows hold up to max_entries entries
__host__ __device__ __forceinline__ bool Narrow(long long count, long long entries, const Limits &lim)
{
    return count <= lim.max_list && entries <= lim.max_entries;
}

// ---------------- the tile rule ----------------

// Queue entries a wave takes at a time, a power of two up to 64.  Long rows want few (the rows of a short sub-round are spread over
// the waves and not walked one after the other by one of them); short rows want 64 (a wave's appends are one atomic on the tail
// per step whatever the tile: waves of 2 lanes on a grid's front sent 30 000 atomics per sub-round to that one word, which takes
// them at under 100 per microsecond).  So: about kTileEntries row entries per wave, and never more waves than there are.
constexpr long long kTileEntries = 512;
__host__ __device__ __forceinline__ int TileFor(long long count, long long waves, long long entries)
{
    int tile = 1;
    while (tile < util::kWaveSize && (count > tile * waves || entries * tile < kTileEntries * count)) tile <<= 1;
    return tile;
}

// ---------------- the ticket ----------------

// The append of a wave, in the caller's `const unsigned long long mask = __ballot(hit); if (!mask) return;` (the ballot and the
// way out stay with the caller: a merge of the two paths behind a call costs registers).  All lanes call with the wave's mask,
// which is not 0.  The lanes of the mask take consecutive positions from *word, in lane order: one atomic per wave, by lane 0,
// of the number of hits (and the same number onto *also, a second count of the same items, when given).  Returns the lane's
// position, meaningless for a lane outside the mask.  T: the word's type, unsigned or unsigned long long.
template <typename T>
__device__ __forceinline__ T WaveTicket(T *word, unsigned long long mask, T *also = nullptr)
{
    const int lane = static_cast<int>(util::LaneId());
    T at = 0;
    if (lane == 0) {
        at = atomicAdd(word, static_cast<T>(__popcll(mask)));
        if (also) atomicAdd(also, static_cast<T>(__popcll(mask)));
    }
    at = __shfl(at, 0, util::kWaveSize);
    return at + __popcll(mask & ((1ull << lane) - 1ull));
}

// ---------------- two one-line kernels ----------------

// the constant-rate counter, by one thread: the marks a phase or level trace is cut at
template <typename T = unsigned long long>
__global__ void StampKernel(T *d_clock)
{
    *d_clock = wall_clock64();
}

template <typename T>
__global__ void FillKernel(T *d_out, long long count, T value)
{
    const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
    for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) d_out[i] = value;
}

}  // namespace oprtr
}  // namespace gunrock
