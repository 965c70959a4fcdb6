// oprtr/lds_table.hpp -- the open-addressed key table a wave or a workgroup keeps in LDS, and the fences around it (wave64).
//
// Label propagation's label -> score table, 4-cycle counting's and similarity's end -> count table are one table: int keys, -1 for an
// empty slot, a power-of-two number of slots, linear probing from the low bits of a 32-bit hash.  Here are its caller-neutral pieces:
// the size rule, the clear, the claim and the find, and the three fences a group of lanes puts between its phases.  The value array
// (64-bit scores, int counts) and everything that is done with a slot stay with the caller; nothing here knows who calls it.
#pragma once

#include <hip/hip_runtime.h>

namespace gunrock {
namespace oprtr {
namespace lds {

constexpr int kMinTableSlots = 64;  // a table is never smaller: one slot per lane

// the lanes of one wave have finished their LDS operations and see each other's
__device__ __forceinline__ void WaveLdsSync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ... of the group that shares a table: the workgroup (BLOCK) or one wave
template <bool BLOCK>
__device__ __forceinline__ void GroupSync()
{
    if (BLOCK) __syncthreads();
    else WaveLdsSync();
}

// every wave's global atomics have been performed and every wave of the workgroup knows
__device__ __forceinline__ void GlobalSync()
{
    __threadfence();
    __syncthreads();
}

// The slots a table of at most `slots` takes for `items` keys: 2 items rounded up to a power of two, at least kMinTableSlots.  With
// items <= slots / 2 the table never fills.
__host__ __device__ __forceinline__ int TableSize(long long items, int slots)
{
    int size = kMinTableSlots;
    while (size < slots && size < 2 * items) size <<= 1;
    return size;
}

// Every key of the `size` slots to empty, by the G threads of a group (tid: this thread's place among them); rest(k) clears what the
// caller keeps next to slot k, in the same pass.  A GroupSync follows before the first Claim.
template <int G, typename Rest>
__device__ __forceinline__ void Clear(int *key, int size, int tid, Rest rest)
{
    for (int k = tid; k < size; k += G) {
        key[k] = -1;
        rest(k);
    }
}

// The slot of x (>= 0), which this call or an earlier one claimed, probing from hash & (size - 1); -1 when all `size` slots hold
// other keys.  `probes` counts the slots looked at (a local the caller throws away costs nothing).
__device__ __forceinline__ int Claim(int *key, int size, unsigned hash, int x, unsigned long long &probes)
{
    const unsigned mask = static_cast<unsigned>(size - 1);
    unsigned at = hash & mask;
    for (int probe = 0; probe < size; ++probe) {
        const int was = atomicCAS(key + at, -1, x);
        ++probes;
        if (was == -1 || was == x) return static_cast<int>(at);
        at = (at + 1) & mask;
    }
    return -1;
}

// The slot of x, or -1 when no Claim put it there: the probing ends at the first empty slot (and after `size` slots).  A caller whose
// key is always present -- 4-cycle counting's second pass looks up what its first pass claimed -- never reaches an empty slot, so the
// test for one changes nothing for it.  No Claim runs between the GroupSync in front and the one behind.
__device__ __forceinline__ int Find(const int *key, int size, unsigned hash, int x, unsigned long long &probes)
{
    const unsigned mask = static_cast<unsigned>(size - 1);
    unsigned at = hash & mask;
    for (int probe = 0; probe < size; ++probe) {
        const int was = key[at];
        ++probes;
        if (was == x) return static_cast<int>(at);
        if (was == -1) return -1;
        at = (at + 1) & mask;
    }
    return -1;
}

}  // namespace lds
}  // namespace oprtr
}  // namespace gunrock
