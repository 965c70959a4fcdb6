// app/table_ladder.hpp -- the WAVE -> BLOCK -> GLOBAL ladder of the primitives that count the ends of a vertex's wedges in a table
// (oprtr/lds_table.hpp): 4-cycle counting and similarity.
//
// A vertex with w wedges is served by the smallest rung that holds it: a table of the wave's part of LDS while w <= table_slots / 2,
// the workgroup's LDS as one table while w <= block_slots / 2, else a dense int32[n] counter row per workgroup slot in global scratch,
// of which scratch_mib MiB buy GlobalSlots().  Here are the rules both primitives share -- the rungs, the three options with their
// ranges, the LDS a launch asks for -- as plain C++ a host-only program can call; a primitive keeps what is its own in front (c4's
// LANE rung, the floor sim puts under a forced strategy).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include <gunrock/app/step_host.hpp>
#include <gunrock/oprtr/lds_table.hpp>

namespace gunrock {
namespace app {
namespace ladder {

enum { WAVE = 2, BLOCK = 3, GLOBAL = 4 };  // (every primitive's own enum and the C header's constants have these values)

using oprtr::lds::kMinTableSlots;
using oprtr::lds::TableSize;
constexpr int kTableSlots = 1024;     // default and largest "table_slots": 8 KiB per wave, 32 KiB per workgroup
constexpr int kBlockSlots = 8192;     // default and largest "block_slots": 64 KiB
constexpr int kMinBlockSlots = 256;
constexpr int kScratchMib = 1024;     // default "scratch_mib"  (256 ran 64 workgroups at R-MAT 20)
constexpr int kMaxScratchMib = 65536;

// Regime r, not below WAVE, widened to the first rung that holds w wedges.
__host__ __device__ __forceinline__ int Widen(int r, long long w, int table_slots, int block_slots)
{
    if (r == WAVE && w > table_slots / 2) r = BLOCK;
    if (r == BLOCK && w > block_slots / 2) r = GLOBAL;
    return r;
}

// The workgroup slots of the GLOBAL regime: min(grid, scratch_mib 2^20 / (4 n)), at least 1.
__host__ __device__ __forceinline__ long long GlobalSlots(long long grid, long long scratch_mib, long long nodes)
{
    const long long row_bytes = 4 * (nodes > 0 ? nodes : 1);
    long long slots = (scratch_mib << 20) / row_bytes;
    if (slots > grid) slots = grid;
    return slots < 1 ? 1 : slots;
}

struct TableOptions {
    int table_slots = kTableSlots;
    int block_slots = kBlockSlots;
    int scratch_mib = kScratchMib;

    static bool PowerOfTwo(long long v) { return v > 0 && (v & (v - 1)) == 0; }

    // a set_option call: 0 taken, -1 a value out of range, 1 not one of these names (the caller looks at its own first)
    int Set(const char *name, double value)
    {
        const long long v = Whole(value);
        if (!std::strcmp(name, "table_slots")) {
            if (v < kMinTableSlots || v > kTableSlots || !PowerOfTwo(v)) return -1;
            table_slots = static_cast<int>(v);
        } else if (!std::strcmp(name, "block_slots")) {
            if (v < kMinBlockSlots || v > kBlockSlots || !PowerOfTwo(v)) return -1;
            block_slots = static_cast<int>(v);
        } else if (!std::strcmp(name, "scratch_mib")) {
            if (v < 1 || v > kMaxScratchMib) return -1;
            scratch_mib = static_cast<int>(v);
        } else {
            return 1;
        }
        return 0;
    }

    long long Slots(long long grid, long long nodes) const { return GlobalSlots(grid, scratch_mib, nodes); }
    // two ints a slot: a table per wave, the workgroup's one table, the largest a workgroup can be given
    size_t SmallLdsBytes(int waves) const { return sizeof(int) * 2 * static_cast<size_t>(waves) * static_cast<size_t>(table_slots); }
    size_t BlockLdsBytes() const { return sizeof(int) * 2 * static_cast<size_t>(block_slots); }
    static constexpr size_t kMaxBlockLdsBytes = sizeof(int) * 2 * kBlockSlots;
};

}  // namespace ladder
}  // namespace app
}  // namespace gunrock
