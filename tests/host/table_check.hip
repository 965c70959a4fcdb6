// tests/host/table_check.hip -- what 4-cycle counting and similarity share of their end -> count table, without a GPU: the size rule
// of oprtr/lds_table.hpp and the ladder of app/table_ladder.hpp -- the WAVE -> BLOCK -> GLOBAL widening, the workgroup slots of the
// GLOBAL regime, the three options with their ranges and ABI codes, the LDS a launch asks for.  Every expectation follows from a
// formula in those two headers.  Built with -Xarch_host -fsanitize=address,undefined by tests/test_table_host.py; makes no HIP call.
#include <cstdio>
#include <cstdlib>

#include <gunrock/app/table_ladder.hpp>
#include <gunrock/oprtr/lds_table.hpp>

using namespace gunrock::app::ladder;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main()
{
    // the size of a table: 2 items rounded up to a power of two, at least 64, at most `slots`
    CHECK(kMinTableSlots == 64 && gunrock::oprtr::lds::kMinTableSlots == 64);
    CHECK(TableSize(512, 1024) == 1024 && TableSize(4096, 8192) == 8192 && TableSize(2, 1024) == 64 && TableSize(33, 1024) == 128);
    CHECK(TableSize(512, 1024) == 1024 && TableSize(4096, 8192) == 8192 && TableSize(0, 1024) == 64 && TableSize(33, 1024) == 128);
    CHECK(TableSize(32, 1024) == 64 && TableSize(64, 1024) == 128 && TableSize(65, 1024) == 256 && TableSize(1 << 30, 64) == 64);
    CHECK(TableSize(2147483647LL, 8192) == 8192 && TableSize(4294967296LL, 1024) == 1024 && TableSize(-1, 1024) == 64);
    for (int slots = kMinTableSlots; slots <= kBlockSlots; slots <<= 1)
        for (long long w = 0; w <= slots / 2; ++w) {  // what a rung holds fits twice: the table never fills
            const int size = TableSize(w, slots);
            CHECK(size >= 2 * w && (size & (size - 1)) == 0 && size >= kMinTableSlots && size <= slots && size % 64 == 0);
            CHECK(size == kMinTableSlots || size < 4 * w);  // ... and is the smallest such power of two
        }

    // the rungs: WAVE while w <= table_slots / 2, BLOCK while w <= block_slots / 2, then GLOBAL; a rung given is a floor
    CHECK(WAVE == 2 && BLOCK == 3 && GLOBAL == 4);
    CHECK(Widen(WAVE, 0, 1024, 8192) == WAVE && Widen(WAVE, 512, 1024, 8192) == WAVE && Widen(WAVE, 513, 1024, 8192) == BLOCK);
    CHECK(Widen(WAVE, 4096, 1024, 8192) == BLOCK && Widen(WAVE, 4097, 1024, 8192) == GLOBAL && Widen(WAVE, 2147483647LL, 1024, 8192) == GLOBAL);
    for (long long w = 0; w < 400; ++w) {
        const int want = w <= 32 ? WAVE : w <= 128 ? BLOCK : GLOBAL;
        CHECK(Widen(WAVE, w, 64, 256) == want);
        for (int r = WAVE; r <= GLOBAL; ++r) {
            CHECK(Widen(r, w, 64, 256) == (want > r ? want : r));
            CHECK(Widen(r, w, 64, 256) <= Widen(r, w + 1, 64, 256));
        }
    }
    CHECK(Widen(WAVE, 200, 1024, 256) == WAVE && Widen(WAVE, 600, 1024, 256) == GLOBAL);  // (a workgroup's table below a wave's: skipped)
    CHECK(Widen(1, 1 << 20, 64, 256) == 1);  // a regime below the ladder is the caller's: left as it is

    // the GLOBAL regime's slots: min(grid, scratch_mib 2^20 / (4 n)), at least 1
    CHECK(GlobalSlots(1024, 1024, 1024) == 1024 && GlobalSlots(1024, 1024, 1 << 20) == 256 && GlobalSlots(1024, 1024, 1 << 22) == 64);
    CHECK(GlobalSlots(1024, 1024, 2147483647LL) == 1 && GlobalSlots(1, 1024, 10) == 1 && GlobalSlots(0, 1024, 10) == 1);
    CHECK(GlobalSlots(1024, 2, 300503) == 1 && GlobalSlots(1024, 2, 262144) == 2 && GlobalSlots(1024, 2, 262145) == 1);
    CHECK(GlobalSlots(1 << 30, 65536, 1) == (1 << 30) && GlobalSlots(1LL << 40, 65536, 1) == (65536LL << 20) / 4);
    CHECK(GlobalSlots(1024, 1, 0) == 1024 && GlobalSlots(1LL << 40, 1, 0) == (1 << 18) && GlobalSlots(1024, 1, -3) == 1024);  // n < 1 counts as 1

    // the options: 0 taken, -1 out of range (what no integer holds and a NaN among it), 1 a name of the caller's own
    TableOptions o;
    const double nan = std::strtod("nan", nullptr);
    CHECK(kTableSlots == 1024 && kBlockSlots == 8192 && kMinBlockSlots == 256 && kScratchMib == 1024 && kMaxScratchMib == 65536);
    CHECK(o.table_slots == kTableSlots && o.block_slots == kBlockSlots && o.scratch_mib == kScratchMib);
    CHECK(o.Set("nope", 1) == 1 && o.Set("", 1) == 1 && o.Set("strategy", 2) == 1 && o.Set("nope", nan) == 1);
    CHECK(o.Set("table_slots", 96) == -1 && o.Set("table_slots", 32) == -1 && o.Set("table_slots", 2048) == -1);
    CHECK(o.Set("table_slots", nan) == -1 && o.Set("table_slots", 0) == -1 && o.Set("table_slots", -64) == -1 && o.Set("table_slots", 1e300) == -1);
    CHECK(o.Set("block_slots", 128) == -1 && o.Set("block_slots", 16384) == -1 && o.Set("block_slots", 1e300) == -1 && o.Set("block_slots", -1e300) == -1);
    CHECK(o.Set("block_slots", nan) == -1 && o.Set("block_slots", 384) == -1);
    CHECK(o.Set("scratch_mib", 0) == -1 && o.Set("scratch_mib", kMaxScratchMib + 1) == -1 && o.Set("scratch_mib", nan) == -1 &&
          o.Set("scratch_mib", -1e300) == -1);
    // a refused value leaves the option as it was
    CHECK(o.table_slots == kTableSlots && o.block_slots == kBlockSlots && o.scratch_mib == kScratchMib);
    // the ends of the ranges are taken
    CHECK(o.Set("table_slots", 64) == 0 && o.table_slots == 64 && o.Set("table_slots", 1024) == 0 && o.table_slots == 1024);
    CHECK(o.Set("block_slots", 256) == 0 && o.block_slots == 256 && o.Set("block_slots", 8192) == 0 && o.block_slots == 8192);
    CHECK(o.Set("scratch_mib", 1) == 0 && o.scratch_mib == 1 && o.Set("scratch_mib", kMaxScratchMib) == 0 && o.scratch_mib == kMaxScratchMib);
    CHECK(o.Set("scratch_mib", 2.9) == 0 && o.scratch_mib == 2);  // (a fraction is cut, as everywhere)
    CHECK(o.Slots(1024, 300503) == 1 && o.Slots(1024, 262144) == 2);
    CHECK(TableOptions::PowerOfTwo(1) && TableOptions::PowerOfTwo(1LL << 40) && !TableOptions::PowerOfTwo(0) && !TableOptions::PowerOfTwo(-4) &&
          !TableOptions::PowerOfTwo(96));

    // LDS: two ints a slot
    TableOptions d;
    CHECK(d.SmallLdsBytes(4) == 32768 && d.BlockLdsBytes() == 65536 && TableOptions::kMaxBlockLdsBytes == 65536);
    CHECK(d.Set("table_slots", 64) == 0 && d.Set("block_slots", 256) == 0 && d.SmallLdsBytes(4) == 2048 && d.SmallLdsBytes(1) == 512 &&
          d.BlockLdsBytes() == 2048);
    std::puts("table host checks passed");
    return 0;
}
