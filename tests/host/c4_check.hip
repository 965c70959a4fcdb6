// tests/host/c4_check.hip -- the host side of 4-cycle counting without a GPU: C4Options (app/c4/c4_enactor.hpp) parses the options,
// chooses the regime of a start vertex from its W and sizes the GLOBAL regime's workgroup slots.  What it shares with similarity --
// TableSize, GlobalSlots, the three table options on their own -- is pinned in tests/host/table_check.hip.  Every expectation follows
// from a formula in those headers.
// Built with -Xarch_host -fsanitize=address,undefined by tests/test_c4_host.py; makes no HIP call.
#include <cstdio>
#include <cstdlib>

#include <gunrock/app/c4/c4_enactor.hpp>

using namespace gunrock::app::c4;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main()
{
    C4Options o;
    // parsing: 1 for a name nobody knows, -1 for a value out of range, a NaN or what no integer holds
    CHECK(o.Set("nope", 1) == 1);
    CHECK(o.Set("strategy", 5) == -1 && o.Set("strategy", -1) == -1 && o.Set("strategy", C4_GLOBAL) == 0 && o.Set("strategy", C4_AUTO) == 0);
    const double nan = std::strtod("nan", nullptr);
    CHECK(o.Set("lane_max_wedges", kLaneArray + 1) == -1 && o.Set("lane_max_wedges", -1) == -1 && o.Set("lane_max_wedges", nan) == -1);
    CHECK(o.Set("table_slots", 96) == -1 && o.Set("table_slots", 32) == -1 && o.Set("table_slots", 2048) == -1);
    CHECK(o.Set("block_slots", 128) == -1 && o.Set("block_slots", 16384) == -1 && o.Set("block_slots", 1e300) == -1 && o.Set("block_slots", -1e300) == -1);
    CHECK(o.Set("scratch_mib", 0) == -1 && o.Set("scratch_mib", kMaxScratchMib + 1) == -1 && o.Set("edges", 2) == -1 && o.Set("edges", -1) == -1);
    CHECK(o.Set("count_limit", 0) == -1 && o.Set("count_limit", 9.3e18) == -1 && o.Set("count_limit", nan) == -1);
    CHECK(o.Set("count_limit", 784) == 0 && o.count_limit == 784.0 && o.Set("count_limit", kCountLimit) == 0);
    // a refused value leaves the option as it was
    CHECK(o.strategy == C4_AUTO && o.lane_max_wedges == kLaneMaxWedges && o.table.table_slots == kTableSlots &&
          o.table.block_slots == kBlockSlots && o.table.scratch_mib == kScratchMib && o.edges == 1);

    // the regimes under the defaults: W <= 16 | <= 1024 / 2 | <= 8192 / 2 | the rest
    CHECK(o.RegimeOf(2) == C4_LANE && o.RegimeOf(16) == C4_LANE && o.RegimeOf(17) == C4_WAVE && o.RegimeOf(512) == C4_WAVE);
    CHECK(o.RegimeOf(513) == C4_BLOCK && o.RegimeOf(4096) == C4_BLOCK && o.RegimeOf(4097) == C4_GLOBAL && o.RegimeOf(2147483647LL) == C4_GLOBAL);
    CHECK(!o.AnyBlock(512) && o.AnyBlock(513) && !o.AnyGlobal(4096) && o.AnyGlobal(4097) && !o.AnyBlock(0) && !o.AnyGlobal(1));
    // ... and under the smallest tables: the borders at 4, 32 and 128; a forced regime is a floor; the regime never falls as W grows
    CHECK(o.Set("lane_max_wedges", 4) == 0 && o.Set("table_slots", 64) == 0 && o.Set("block_slots", 256) == 0);
    for (long long w = 2; w < 400; ++w) {
        const int want = w <= 4 ? C4_LANE : w <= 32 ? C4_WAVE : w <= 128 ? C4_BLOCK : C4_GLOBAL;
        CHECK(o.RegimeOf(w) == want);
        for (int s = C4_LANE; s <= C4_GLOBAL; ++s) {
            C4Options f = o;
            f.strategy = s;
            CHECK(f.RegimeOf(w) == (want > s ? want : s));
            CHECK(f.RegimeOf(w) <= f.RegimeOf(w + 1));
        }
        if (want == C4_WAVE || want == C4_BLOCK) {  // the table holds 2 W: it never fills
            const int slots = want == C4_WAVE ? 64 : 256, size = TableSize(w, slots);
            CHECK(size >= 2 * w && (size & (size - 1)) == 0 && size >= kMinTableSlots && size <= slots);
        }
    }
    C4Options no_lane;
    CHECK(no_lane.Set("lane_max_wedges", 0) == 0 && no_lane.RegimeOf(2) == C4_WAVE);

    // the GLOBAL regime's slots: min(grid, scratch_mib 2^20 / (4 n)), at least 1
    C4Options d;
    CHECK(d.table.scratch_mib == 1024);
    CHECK(d.Slots(1024, 1024) == 1024 && d.Slots(1024, 1 << 20) == 256 && d.Slots(1024, 1 << 22) == 64 && d.Slots(1024, 2147483647LL) == 1);
    CHECK(d.Slots(1, 10) == 1 && d.Slots(0, 10) == 1);
    CHECK(d.Set("scratch_mib", 2) == 0 && d.Slots(1024, 300503) == 1 && d.Slots(1024, 262144) == 2);
    CHECK(d.Set("scratch_mib", kMaxScratchMib) == 0 && d.Slots(1 << 30, 1) == (1 << 30) && d.Slots(1LL << 40, 1) == (65536LL << 20) / 4);
    // LDS: two ints a slot
    CHECK(d.SmallLdsBytes() == 32768 && d.BlockLdsBytes() == 65536 && o.SmallLdsBytes() == 2048 && o.BlockLdsBytes() == 2048);
    std::puts("c4 host checks passed");
    return 0;
}
