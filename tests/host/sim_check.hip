// tests/host/sim_check.hip -- the host side of vertex similarity without a GPU: SimOptions (app/sim/sim_enactor.hpp) parses the options,
// chooses the regime of a pair from its rows and of a source from its Wd, sizes the tables, the LDS and the GLOBAL regime's workgroup
// slots and refuses what int32 offsets do not address; Fraction (app/sim/sim_functor.hpp) is the formula the kernels share with it.
// What it shares with 4-cycle counting -- TableSize, GlobalSlots, the three table options on their own -- is pinned in
// tests/host/table_check.hip.  Every expectation follows from a formula in those headers.
// Built with -Xarch_host -fsanitize=address,undefined by tests/test_sim_host.py; makes no HIP call.
#include <cstdio>
#include <cstdlib>

#include <gunrock/app/sim/sim_enactor.hpp>

using namespace gunrock::app::sim;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

static bool Is(int metric, int c, int du, int dv, int num, int den)
{
    int n = -7, d = -7;
    Fraction(metric, c, du, dv, n, d);
    return n == num && d == den;
}

int main()
{
    SimOptions o;
    // parsing: 1 for a name nobody knows, -1 for a value out of range, a NaN or what no integer holds
    const double nan = std::strtod("nan", nullptr);
    CHECK(o.Set("nope", 1) == 1);
    CHECK(o.Set("metric", 4) == -1 && o.Set("metric", -1) == -1 && o.Set("metric", nan) == -1 && o.Set("metric", SIM_SORENSEN) == 0 &&
          o.Set("metric", SIM_JACCARD) == 0);
    CHECK(o.Set("strategy", 5) == -1 && o.Set("strategy", -1) == -1 && o.Set("strategy", SIM_GLOBAL) == 0 && o.Set("strategy", SIM_AUTO) == 0);
    CHECK(o.Set("skip_neighbors", 2) == -1 && o.Set("skip_neighbors", -1) == -1 && o.Set("skip_neighbors", 1) == 0 && o.Set("skip_neighbors", 0) == 0);
    CHECK(o.Set("lane_max", kMaxLaneMax + 1) == -1 && o.Set("lane_max", -1) == -1 && o.Set("lane_max", 1e300) == -1);
    CHECK(o.Set("table_slots", 96) == -1 && o.Set("table_slots", 32) == -1 && o.Set("table_slots", 2048) == -1);
    CHECK(o.Set("block_slots", 128) == -1 && o.Set("block_slots", 16384) == -1 && o.Set("block_slots", -1e300) == -1);
    CHECK(o.Set("scratch_mib", 0) == -1 && o.Set("scratch_mib", kMaxScratchMib + 1) == -1);
    // a refused value leaves the option as it was
    CHECK(o.metric == SIM_JACCARD && o.strategy == SIM_AUTO && o.skip_neighbors == 0 && o.lane_max == kLaneMax &&
          o.table.table_slots == kTableSlots && o.table.block_slots == kBlockSlots && o.table.scratch_mib == kScratchMib);

    // the fractions
    CHECK(Is(SIM_COMMON, 3, 5, 7, 3, 1) && Is(SIM_JACCARD, 3, 5, 7, 3, 9) && Is(SIM_OVERLAP, 3, 5, 7, 3, 5) && Is(SIM_SORENSEN, 3, 5, 7, 6, 12));
    CHECK(Is(SIM_JACCARD, 0, 0, 0, 0, 0) && Is(SIM_OVERLAP, 0, 0, 9, 0, 0) && Is(SIM_SORENSEN, 0, 0, 0, 0, 0) && Is(SIM_COMMON, 0, 0, 0, 0, 1));
    CHECK(Is(SIM_JACCARD, 0, 0, 9, 0, 9) && Is(SIM_JACCARD, 4, 4, 4, 4, 4) && Is(SIM_SORENSEN, 1073741823, 1073741823, 1073741824, 2147483646, 2147483647));

    // pair mode: LANE while d(u) + d(v) <= lane_max and nothing larger is forced
    CHECK(o.PairRegimeOf(0) == SIM_LANE && o.PairRegimeOf(64) == SIM_LANE && o.PairRegimeOf(65) == SIM_WAVE && o.PairRegimeOf(4294967294LL) == SIM_WAVE);
    CHECK(o.Set("lane_max", 8) == 0 && o.PairRegimeOf(8) == SIM_LANE && o.PairRegimeOf(9) == SIM_WAVE);
    for (int s = SIM_AUTO; s <= SIM_GLOBAL; ++s) {
        SimOptions f = o;
        f.strategy = s;
        for (long long rows = 0; rows < 20; ++rows) {
            CHECK(f.PairRegimeOf(rows) == (s >= SIM_WAVE || rows > 8 ? SIM_WAVE : SIM_LANE));
            CHECK(f.PairRegimeOf(rows) <= f.PairRegimeOf(rows + 1));
        }
    }
    CHECK(o.Set("lane_max", 0) == 0 && o.PairRegimeOf(0) == SIM_LANE && o.PairRegimeOf(1) == SIM_WAVE);

    // top-k mode under the defaults: Wd <= 1024 / 2 | <= 8192 / 2 | the rest
    CHECK(o.TopkRegimeOf(0) == SIM_WAVE && o.TopkRegimeOf(512) == SIM_WAVE && o.TopkRegimeOf(513) == SIM_BLOCK && o.TopkRegimeOf(4096) == SIM_BLOCK);
    CHECK(o.TopkRegimeOf(4097) == SIM_GLOBAL && o.TopkRegimeOf(2147483647LL) == SIM_GLOBAL);
    CHECK(!o.AnyBlock(512) && o.AnyBlock(513) && o.AnyBlock(4097) && !o.AnyGlobal(4096) && o.AnyGlobal(4097) && !o.AnyBlock(0) && !o.AnyGlobal(0));
    // ... and under the smallest tables: the borders at 32 and 128; a forced regime is a floor; the regime never falls as Wd grows
    CHECK(o.Set("table_slots", 64) == 0 && o.Set("block_slots", 256) == 0);
    for (long long w = 0; w < 400; ++w) {
        const int want = w <= 32 ? SIM_WAVE : w <= 128 ? SIM_BLOCK : SIM_GLOBAL;
        CHECK(o.TopkRegimeOf(w) == want);
        for (int s = SIM_AUTO; s <= SIM_GLOBAL; ++s) {
            SimOptions f = o;
            f.strategy = s;
            CHECK(f.TopkRegimeOf(w) == (want > s ? want : s));
            CHECK(f.TopkRegimeOf(w) <= f.TopkRegimeOf(w + 1));
            CHECK(f.AnyBlock(399) == (s != SIM_GLOBAL) && f.AnyGlobal(399));
        }
        if (want != SIM_GLOBAL) {  // the table holds 2 Wd: it never fills; a whole number of waves scans it
            const int slots = want == SIM_WAVE ? 64 : 256, size = TableSize(w, slots);
            CHECK(size >= 2 * w && (size & (size - 1)) == 0 && size >= kMinTableSlots && size <= slots && size % 64 == 0);
        }
    }
    SimOptions forced;
    CHECK(forced.Set("strategy", SIM_GLOBAL) == 0 && forced.AnyGlobal(0) && !forced.AnyBlock(0) && !forced.AnyBlock(1 << 20));
    CHECK(forced.Set("strategy", SIM_BLOCK) == 0 && forced.AnyBlock(0) && !forced.AnyGlobal(4096) && forced.AnyGlobal(4097));

    // the GLOBAL regime's slots: min(grid, scratch_mib 2^20 / (4 n)), at least 1
    SimOptions d;
    CHECK(d.table.scratch_mib == 1024);
    CHECK(d.Slots(1024, 1024) == 1024 && d.Slots(1024, 1 << 20) == 256 && d.Slots(1024, 1 << 22) == 64 && d.Slots(1024, 2147483647LL) == 1);
    CHECK(d.Slots(1, 10) == 1 && d.Slots(0, 10) == 1);
    CHECK(d.Set("scratch_mib", 2) == 0 && d.Slots(1024, 300503) == 1 && d.Slots(1024, 262144) == 2);
    CHECK(d.Set("scratch_mib", kMaxScratchMib) == 0 && d.Slots(1 << 30, 1) == (1 << 30) && d.Slots(1LL << 40, 1) == (65536LL << 20) / 4);
    // LDS: two ints a slot; a workgroup's table is never smaller than the lists its waves exchange in it
    CHECK(d.SmallLdsBytes() == 32768 && d.BlockLdsBytes() == 65536 && o.SmallLdsBytes() == 2048);
    CHECK(kExchangeInts == 3 * 256 + 4 && o.BlockLdsBytes() == sizeof(int) * kExchangeInts && o.BlockLdsBytes() > sizeof(int) * 2 * 256);
    CHECK(d.Set("block_slots", 512) == 0 && d.BlockLdsBytes() == 4096);

    // k and what int32 offsets address
    CHECK(!SimOptions::ValidK(0) && SimOptions::ValidK(1) && SimOptions::ValidK(64) && !SimOptions::ValidK(65) && !SimOptions::ValidK(-1));
    CHECK(SimOptions::PairsFit(0) && SimOptions::PairsFit(2147483647LL) && !SimOptions::PairsFit(2147483648LL) && !SimOptions::PairsFit(-1));
    CHECK(SimOptions::TopkFits(0, 64) && SimOptions::TopkFits(2147483647LL, 1) && !SimOptions::TopkFits(2147483647LL, 2));
    CHECK(SimOptions::TopkFits(33554431, 64) && !SimOptions::TopkFits(33554432, 64) && !SimOptions::TopkFits(-1, 1) &&
          !SimOptions::TopkFits(4294967296LL, 1));
    std::puts("sim host checks passed");
    return 0;
}
