// The host-callable pieces of gunrock/oprtr/step.hpp and gunrock/app/step_host.hpp -- the tile rule, Narrow and the Limits a
// schedule gives, the parsing of the four loop options, the grids of a step and of a one-shot launch -- run on their own, without a GPU call, pinned to
// values that follow from their formulas, in a host build with the address and undefined-behaviour sanitizers
// (tests/test_step_host.py compiles and runs this file that way).  Exit status 0 = every check held.
#include <climits>
#include <cstdio>
#include <limits>

#include <gunrock/app/step_host.hpp>
#include <gunrock/oprtr/step.hpp>

using namespace gunrock;
using namespace gunrock::app;

namespace {

int failures = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// tile: the first power of two, up to 64, with count <= tile * waves and entries * tile >= 512 * count
void TileForFollowsTheRule()
{
    CHECK(oprtr::kTileEntries == 512);
    CHECK(oprtr::TileFor(1, 8192, 512) == 1);       // one row of 512 entries: a wave of its own
    CHECK(oprtr::TileFor(64, 1, 64) == 64);         // one wave for 64 items: all of them, whatever their rows
    CHECK(oprtr::TileFor(100, 8192, 800) == 64);    // 8 entries per row: 64 rows make the 512
    CHECK(oprtr::TileFor(100, 8192, 12800) == 4);   // 128 entries per row: 4 rows make the 512
    CHECK(oprtr::TileFor(0, 1, 0) == 1);            // nothing to do: neither condition holds
    // the ends of the two conditions
    CHECK(oprtr::TileFor(8192, 8192, 8192ll * 512) == 1);
    CHECK(oprtr::TileFor(8193, 8192, 8193ll * 512) == 2);   // one item too many for a wave each
    CHECK(oprtr::TileFor(10, 8192, 10 * 256) == 2);         // 256 entries per row: 2 rows make the 512
    CHECK(oprtr::TileFor(10, 8192, 10 * 256 - 1) == 4);     // just under: 2 rows do not
    CHECK(oprtr::TileFor(1ll << 40, 8192, 0) == 64);        // never more than a wave's lanes
}

void NarrowAndTheLimitsOfASchedule()
{
    const oprtr::Limits lim = {100, 1000, 7};
    CHECK(oprtr::Narrow(100, 1000, lim));
    CHECK(!oprtr::Narrow(101, 1000, lim));
    CHECK(!oprtr::Narrow(100, 1001, lim));
    CHECK(oprtr::Narrow(0, 0, lim));

    LoopOptions o;
    CHECK(o.schedule == SCHEDULE_AUTO && o.wave_min_row == oprtr::kWaveMinRow && o.loop_max_list == oprtr::kLoopMaxList &&
          o.loop_max_entries == oprtr::kLoopMaxEntries);
    oprtr::Limits got = o.LimitsFor();
    CHECK(got.max_list == 32768 && got.max_entries == 8192 && got.max_steps == oprtr::kLoopMaxSteps && got.max_steps == 4096);
    CHECK(o.InLoop(32768, 8192) && !o.InLoop(32769, 8192) && !o.InLoop(32768, 8193));
    o.schedule = SCHEDULE_ROUNDS;
    CHECK(!o.InLoop(1, 1) && !o.InLoop(0, 0));
    o.schedule = SCHEDULE_DEVICE_LOOP;
    got = o.LimitsFor();
    CHECK(got.max_list == LLONG_MAX && got.max_entries == LLONG_MAX && got.max_steps == oprtr::kLoopMaxSteps);
    CHECK(o.InLoop(LLONG_MAX, LLONG_MAX));
}

void SetGivesTheAbiCodes()
{
    LoopOptions o;
    CHECK(o.Set("compact_below", 0.5) == 1);  // not one of the four: the caller's
    CHECK(o.Set("", 1) == 1);
    CHECK(o.Set("schedule", 2) == 0 && o.schedule == SCHEDULE_DEVICE_LOOP);
    CHECK(o.Set("schedule", 3) == -1 && o.schedule == SCHEDULE_DEVICE_LOOP);
    CHECK(o.Set("schedule", -1) == -1);
    CHECK(o.Set("schedule", 2, SCHEDULE_ROUNDS) == -1);  // truss: AUTO..ROUNDS
    CHECK(o.Set("schedule", 1, SCHEDULE_ROUNDS) == 0 && o.schedule == SCHEDULE_ROUNDS);
    CHECK(o.Set("wave_min_row", 0) == -1 && o.wave_min_row == oprtr::kWaveMinRow);
    CHECK(o.Set("wave_min_row", 1) == 0 && o.wave_min_row == 1);
    CHECK(o.Set("wave_min_row", 1099511627776.0) == 0 && o.wave_min_row == (1 << 30));  // 2^40
    CHECK(o.Set("loop_max_list", -1) == -1 && o.loop_max_list == oprtr::kLoopMaxList);
    CHECK(o.Set("loop_max_list", 0) == 0 && o.loop_max_list == 0);
    CHECK(o.Set("loop_max_list", 123456789012.0) == 0 && o.loop_max_list == 123456789012ll);
    CHECK(o.Set("loop_max_entries", -1) == -1 && o.loop_max_entries == oprtr::kLoopMaxEntries);
    CHECK(o.Set("loop_max_entries", 65536) == 0 && o.loop_max_entries == 65536);
    // values no long long holds are out of range, not undefined
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(Whole(nan) == LLONG_MIN && Whole(1e300) == LLONG_MAX && Whole(-1e300) == LLONG_MIN);
    CHECK(Whole(-0.9) == 0 && Whole(2.9) == 2);
    // ... the ends of the range: 9.0e18 and beyond is LLONG_MAX, below it the value itself (2^62 is exact)
    CHECK(Whole(9.0e18) == LLONG_MAX && Whole(-9.0e18) == LLONG_MIN && Whole(4611686018427387904.0) == (1ll << 62) &&
          Whole(-4611686018427387904.0) == -(1ll << 62) && Whole(0.0) == 0 && Whole(-1.0) == -1);
    CHECK(o.Set("schedule", nan) == -1 && o.Set("wave_min_row", nan) == -1 && o.Set("loop_max_list", nan) == -1);
    CHECK(o.Set("loop_max_entries", 1e300) == 0 && o.loop_max_entries == LLONG_MAX);
    CHECK(o.Set("wave_min_row", 1e300) == 0 && o.wave_min_row == (1 << 30));
}

void GridsStayInTheirBounds()
{
    CHECK(kStepBlocks == 2048);
    // a wave per tile, 4 waves per block: ceil(ceil(count / tile) / 4), within [1, 2048] and under max_grid_size
    CHECK(StepGrid(0, 1, 4, 0).x == 1);
    CHECK(StepGrid(1, 64, 4, 0).x == 1);
    CHECK(StepGrid(257, 64, 4, 0).x == 2);  // 5 tiles
    CHECK(StepGrid(256, 64, 4, 0).x == 1);  // 4 tiles
    CHECK(StepGrid(1ll << 40, 1, 4, 0).x == 2048);
    CHECK(StepGrid(1ll << 40, 1, 4, 7).x == 7);
    CHECK(StepGrid(1, 1, 4, 7).x == 1);
    // 256 items per block
    CHECK(GridFor(0, 0).x == 1 && GridFor(256, 0).x == 1 && GridFor(257, 0).x == 2);
    CHECK(GridFor(1ll << 40, 0).x == 2048 && GridFor(1ll << 40, 3).x == 3);
    // a one-shot enactor's launch: min(blocks, cap), then min(.., max_grid_size) when that is set, at least 1 -- at the borders of
    // the caps the enactors use
    for (long long cap : {1024ll, 2048ll, 4096ll, 8192ll}) {
        CHECK(CappedGrid(cap - 1, cap, 0) == cap - 1 && CappedGrid(cap, cap, 0) == cap && CappedGrid(cap + 1, cap, 0) == cap);
        CHECK(CappedGrid(1ll << 40, cap, 0) == cap && CappedGrid(1ll << 40, cap, 7) == 7);
        CHECK(CappedGrid(cap, cap, static_cast<int>(cap)) == cap && CappedGrid(cap, cap, static_cast<int>(cap) - 1) == cap - 1 &&
              CappedGrid(cap, cap, static_cast<int>(cap) + 1) == cap);
    }
    CHECK(CappedGrid(0, 4096, 0) == 1 && CappedGrid(-5, 4096, 0) == 1 && CappedGrid(0, 4096, 3) == 1 && CappedGrid(1, 4096, 1) == 1);
    CHECK(CappedGrid(5, 4096, 3) == 3 && CappedGrid(3, 4096, 5) == 3 && CappedGrid(5, 4096, -1) == 5 && CappedGrid(2147483647ll, 1ll << 40, 0) == 2147483647);
}

// An enactor that never ran: nothing was made, so the destructor has nothing to free (and frees nothing twice).
void AnUnusedStepHostOwnsNothing()
{
    StepHost<true> timed("StepCheck");
    StepHost<false> plain("StepCheck");
    CHECK(timed.pinned == nullptr && plain.pinned == nullptr);
    CHECK(timed.launches == 0 && timed.readbacks == 0 && timed.kernel_ms == 0);
}

}  // namespace

int main()
{
    TileForFollowsTheRule();
    NarrowAndTheLimitsOfASchedule();
    SetGivesTheAbiCodes();
    GridsStayInTheirBounds();
    AnUnusedStepHostOwnsNothing();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("step host checks passed\n");
    return 0;
}
