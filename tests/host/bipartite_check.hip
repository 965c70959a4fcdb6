// tests/host/bipartite_check.hip -- the host side of the bipartite matching, without a GPU: the options with their ranges and ABI
// codes, the lane / wave / workgroup split of a frontier column, the layout of the pinned read-back buffer and the narrow-or-wide
// decision for a level.  Every expectation follows from a formula in app/bipartite/bipartite_functor.hpp, bipartite_enactor.hpp or
// app/step_host.hpp.  Built with -Xarch_host -fsanitize=address,undefined by tests/test_bipartite_host.py; makes no HIP call.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include <gunrock/gunrock_mi355x.h>

#include <gunrock/app/bipartite/bipartite_enactor.hpp>
#include <gunrock/app/handle_runner.hpp>

using namespace gunrock::app;
using namespace gunrock::app::bipartite;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main()
{
    // the ABI's values
    CHECK(GRX_BIPARTITE_AUTO == 0 && GRX_BIPARTITE_LANE == 1 && GRX_BIPARTITE_WAVE == 2 && GRX_BIPARTITE_BLOCK == 3);
    CHECK(GRX_BIPARTITE_HORIZONTAL == 0 && GRX_BIPARTITE_SQUARE == 1 && GRX_BIPARTITE_VERTICAL == 2);
    CHECK(GRX_BIPARTITE_MAXIMUM == 0 && GRX_BIPARTITE_CAPPED == 1);
    CHECK(kNotCertified == -4 && kBadMatching == -5 && kNotMaximum == -6 && kMalformedGraph == -2 && kHandleTaken == -3);
    CHECK(kFree == -1 && kNone == INT_MAX);

    // the defaults and the ranges of the options: 0 set, 1 unknown, -1 out of range
    BipartiteOptions o;
    CHECK(o.strategy == BIPARTITE_AUTO && o.greedy == 1 && o.max_phases == 0 && o.block_min_row == 2048);
    CHECK(o.loop.schedule == SCHEDULE_AUTO && o.loop.wave_min_row == 16 && o.loop.loop_max_list == 32768 && o.loop.loop_max_entries == 8192);
    CHECK(o.Set("strategy", 3) == 0 && o.strategy == BIPARTITE_BLOCK && o.Set("strategy", 4) == -1 && o.Set("strategy", -1) == -1 && o.strategy == 3);
    CHECK(o.Set("strategy", 0) == 0);
    CHECK(o.Set("greedy", 0) == 0 && o.greedy == 0 && o.Set("greedy", 2) == -1 && o.Set("greedy", -1) == -1 && o.Set("greedy", 1) == 0);
    CHECK(o.Set("max_phases", 7) == 0 && o.max_phases == 7 && o.Set("max_phases", -1) == -1 && o.Set("max_phases", 2e12) == -1 && o.max_phases == 7);
    CHECK(o.Set("max_phases", static_cast<double>(kMaxMaxPhases)) == 0 && o.Set("max_phases", 0) == 0);
    CHECK(o.Set("block_min_row", 0) == -1 && o.Set("block_min_row", 1) == 0 && o.block_min_row == 1);
    CHECK(o.Set("block_min_row", 1e18) == 0 && o.block_min_row == 1 << 30 && o.Set("block_min_row", 2048) == 0);
    CHECK(o.Set("wave_min_row", 0) == -1 && o.Set("wave_min_row", 4) == 0 && o.loop.wave_min_row == 4 && o.Set("wave_min_row", 16) == 0);
    CHECK(o.Set("schedule", 3) == -1 && o.Set("schedule", 2) == 0 && o.loop.schedule == SCHEDULE_DEVICE_LOOP && o.Set("schedule", 0) == 0);
    CHECK(o.Set("loop_max_list", -1) == -1 && o.Set("loop_max_entries", -1) == -1);
    CHECK(o.Set("no such option", 1) == 1 && o.Set("no such option", std::nan("")) == 1);
    CHECK(o.Set("strategy", std::nan("")) == -1 && o.Set("greedy", std::nan("")) == -1 && o.Set("max_phases", std::nan("")) == -1);
    CHECK(o.strategy == 0 && o.greedy == 1 && o.max_phases == 0);

    // the split: fewer than wave_min_row entries a lane, fewer than block_min_row a wave, the others a workgroup; a forced
    // strategy sends every column its way; a block_min_row under wave_min_row does not undercut it
    const int lens[] = {1, 15, 16, 17, 2047, 2048, 2049, 1 << 30};
    const int want[] = {1, 1, 2, 2, 2, 3, 3, 3};
    for (int i = 0; i < 8; ++i) CHECK(o.RegimeOf(lens[i]) == want[i] && Regime(lens[i], BIPARTITE_AUTO, 16, 2048) == want[i]);
    for (int s = BIPARTITE_LANE; s <= BIPARTITE_BLOCK; ++s)
        for (int len : lens) CHECK(Regime(len, s, 16, 2048) == s);
    CHECK(Regime(3, 0, 4, 9) == 1 && Regime(4, 0, 4, 9) == 2 && Regime(5, 0, 4, 9) == 2);
    CHECK(Regime(8, 0, 4, 9) == 2 && Regime(9, 0, 4, 9) == 3 && Regime(10, 0, 4, 9) == 3);
    CHECK(Regime(5, 0, 8, 2) == 1 && Regime(8, 0, 8, 2) == 3 && Regime(1, 0, 1, 1) == 3 && Regime(1, 0, 1, 2) == 2);

    // the pinned buffer: 8 words, the front, 16 counts, the two ints of the square graph; nothing overlaps
    CHECK(kPinnedWords == 0 && sizeof(unsigned) * W_COUNT == 32 && kPinnedFront == 32 && sizeof(Front) == 24);
    CHECK(kPinnedCounts == 64 && sizeof(unsigned long long) * C_COUNT == 128 && kPinnedSquare == 192 && kPinnedBytes == 208);
    CHECK(W_TAIL == 0 && W_ENTRIES == 1 && W_FOUND == 2 && W_AUG == 3 && W_GREEDY == 4 && W_BAD == 5 && W_COUNT == 8);
    CHECK(C_BAD_PAIRS == 0 && C_UNCOVERED == 1 && C_COVER == 2 && C_SIZE == 3 && C_REGIME == 4 && C_PART == 7 && C_PART + 6 <= C_COUNT);

    // a level runs in the device loop when it is narrow -- at most loop_max_list vertices with at most loop_max_entries entries --
    // under AUTO, never under ROUNDS, always under DEVICE_LOOP
    CHECK(o.LevelInLoop(1, 1) && o.LevelInLoop(32768, 8192) && !o.LevelInLoop(32769, 8192) && !o.LevelInLoop(32768, 8193) && o.LevelInLoop(0, 0));
    CHECK(o.Set("loop_max_list", 8) == 0 && o.Set("loop_max_entries", 64) == 0);
    CHECK(o.LevelInLoop(8, 64) && !o.LevelInLoop(9, 64) && !o.LevelInLoop(8, 65));
    CHECK(o.Set("loop_max_list", 0) == 0 && !o.LevelInLoop(1, 0) && o.LevelInLoop(0, 0));
    CHECK(o.Set("schedule", SCHEDULE_ROUNDS) == 0 && !o.LevelInLoop(0, 0) && !o.LevelInLoop(1, 1));
    CHECK(o.Set("schedule", SCHEDULE_DEVICE_LOOP) == 0 && o.LevelInLoop(1ll << 40, 1ll << 40));
    const gunrock::oprtr::Limits all = o.loop.LimitsFor();
    CHECK(all.max_list == LLONG_MAX && all.max_entries == LLONG_MAX && all.max_steps == 4096);

    // the cap: max_phases 0 is none
    CHECK(!o.Capped(1000000));
    CHECK(o.Set("max_phases", 2) == 0 && !o.Capped(1) && o.Capped(2) && o.Capped(3));

    std::printf("bipartite host checks passed\n");
    return 0;
}
