// tests/host/sample_check.hip -- the host side of the neighbourhood sampling without a GPU: SampleOptions (app/sample/sample_enactor.hpp)
// parses the options and the fanouts and picks the strategy of AUTO; ValidFanout, WholeRow, PickCount, GroupWidth, FloydCandidate and
// FloydPicks (app/sample/sample_functor.hpp) are the __host__ __device__ functions the kernels sample with.  The picks are the literals
// tests/test_sample_cpu.py pins; every other expectation follows from a formula of the definition.  Built with -Xarch_host
// -fsanitize=address,undefined by tests/test_sample_host.py; makes no HIP call.
#include <cstdio>
#include <cstdlib>

#include <gunrock/app/sample/sample_enactor.hpp>

using namespace gunrock::app::sample;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

static bool Picks(unsigned long long seed, int v, int hop, int d, int f, const int *want)
{
    int got[kMaxFanout];
    FloydPicks(seed, v, hop, d, f, got);
    for (int s = 0; s < f; ++s)
        if (got[s] != want[s]) return false;
    return true;
}

int main()
{
    SampleOptions o;
    // parsing: 1 for a name nobody knows, -1 for a value out of range, a NaN or what no integer holds
    const double nan = std::strtod("nan", nullptr);
    CHECK(o.Set("nope", 1, true) == 1);
    CHECK(o.Set("strategy", 3, true) == -1 && o.Set("strategy", -1, true) == -1 && o.Set("strategy", nan, true) == -1);
    CHECK(o.Set("seed", -1, true) == -1 && o.Set("seed", 9007199254740992.0, true) == -1 && o.Set("seed", 0.5, true) == -1 && o.Set("seed", -1e300, true) == -1);
    CHECK(o.Set("replace", 2, true) == -1 && o.Set("replace", -1, true) == -1);
    CHECK(o.Set("edge_limit", 0, true) == -1 && o.Set("edge_limit", 2147483648.0, true) == -1 && o.Set("edge_limit", 1e300, true) == -1);
    CHECK(o.Set("long_row", 7, true) == -1 && o.Set("long_row", nan, true) == -1 && o.Set("eids", 2, true) == -1 && o.Set("eids", -1, true) == -1);
    // weighted sampling without replacement is refused, in either order of the two options
    CHECK(o.Set("weighted", 1, true) == -1 && o.weighted == 0);
    CHECK(o.Set("replace", 1, true) == 0 && o.Set("weighted", 1, false) == -1 && o.Set("weighted", 2, true) == -1 && o.Set("weighted", 1, true) == 0);
    CHECK(o.Set("replace", 0, true) == -1 && o.replace == 1 && o.weighted == 1);
    CHECK(o.Set("weighted", 0, true) == 0 && o.Set("replace", 0, true) == 0);
    // a refused value leaves the option as it was: the defaults
    CHECK(o.strategy == SAMPLE_AUTO && o.seed == 0 && o.replace == 0 && o.weighted == 0 && o.edge_limit == 2147483647ll && o.long_row == 4096 &&
          o.eids == 1 && o.fanouts.empty());
    CHECK(o.Set("seed", 9007199254740991.0, true) == 0 && o.seed == 9007199254740991ull && o.Set("edge_limit", 1, true) == 0 && o.edge_limit == 1 &&
          o.Set("edge_limit", 2147483647.0, true) == 0 && o.Set("long_row", 8, true) == 0 && o.long_row == 8 && o.Set("long_row", 1e300, true) == 0 &&
          o.long_row == (1 << 30) && o.Set("eids", 0, true) == 0 && o.eids == 0);

    // the fanouts: -1 or 1 .. 64, for 1 .. 16 hops; a refused list leaves the one before
    const int good[16] = {-1, 1, 64, 5, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2};
    const int zero[2] = {5, 0}, above[1] = {65}, below[3] = {1, 2, -2};
    int many[17];
    for (int &f : many) f = 1;
    CHECK(o.SetFanouts(3, good) == 0 && o.fanouts.size() == 3 && o.fanouts[0] == -1 && o.fanouts[2] == 64);
    CHECK(o.SetFanouts(0, good) == -1 && o.SetFanouts(17, many) == -1 && o.SetFanouts(-1, good) == -1 && o.SetFanouts(1, nullptr) == -1);
    CHECK(o.SetFanouts(2, zero) == -1 && o.SetFanouts(1, above) == -1 && o.SetFanouts(3, below) == -1 && o.fanouts.size() == 3);
    CHECK(o.SetFanouts(16, good) == 0 && o.fanouts.size() == 16 && o.SetFanouts(16, many) == 0 && o.SetFanouts(1, good) == 0 && o.fanouts.size() == 1);
    CHECK(ValidFanout(-1) && ValidFanout(1) && ValidFanout(64) && !ValidFanout(0) && !ValidFanout(65) && !ValidFanout(-2));

    // AUTO takes GROUP, and LANE with replacement from kLaneMinSeeds seeds on; a forced strategy stays
    SampleOptions a;
    CHECK(a.Strategy(1) == SAMPLE_GROUP && a.Strategy(kLaneMinSeeds) == SAMPLE_GROUP && a.Strategy(2147483647) == SAMPLE_GROUP);
    CHECK(a.Set("replace", 1, false) == 0 && a.Strategy(1) == SAMPLE_GROUP && a.Strategy(kLaneMinSeeds - 1) == SAMPLE_GROUP &&
          a.Strategy(kLaneMinSeeds) == SAMPLE_LANE && a.Strategy(2147483647) == SAMPLE_LANE);
    CHECK(a.Set("strategy", SAMPLE_GROUP, false) == 0 && a.Strategy(kLaneMinSeeds) == SAMPLE_GROUP && a.Set("strategy", SAMPLE_LANE, false) == 0 &&
          a.Strategy(1) == SAMPLE_LANE && a.Set("replace", 0, false) == 0 && a.Strategy(1) == SAMPLE_LANE &&
          a.Set("strategy", SAMPLE_AUTO, false) == 0 && a.Strategy(kLaneMinSeeds) == SAMPLE_GROUP);

    // the group width: the power of two with f <= g <= 64
    CHECK(GroupWidth(1) == 1 && GroupWidth(2) == 2 && GroupWidth(3) == 4 && GroupWidth(4) == 4 && GroupWidth(5) == 8 && GroupWidth(8) == 8 &&
          GroupWidth(9) == 16 && GroupWidth(16) == 16 && GroupWidth(17) == 32 && GroupWidth(32) == 32 && GroupWidth(33) == 64 && GroupWidth(64) == 64);
    for (int f = 1; f <= kMaxFanout; ++f) {
        const int g = GroupWidth(f);
        CHECK(g >= f && g <= 64 && (g & (g - 1)) == 0 && (g == 1 || g / 2 < f) && 64 % g == 0);
    }
    CHECK(GroupWidth(kAllNeighbours) == kCopyGroup && 64 % kCopyGroup == 0);

    // the counts: d under -1; min(d, f) without replacement; f or nothing with it
    CHECK(PickCount(0, -1, 0, 1) == 0 && PickCount(700, -1, 0, 1) == 700 && PickCount(700, -1, 1, 0) == 700);
    CHECK(PickCount(0, 5, 0, 1) == 0 && PickCount(4, 5, 0, 1) == 4 && PickCount(5, 5, 0, 1) == 5 && PickCount(6, 5, 0, 1) == 5 && PickCount(2147483647, 64, 0, 1) == 64);
    CHECK(PickCount(0, 5, 1, 1) == 0 && PickCount(1, 5, 1, 1) == 5 && PickCount(9, 5, 1, 1) == 5 && PickCount(9, 5, 1, 0) == 0 && PickCount(1, 64, 1, 7) == 64);
    CHECK(WholeRow(9, -1, 0) && WholeRow(9, -1, 1) && WholeRow(4, 5, 0) && WholeRow(5, 5, 0) && !WholeRow(6, 5, 0) && !WholeRow(4, 5, 1) && !WholeRow(0, 5, 1));

    // Floyd's subset against the pinned picks: one collision, none, two
    const int p0[4] = {2, 0, 8, 3}, p1[4] = {2, 0, 7, 5}, p2[6] = {2, 4, 3, 0, 7, 5};
    CHECK(Picks(7, 5, 0, 10, 4, p0) && Picks(7, 5, 2, 10, 4, p1) && Picks(1, 0, 1, 9, 6, p2));
    CHECK(FloydCandidate(7, 5, 0, 2, 10, 4) != 8 && FloydCandidate(7, 5, 2, 2, 10, 4) == 7);  // slot 2: moved by the rule, and not
    // a candidate of slot s is a position of 0 .. d - f + s; the picks are distinct, whatever the row
    for (int d = 65; d <= 100; d += 5) {
        int picks[kMaxFanout];
        FloydPicks(20261020, d, 3, d, 64, picks);
        for (int s = 0; s < 64; ++s) {
            CHECK(FloydCandidate(20261020, d, 3, s, d, 64) >= 0 && FloydCandidate(20261020, d, 3, s, d, 64) <= d - 64 + s && picks[s] >= 0 && picks[s] < d);
            for (int j = 0; j < s; ++j) CHECK(picks[j] != picks[s]);
        }
    }
    // the draw is rw's, with (walk, step, t) = (v, hop, s)
    CHECK(Draw(1, 2, 3, 4) == 13731179152291499476ull && Draw(9007199254740991ull, 2147483647, 15, 63) == gunrock::app::rw::Draw(9007199254740991ull, 2147483647ull, 15, 63));
    CHECK(DistinctVertices(good + 1, 2, 65) && !DistinctVertices(good + 1, 2, 64) && !DistinctVertices(good, 2, 65) && !DistinctVertices(good + 5, 2, 65));
    std::puts("sample host checks passed");
    return 0;
}
