// tests/host/spgemm_check.hip -- the host side of the sparse product without a GPU: SpgemmOptions (app/spgemm/spgemm_enactor.hpp) parses
// the options and holds the bound against count_limit; the __host__ __device__ functions of app/spgemm/spgemm_functor.hpp choose the
// regime of a row from its products, size the LDS of a launch and the workgroup slots of the GLOBAL regime, saturate the bound and
// refuse what int32 does not address.  What the table shares with 4-cycle counting and similarity -- TableSize, the three table options
// on their own -- is pinned in tests/host/table_check.hip.  Every expectation follows from a formula in those headers.
// Built with -Xarch_host -fsanitize=address,undefined by tests/test_spgemm_host.py; makes no HIP call.
#include <climits>
#include <cstdio>
#include <cstdlib>

#include <gunrock/gunrock_mi355x.h>

#include <gunrock/app/spgemm/spgemm_enactor.hpp>

using namespace gunrock::app::spgemm;

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #x);   \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main()
{
    SpgemmOptions o;
    // parsing: 1 for a name nobody knows, -1 for a value out of range, a NaN or what no integer holds
    const double nan = std::strtod("nan", nullptr);
    CHECK(o.Set("nope", 1) == 1);
    CHECK(o.Set("right", 3) == -1 && o.Set("right", -1) == -1 && o.Set("right", nan) == -1 && o.Set("right", SPGEMM_GIVEN) == 0 &&
          o.Set("right", SPGEMM_SELF) == 0);
    CHECK(o.Set("strategy", 5) == -1 && o.Set("strategy", -1) == -1 && o.Set("strategy", SPGEMM_GLOBAL) == 0 && o.Set("strategy", SPGEMM_AUTO) == 0);
    CHECK(o.Set("pattern_only", 2) == -1 && o.Set("pattern_only", -1) == -1 && o.Set("pattern_only", 1) == 0 && o.Set("pattern_only", 0) == 0);
    CHECK(o.Set("lane_max", 65) == -1 && o.Set("lane_max", -1) == -1 && o.Set("lane_max", 1e300) == -1);
    CHECK(o.Set("count_limit", 0) == -1 && o.Set("count_limit", 1e19) == -1 && o.Set("count_limit", nan) == -1);
    CHECK(o.Set("table_slots", 96) == -1 && o.Set("table_slots", 32) == -1 && o.Set("table_slots", 2048) == -1);
    CHECK(o.Set("block_slots", 128) == -1 && o.Set("block_slots", 16384) == -1 && o.Set("block_slots", -1e300) == -1);
    CHECK(o.Set("scratch_mib", 0) == -1 && o.Set("scratch_mib", kMaxScratchMib + 1) == -1);
    // a refused value leaves the option as it was
    CHECK(o.right == SPGEMM_SELF && o.strategy == SPGEMM_AUTO && o.pattern_only == 0 && o.lane_max == kLaneMax && o.count_limit == kCountLimit &&
          o.table.table_slots == kTableSlots && o.table.block_slots == kBlockSlots && o.table.scratch_mib == kScratchMib);
    // the header's codes
    CHECK(GRX_SPGEMM_TOO_LARGE == kSpgemmTooLarge && GRX_SPGEMM_OVERFLOW == kSpgemmOverflow && GRX_SPGEMM_OVERFLOW == GRX_C4_OVERFLOW);
    CHECK(GRX_SPGEMM_SELF == 0 && GRX_SPGEMM_TRANSPOSE == 1 && GRX_SPGEMM_GIVEN == 2 && GRX_SPGEMM_GLOBAL == 4);

    // the regimes under the defaults: w <= 64 | <= 1024 / 2 | <= 8192 / 2 | the rest
    CHECK(o.RegimeOf(0) == SPGEMM_LANE && o.RegimeOf(64) == SPGEMM_LANE && o.RegimeOf(65) == SPGEMM_WAVE && o.RegimeOf(512) == SPGEMM_WAVE);
    CHECK(o.RegimeOf(513) == SPGEMM_BLOCK && o.RegimeOf(4096) == SPGEMM_BLOCK && o.RegimeOf(4097) == SPGEMM_GLOBAL &&
          o.RegimeOf(2147483647LL) == SPGEMM_GLOBAL);
    // ... and under the smallest tables: the borders at 8, 32 and 128; a forced regime is a floor; the regime never falls as w grows
    CHECK(o.Set("lane_max", 8) == 0 && o.Set("table_slots", 64) == 0 && o.Set("block_slots", 256) == 0);
    for (long long w = 0; w < 400; ++w) {
        const int want = w <= 8 ? SPGEMM_LANE : w <= 32 ? SPGEMM_WAVE : w <= 128 ? SPGEMM_BLOCK : SPGEMM_GLOBAL;
        CHECK(o.RegimeOf(w) == want);
        for (int s = SPGEMM_AUTO; s <= SPGEMM_GLOBAL; ++s) {
            SpgemmOptions f = o;
            f.strategy = s;
            const int floor = s <= SPGEMM_LANE ? want : (want > s ? want : s);
            CHECK(f.RegimeOf(w) == floor);
            CHECK(f.RegimeOf(w) <= f.RegimeOf(w + 1));
        }
        if (want == SPGEMM_WAVE || want == SPGEMM_BLOCK) {  // the table holds 2 w: it never fills; whole waves sort and scan it
            const int slots = want == SPGEMM_WAVE ? 64 : 256, size = TableSize(w, slots);
            CHECK(size >= 2 * w && (size & (size - 1)) == 0 && size >= kMinTableSlots && size <= slots && size % 64 == 0);
        }
    }
    CHECK(o.Set("lane_max", 0) == 0 && o.RegimeOf(0) == SPGEMM_LANE && o.RegimeOf(1) == SPGEMM_WAVE);

    // LDS: twelve bytes a slot with values (the int key, the int64 sum), four without; the default workgroup table is 96 KiB of 160
    SpgemmOptions d;
    CHECK(SlotBytes(true) == 12 && SlotBytes(false) == 4);
    CHECK(d.SmallLdsBytes(true) == 49152 && d.SmallLdsBytes(false) == 16384 && d.BlockLdsBytes(true) == 98304 && d.BlockLdsBytes(false) == 32768);
    CHECK(kMaxBlockLdsBytes == 98304 && kMaxBlockLdsBytes <= 160 * 1024 && o.SmallLdsBytes(true) == 12 * 4 * 64 && o.BlockLdsBytes(true) == 12 * 256);
    // the GLOBAL regime's slots: cols sums and a bit per column in 64-bit words; min(grid, scratch / slot), at least 1
    CHECK(BitmapWords(0) == 0 && BitmapWords(1) == 1 && BitmapWords(64) == 1 && BitmapWords(65) == 2 && SlotWords(65) == 67 && SlotWords(0) == 0);
    CHECK(d.Slots(1024, 1024) == 1024 && d.Slots(1024, 1 << 20) == 126 && d.Slots(1024, 2147483647LL) == 1 && d.Slots(1, 10) == 1 && d.Slots(0, 10) == 1);
    CHECK(d.Slots(1024, 0) == 1024);
    CHECK(d.Set("scratch_mib", 1) == 0 && d.Slots(1024, 140000) == 1 && d.Slots(1 << 20, 65) == (1 << 20) / (8 * 67) && d.Slots(1024, 65) == 1024);
    CHECK(d.Set("scratch_mib", kMaxScratchMib) == 0 && d.Slots(1LL << 40, 1) == (65536LL << 20) / 16);

    // the bound saturates and never wraps
    CHECK(SatAdd(1, 2) == 3 && SatAdd(kSaturated, 1) == kSaturated && SatAdd(kSaturated - 1, 1) == kSaturated && SatAdd(kSaturated, kSaturated) == kSaturated);
    CHECK(SatMul(0, kSaturated) == 0 && SatMul(kSaturated, 0) == 0 && SatMul(3, 5) == 15 && SatMul(1LL << 31, 1LL << 31) == (1LL << 62));
    CHECK(SatMul(1LL << 32, 1LL << 31) == kSaturated && SatMul(kSaturated, 2) == kSaturated && SatMul(3037000500LL, 3037000500LL) == kSaturated);
    CHECK(SatMul(3037000499LL, 3037000499LL) == 3037000499LL * 3037000499LL);
    CHECK(Abs64(INT_MIN) == 2147483648LL && Abs64(-1) == 1 && Abs64(0) == 0 && Abs64(INT_MAX) == 2147483647LL);
    // count_limit: refused from the limit on, the default 2^62
    CHECK(!d.Overflows(0) && !d.Overflows((1LL << 62) - 1024) && d.Overflows(1LL << 62) && d.Overflows(kSaturated));
    CHECK(d.Set("count_limit", 100) == 0 && !d.Overflows(99) && d.Overflows(100) && d.Set("count_limit", kCountLimit) == 0 && !d.Overflows(100));

    // what int32 addresses
    CHECK(Fits(0, 0) && Fits(2147483647LL, 2147483647LL) && !Fits(2147483648LL, 0) && !Fits(0, 2147483648LL) && !Fits(-1, 0) && !Fits(0, -1));
    CHECK(!Fits(1LL << 40, 1) && !Fits(1, 1LL << 40));
    std::puts("spgemm host checks passed");
    return 0;
}
